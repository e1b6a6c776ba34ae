"""The BAI index in the C ABI, checked without a GPU: include/kiss_hip_bai.h compiles as C and as C++, both libraries export exactly
its two symbols, BAI_EXPORTED_SYMBOLS is what the header declares and shares nothing with the other lists, the ctypes mirror has the
header's size and offsets, the host entry refuses what the header refuses and answers a file without records before it touches a
device, and the index is opt-in in Python."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bai_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_bai.h")
REPORT = ("records", "bam_bytes", "bai_bytes", "chunks", "bins", "windows", "mapped", "unmapped_placed", "no_coor", "bad", "first_bad",
          "ms_total", "ms_record", "ms_window", "ms_sort", "ms_emit")
COUNTS = {"kiss_hip_bai_dev": 13, "kiss_hip_bai_host": 12}


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.BAI_EXPORTED_SYMBOLS) == sorted(COUNTS)
    others = (_lib.EXPORTED_SYMBOLS + _lib.SAM_EXPORTED_SYMBOLS + _lib.BAM_EXPORTED_SYMBOLS + _lib.READS_EXPORTED_SYMBOLS + _lib.MD_EXPORTED_SYMBOLS
              + _lib.INSERT_EXPORTED_SYMBOLS + _lib.PILEUP_EXPORTED_SYMBOLS + _lib.DEFLATE_EXPORTED_SYMBOLS + _lib.BAM_SORT_EXPORTED_SYMBOLS)
    assert not set(syms) & set(others)
    assert not [s for s in syms if re.match(r"kiss_hip_(bam_sort|bgzf|fmi_bam)", s)]   # (the prefixes the other ABI tests own)
    assert '#include "kiss_hip_bam_sort.h"' in text
    assert int(re.search(r"#define KISS_HIP_BAI_PSEUDO_BIN (\d+)u", text).group(1)) == _lib.BAI_PSEUDO_BIN == M.PSEUDO_BIN == 37450
    assert _lib.BAI_MAX_END == M.MAX_END == 1 << 29 and "KISS_HIP_BAI_MAX_END (1u << 29)" in text
    assert "bai" not in open(os.path.join(ROOT, "include", "kiss_hip_bam_sort.h")).read()
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.HOOKS_LIB_PATH if hooks else _lib.LIB_PATH]).decode()
        assert sorted(re.findall(r"\bT (kiss_hip_bai\w*)", out)) == syms
        assert not re.findall(r"\bT (\w*bai\w*)", out.replace("kiss_hip_bai_dev", "").replace("kiss_hip_bai_host", ""))
        for s, count in COUNTS.items():
            assert getattr(lib, s).restype is ctypes.c_int and len(getattr(lib, s).argtypes) == count, s
            params = re.search(s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
            assert len(params.split(",")) == count, s


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirror_matches_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_bai_report, %s));' % f for f in REPORT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_bai.h"\n'
                   'int main(void){printf("%zu ", sizeof(kiss_hip_bai_report));' + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.BaiReport) == got[0] == 112
    assert tuple(f for f, _ in _lib.BaiReport._fields_) == REPORT
    assert [getattr(_lib.BaiReport, f).offset for f in REPORT] == got[1:]


def test_the_host_entry_refuses_bad_arguments_and_answers_no_record_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint8)
    ri = np.array([0, 40], np.uint64)
    out = np.full(64, 7, np.uint8)

    def index(n=40, records=1, cap=64, bam=z.ctypes.data, idx=ri.ctypes.data, dst=out.ctypes.data, n_ref=1, bb=0, base=0, report=True):
        rep = _lib.BaiReport()
        rc = lib.kiss_hip_bai_host(bam, n, idx, records, n_ref, bb, None, base, dst, cap, ctypes.byref(rep) if report else None, 0)
        return rc, int(rep.records), int(rep.bam_bytes), int(rep.bai_bytes)

    assert index(bam=None)[0] == _lib.KISS_HIP_E_INVALID and index(idx=None)[0] == _lib.KISS_HIP_E_INVALID
    assert index(dst=None)[0] == _lib.KISS_HIP_E_INVALID
    assert index(bb=65506)[0] == _lib.KISS_HIP_E_INVALID
    assert index(records=0, n=40)[0] == _lib.KISS_HIP_E_INVALID                  # bytes without records
    assert index(records=1 << 32, n=1 << 40)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    assert index(n_ref=1 << 31)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    assert index(base=1 << 48)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    assert np.all(out == 7)
    # no record: the empty index, sized and then filled, without a device
    assert index(records=0, n=0, bam=None, n_ref=3, cap=0, dst=None) == (_lib.KISS_HIP_E_INVALID, 0, 0, 40)
    assert index(records=0, n=0, bam=None, n_ref=3, cap=39) == (_lib.KISS_HIP_E_INVALID, 0, 0, 40) and np.all(out == 7)
    assert index(records=0, n=0, bam=None, n_ref=3, cap=64, report=False)[0] == 0
    assert out[:40].tobytes() == b"BAI\1" + struct.pack("<i", 3) + bytes(32) == M.build(b"", [0], 3)["bai"] and np.all(out[40:] == 7)
    assert index(records=0, n=0, bam=None, n_ref=0, cap=16) == (0, 0, 0, 16) and out[:16].tobytes() == b"BAI\1" + bytes(12)
    # the device entry looks at its arguments before it looks at the ctx
    assert lib.kiss_hip_bai_dev(None, None, 0, None, 0, 0, 0, None, 0, None, 0, None, None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_bai_dev(None, None, 0, ri.ctypes.data, 0, 0, 0, None, 0, out.ctypes.data, 64, None, None) == _lib.KISS_HIP_E_INVALID  # (no ctx)


def test_the_index_is_opt_in_everywhere():
    import kiss_amd.bam_writer as W
    import kiss_amd.batches as batches
    import kiss_amd.fm_index as fm
    for name in ("bam_index", "bam_index_dev", "write_bam"):
        assert callable(getattr(W, name)), name
    sig = inspect.signature(W.write_bam)
    assert sig.parameters["bai"].default is None and sig.parameters["sort"].default is False
    assert list(inspect.signature(W.bam_index).parameters) == ["bam", "rec_index", "n_ref", "block_bytes", "block_index", "file_base", "device", "hooks"]
    assert list(inspect.signature(W.bam_index_dev).parameters) == ["lib", "ctx", "device", "d_bam", "n", "d_rec_index", "records", "n_ref", "block_bytes",
                                                                  "d_block_index", "file_base", "stream"]
    # a batch does not know where its blocks will stand in a file: map and map_file take no keyword for an index
    for f in (fm.FMIndex.map, fm.FMIndex.map_pairs, batches.map_file):
        assert not [p for p in inspect.signature(f).parameters if "index" in p and "bam" in p]
    for kw in (dict(bai=True), dict(bai="x.bai", compress=True)):
        with pytest.raises(ValueError, match="sort=True"):
            W.write_bam("never.bam", None, "no such file", None, ref_names=["r"], bounds=[0, 5], version="X", **kw)
    assert not os.path.exists("never.bam")
    got = W.bam_index(b"", [0], 3)                                                # (no record: no device)
    assert got["bai"] == M.build(b"", [0], 3)["bai"] and got["report"]["bai_bytes"] == 40 and got["report"]["records"] == 0
    with pytest.raises(ValueError):
        W.bam_index(b"", [0], 3, block_bytes=65506)
