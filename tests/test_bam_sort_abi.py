"""The BAM sort in the C ABI, checked without a GPU: include/kiss_hip_bam_sort.h compiles as C and as C++, both libraries export
exactly its two symbols, BAM_SORT_EXPORTED_SYMBOLS is what the header declares and shares nothing with the other lists, the ctypes
mirror has the header's size and offsets, the host entry refuses what the header refuses before it touches a device, bam_sort is
opt-in in Python, and the headers' default bytes are what they were."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_bam_sort.h")
REPORT = ("records", "bam_bytes", "unplaced", "longest", "bad", "first_bad", "ms_total", "ms_key", "ms_sort", "ms_copy")
COUNTS = {"kiss_hip_bam_sort_dev": 12, "kiss_hip_bam_sort_host": 11}


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.BAM_SORT_EXPORTED_SYMBOLS) == sorted(COUNTS)
    others = (_lib.EXPORTED_SYMBOLS + _lib.SAM_EXPORTED_SYMBOLS + _lib.BAM_EXPORTED_SYMBOLS + _lib.READS_EXPORTED_SYMBOLS + _lib.MD_EXPORTED_SYMBOLS
              + _lib.INSERT_EXPORTED_SYMBOLS + _lib.PILEUP_EXPORTED_SYMBOLS + _lib.DEFLATE_EXPORTED_SYMBOLS)
    assert not set(syms) & set(others)
    assert '#include "kiss_hip_bam.h"' in text
    assert int(re.search(r"#define KISS_HIP_BAM_RECORD_MIN (\d+)u", text).group(1)) == _lib.BAM_RECORD_MIN == 36
    # (kiss_hip_bam.h declares what it declared: tests/test_fm_bam_abi.py pins its four symbols)
    assert "bam_sort" not in open(os.path.join(ROOT, "include", "kiss_hip_bam.h")).read()
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.HOOKS_LIB_PATH if hooks else _lib.LIB_PATH]).decode()
        assert sorted(re.findall(r"\bT (kiss_hip_bam_sort\w*)", out)) == syms
        for s, count in COUNTS.items():
            assert getattr(lib, s).restype is ctypes.c_int and len(getattr(lib, s).argtypes) == count, s
            params = re.search(s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
            assert len(params.split(",")) == count, s


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirror_matches_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_bam_sort_report, %s));' % f for f in REPORT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_bam_sort.h"\n'
                   'int main(void){printf("%zu ", sizeof(kiss_hip_bam_sort_report));' + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.BamSortReport) == got[0] == 64
    assert tuple(f for f, _ in _lib.BamSortReport._fields_) == REPORT
    assert [getattr(_lib.BamSortReport, f).offset for f in REPORT] == got[1:]


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint8)
    ri = np.array([0, 40], np.uint64)
    out = np.full(64, 7, np.uint8)
    oi = np.full(4, 9, np.uint64)
    order = np.full(4, 5, np.uint32)

    def sort(n=40, records=1, cap=64, bam=z.ctypes.data, index=ri.ctypes.data, dst=out.ctypes.data, n_ref=1, report=True):
        rep = _lib.BamSortReport()
        rc = lib.kiss_hip_bam_sort_host(bam, n, index, records, n_ref, dst, cap, oi.ctypes.data, order.ctypes.data,
                                        ctypes.byref(rep) if report else None, 0)
        return rc, int(rep.records), int(rep.bam_bytes)

    assert sort(bam=None)[0] == _lib.KISS_HIP_E_INVALID and sort(index=None)[0] == _lib.KISS_HIP_E_INVALID
    assert sort(dst=None)[0] == _lib.KISS_HIP_E_INVALID
    assert sort(cap=39) == (_lib.KISS_HIP_E_INVALID, 1, 40)                      # the totals, nothing written
    assert sort(cap=0, dst=None) == (_lib.KISS_HIP_E_INVALID, 1, 40)
    assert sort(cap=39, report=False)[0] == _lib.KISS_HIP_E_INVALID
    assert sort(records=1 << 32, n=1 << 40, cap=1 << 40)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    assert sort(records=0, n=40)[0] == _lib.KISS_HIP_E_INVALID                   # bytes without records
    assert np.all(out == 7) and np.all(oi == 9) and np.all(order == 5)
    assert sort(records=0, n=0, cap=0, bam=None, dst=None) == (0, 0, 0)          # nothing to sort, no device needed
    assert oi.tolist() == [0, 9, 9, 9] and np.all(out == 7) and np.all(order == 5)
    rep = _lib.BamSortReport()
    assert lib.kiss_hip_bam_sort_host(None, 0, ri.ctypes.data, 0, 0, None, 0, None, None, ctypes.byref(rep), 0) == 0
    # the device entry looks at its arguments before it looks at the ctx
    assert lib.kiss_hip_bam_sort_dev(None, None, 0, None, 0, 0, None, 0, None, None, None, None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_bam_sort_dev(None, None, 0, ri.ctypes.data, 0, 0, None, 0, None, None, None, None) == _lib.KISS_HIP_E_INVALID  # (no ctx)


def test_bam_sort_is_opt_in_everywhere():
    import kiss_amd.bam_writer as W
    import kiss_amd.fm_index as fm
    assert not [k for k in vars(kiss_amd) if "bam" in k.lower() and k != "bam_writer"]
    given = dict(bam=True, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert so["bam_sort"] is False and so["bam_unframed"] is False and given == dict(overlap=1)
    given = dict(bam=True, bam_sort=True, bam_compress=True, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert so["bam"] and so["bam_sort"] is True and so["bam_compress"] is True and given == dict(overlap=1)
    for kw in (dict(bam_sort=True), dict(sam=True, bam_sort=True, ref_names=["r"])):
        with pytest.raises(ValueError):
            fm.FMIndex._sam_options(kw, True, [0, 5])
    for name in ("bam_sort", "bam_sort_dev", "bam_sorted", "bam_unframed", "write_bam"):
        assert callable(getattr(W, name)), name
    with pytest.raises(ValueError, match="write_bam"):
        next(kiss_amd.batches.map_file(None, "no such file", None, bam=True, bam_sort=True))
    got = W.bam_sort(b"", [0], 3)                                               # (no record: no device)
    assert got["bam"].size == 0 and got["rec_index"].tolist() == [0] and got["order"].size == 0 and got["report"]["records"] == 0


def test_the_default_headers_are_unchanged_and_the_sort_order_is_one_word():
    import kiss_amd.bam_writer as W
    names, bounds = [b"chrA", "chrB"], [0, 100, 250]
    text = kiss_amd.sam_header(names, bounds, "9")
    assert text == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:100\n@SQ\tSN:chrB\tLN:150\n@PG\tID:kiss\tPN:kiss\tVN:9\n"
    assert W.sam_header(names, bounds, "9") == text and W.sam_header(names, bounds, "9", sort_order="unsorted") == text
    sorted_text = W.sam_header(names, bounds, "9", sort_order="coordinate")
    assert sorted_text == text.replace(b"SO:unsorted", b"SO:coordinate") and sorted_text.count(b"coordinate") == 1
    head = W.bam_header(names, bounds, "9")
    assert head == (b"BAM\1" + len(text).to_bytes(4, "little") + text + (2).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"chrA\0"
                    + (100).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"chrB\0" + (150).to_bytes(4, "little"))
    assert W.bam_header(names, bounds, "9", sort_order="unsorted") == head
    got = W.bam_header(names, bounds, "9", sort_order="coordinate")
    assert got == head.replace(b"SO:unsorted", b"SO:coordinate").replace(len(text).to_bytes(4, "little"), len(sorted_text).to_bytes(4, "little"), 1)
    for f in (W.sam_header, W.bam_header):
        with pytest.raises(ValueError):
            f(names, bounds, "9", sort_order="queryname")
