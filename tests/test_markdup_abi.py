"""The duplicate marking in the C ABI, checked without a GPU: include/kiss_hip_markdup.h compiles as C and as C++, both libraries
export exactly its two symbols, MARKDUP_EXPORTED_SYMBOLS is what the header declares and shares nothing with the other lists, the
ctypes mirror has the header's size and offsets, the entries refuse what the header refuses before they touch a device, and the
marking is opt-in in Python."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_markdup.h")
REPORT = ("records", "templates", "pairs", "fragments", "unmapped_templates", "ambiguous", "dup_pairs", "dup_fragments", "dup_records", "bad",
          "first_bad", "ms_total", "ms_record", "ms_class", "ms_sort", "ms_mark")
COUNTS = {"kiss_hip_bam_markdup_dev": 10, "kiss_hip_bam_markdup_host": 9}


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.MARKDUP_EXPORTED_SYMBOLS) == sorted(COUNTS)
    others = (_lib.EXPORTED_SYMBOLS + _lib.SAM_EXPORTED_SYMBOLS + _lib.BAM_EXPORTED_SYMBOLS + _lib.READS_EXPORTED_SYMBOLS + _lib.MD_EXPORTED_SYMBOLS
              + _lib.INSERT_EXPORTED_SYMBOLS + _lib.PILEUP_EXPORTED_SYMBOLS + _lib.DEFLATE_EXPORTED_SYMBOLS + _lib.BAM_SORT_EXPORTED_SYMBOLS
              + _lib.BAI_EXPORTED_SYMBOLS)
    assert not set(syms) & set(others)
    assert '#include "kiss_hip_bam_sort.h"' in text
    assert int(re.search(r"#define KISS_HIP_MARKDUP_MIN_QUAL_DEFAULT (\d+)u", text).group(1)) == _lib.MARKDUP_MIN_QUAL_DEFAULT == 15
    assert int(re.search(r"#define KISS_HIP_MARKDUP_MAX_N_REF (0x[0-9A-F]+)u", text).group(1), 16) == _lib.MARKDUP_MAX_N_REF == (1 << 30) - 1
    assert int(re.search(r"#define KISS_HIP_BAM_FLAG_DUP (0x[0-9A-F]+)u", text).group(1), 16) == _lib.BAM_FLAG_DUP == 0x400
    # (the headers it stands on declare what they declared: their own tests pin their symbols)
    for name in ("kiss_hip_bam.h", "kiss_hip_bam_sort.h", "kiss_hip_bai.h"):
        assert "markdup" not in open(os.path.join(ROOT, "include", name)).read(), name
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.HOOKS_LIB_PATH if hooks else _lib.LIB_PATH]).decode()
        assert sorted(re.findall(r"\bT (kiss_hip_bam_markdup\w*)", out)) == syms
        for s, count in COUNTS.items():
            assert getattr(lib, s).restype is ctypes.c_int and len(getattr(lib, s).argtypes) == count, s
            params = re.search(s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
            assert len(params.split(",")) == count, s


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirror_matches_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_markdup_report, %s));' % f for f in REPORT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_markdup.h"\n'
                   'int main(void){printf("%zu ", sizeof(kiss_hip_markdup_report));' + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.MarkdupReport) == got[0] == 11 * 8 + 5 * 4 + 4
    assert tuple(f for f, _ in _lib.MarkdupReport._fields_) == REPORT
    assert [getattr(_lib.MarkdupReport, f).offset for f in REPORT] == got[1:]


def test_the_entries_refuse_bad_arguments_before_they_touch_a_device():
    lib = kiss_amd.load()
    z = np.full(64, 3, np.uint8)
    ri = np.array([0, 40], np.uint64)
    dup = np.full(4, 7, np.uint8)

    def mark(n=40, records=1, bam=z.ctypes.data, index=ri.ctypes.data, n_ref=1, report=True):
        rep = _lib.MarkdupReport()
        rc = lib.kiss_hip_bam_markdup_host(bam, n, index, records, n_ref, 15, dup.ctypes.data, ctypes.byref(rep) if report else None, 0)
        return rc, int(rep.records)

    assert mark(bam=None)[0] == _lib.KISS_HIP_E_INVALID and mark(index=None)[0] == _lib.KISS_HIP_E_INVALID
    assert mark(index=None, report=False)[0] == _lib.KISS_HIP_E_INVALID
    assert mark(records=0, n=40)[0] == _lib.KISS_HIP_E_INVALID                    # bytes without records
    assert mark(records=1 << 32, n=1 << 40) == (_lib.KISS_HIP_E_UNSUPPORTED, 1 << 32)
    assert mark(n_ref=1 << 30) == (_lib.KISS_HIP_E_UNSUPPORTED, 1)                 # an end is one u64
    assert mark(n=(1 << 54) + 1) == (_lib.KISS_HIP_E_UNSUPPORTED, 1)               # a score stays below 2^63
    assert mark(records=0, n=0, bam=None) == (0, 0)                                # nothing to mark, no device needed
    assert mark(records=0, n=0, bam=None, n_ref=0, report=False)[0] == 0
    assert np.all(z == 3) and np.all(dup == 7)
    # the device entry looks at its arguments before it looks at the ctx
    assert lib.kiss_hip_bam_markdup_dev(None, None, 0, None, 0, 0, 15, None, None, None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_bam_markdup_dev(None, None, 0, ri.ctypes.data, 1 << 32, 0, 15, None, None, None) == _lib.KISS_HIP_E_UNSUPPORTED
    assert lib.kiss_hip_bam_markdup_dev(None, None, 0, ri.ctypes.data, 0, 0, 15, None, None, None) == _lib.KISS_HIP_E_INVALID  # (no ctx)


def test_markdup_is_opt_in_everywhere():
    import kiss_amd.bam_writer as W
    import kiss_amd.fm_index as fm
    assert not [k for k in vars(kiss_amd) if "markdup" in k.lower()]
    given = dict(bam=True, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert so["bam_markdup"] is None and given == dict(overlap=1)
    given = dict(bam=True, bam_markdup=True, bam_sort=True, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert so["bam_markdup"] == dict(min_qual=15) and so["bam_sort"] is True and given == dict(overlap=1)
    so = fm.FMIndex._sam_options(dict(bam=True, bam_markdup=dict(min_qual=0), ref_names=["r"]), True, [0, 5])
    assert so["bam_markdup"] == dict(min_qual=0)
    for kw in (dict(bam_markdup=True), dict(sam=True, bam_markdup=True, ref_names=["r"]), dict(bam=True, bam_markdup=dict(min_q=3), ref_names=["r"]),
               dict(bam=True, bam_markdup=dict(min_qual=-1), ref_names=["r"])):
        with pytest.raises(ValueError):
            fm.FMIndex._sam_options(kw, True, [0, 5])
    for name in ("bam_markdup", "bam_markdup_dev", "bam_marked", "markdup_options", "write_bam"):
        assert callable(getattr(W, name)), name
    assert W.markdup_options(None) is None and W.markdup_options(False) is None and W.markdup_options(True) == dict(min_qual=15)
    with pytest.raises(ValueError, match="write_bam"):
        next(kiss_amd.batches.map_file(None, "no such file", None, bam=True, bam_markdup=True))
    for how in (dict(markdup=True), dict(markdup=dict(min_qual=20), compress=True), dict(markdup=True, sort=False)):
        with pytest.raises(ValueError, match="sort=True"):
            W.write_bam("no such file", None, "no reads", None, ref_names=["r"], bounds=[0, 5], **how)
    with pytest.raises(ValueError, match="min_qual"):
        W.write_bam("no such file", None, "no reads", None, ref_names=["r"], bounds=[0, 5], sort=True, markdup=dict(quality=3))
    got = W.bam_markdup(b"", [0], 3)                                             # (no record: no device)
    assert got["bam"].size == 0 and got["dup"].size == 0 and got["report"]["records"] == 0 and got["report"]["templates"] == 0
