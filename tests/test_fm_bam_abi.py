"""The BAM calls in the C ABI, checked without a GPU: the header compiles as C and as C++, both libraries export the four symbols,
the ctypes mirrors have the sizes and the offsets of include/kiss_hip_bam.h, BAM_EXPORTED_SYMBOLS is what the header declares,
bam is opt-in in Python, and the host entries refuse what the header refuses before they touch a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_bam.h")
REPORT = ("records", "bam_bytes", "unmapped_records", "longest", "bad", "first_bad", "ms_total", "ms_count", "ms_emit", "reserved_")
FRAMING = ("blocks", "out_bytes", "ms_total", "reserved_")
COUNTS = {"kiss_hip_fmi_bam_dev": 9, "kiss_hip_fmi_bam_host": 8, "kiss_hip_bgzf_dev": 9, "kiss_hip_bgzf_host": 8}


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.BAM_EXPORTED_SYMBOLS) == sorted(COUNTS)
    assert not set(syms) & set(_lib.EXPORTED_SYMBOLS + _lib.SAM_EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s, count in COUNTS.items():
            assert getattr(lib, s).restype is ctypes.c_int and len(getattr(lib, s).argtypes) == count, s
    for s, count in COUNTS.items():
        params = re.search(s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == count, s
        assert re.search(r"\bT %s\b" % s, out), s
    assert (_lib.BGZF_BLOCK_DEFAULT, _lib.BGZF_BLOCK_MAX, _lib.BGZF_OVERHEAD, _lib.BGZF_EOF_BYTES) == tuple(
        int(re.search(r"#define KISS_HIP_BGZF_%s (\d+)u" % k, text).group(1)) for k in ("BLOCK_DEFAULT", "BLOCK_MAX", "OVERHEAD", "EOF_BYTES"))
    assert _lib.BGZF_BLOCK_MAX + _lib.BGZF_OVERHEAD == 1 << 16  # (BSIZE is a u16 that holds the bytes of the block less one)


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirrors_match_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_bam_report, %s));' % f for f in REPORT)
    prints += 'printf("%zu ", sizeof(kiss_hip_bgzf_report));'
    prints += "".join('printf("%%zu ", offsetof(kiss_hip_bgzf_report, %s));' % f for f in FRAMING)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_bam.h"\nint main(void){printf("%zu ", sizeof(kiss_hip_bam_report));'
                   + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    n = len(REPORT)
    assert ctypes.sizeof(_lib.BamReport) == got[0] == 64
    assert tuple(f for f, _ in _lib.BamReport._fields_) == REPORT
    assert [getattr(_lib.BamReport, f).offset for f in REPORT] == got[1:1 + n]
    assert ctypes.sizeof(_lib.BgzfReport) == got[1 + n] == 24
    assert tuple(f for f, _ in _lib.BgzfReport._fields_) == FRAMING
    assert [getattr(_lib.BgzfReport, f).offset for f in FRAMING] == got[2 + n:]


def test_bam_is_opt_in_everywhere():
    import kiss_amd.bam_writer as W
    import kiss_amd.fm_index as fm
    assert "bam_writer" not in vars(kiss_amd) or kiss_amd.bam_writer is W  # (a module, never a name of the package's own)
    assert not [k for k in vars(kiss_amd) if "bam" in k.lower() and k != "bam_writer"]
    given = dict(min_score=3)
    assert fm.FMIndex._sam_options(given, True, None) is None and given == dict(min_score=3)
    given = dict(bam=True, names=["a"], ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert given == dict(overlap=1) and so["bam"] and not so["sam"] and so["ref_names"] == ["r"] and so["bounds"].tolist() == [0, 5]
    so = fm.FMIndex._sam_options(dict(sam=True, bam=True, ref_names=["r"]), True, [0, 5])
    assert so["bam"] and so["sam"]
    assert fm.FMIndex._sam_options(dict(sam=True, ref_names=["r"]), True, [0, 5])["bam"] is False
    for kw, cigar, bounds in ((dict(bam=True, ref_names=["r"]), False, [0, 5]), (dict(bam=True), True, [0, 5]),
                              (dict(bam=True, ref_names=["r"]), True, None), (dict(bam=True, ref_names=["r", "s"]), True, [0, 5])):
        with pytest.raises(ValueError):
            fm.FMIndex._sam_options(kw, cigar, bounds)
    for name in ("bam_header", "bam_records", "bam_records_dev", "bgzf", "bgzf_dev", "write_bam"):
        assert callable(getattr(W, name)), name
    assert len(W.BGZF_EOF) == 28
    assert W.bgzf_bytes(0) == 0 and W.bgzf_bytes(0, eof=True) == 28 and W.bgzf_bytes(65281) == 65281 + 62 and W.bgzf_bytes(3, 1) == 3 + 93
    with pytest.raises(ValueError):
        W.bgzf(b"abc", 65506)


def test_the_host_entries_refuse_bad_arguments_before_they_touch_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    one = np.array([0, 4], np.uint64)
    out = np.full(8, 7, np.uint64)

    def bam(null=(), Q=1, C=0, R=1, cap=0, bam_ptr=None, read_rec=out.ctypes.data, **other):
        ptrs = dict.fromkeys(_lib.SamInput.POINTERS, z.ctypes.data)
        ptrs.update(read_index=one.ctypes.data, pairs=None, source=None, md=None, qual=None)
        ptrs.update(other)
        for k in null:
            ptrs[k] = None
        inp = kiss_amd.sam_writer.sam_input(ptrs, Q, C, R, 0)
        rep = _lib.BamReport()
        return lib.kiss_hip_fmi_bam_host(ctypes.byref(inp), bam_ptr, cap, None, 0, read_rec, ctypes.byref(rep), 0)

    for k in ("reads", "read_index", "names", "name_off", "name_len", "alns", "cigar", "cigar_index", "hits", "hit_index", "ref_names",
              "ref_name_index", "bounds"):
        assert bam(null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    assert bam(R=0) == _lib.KISS_HIP_E_INVALID and bam(R=0, Q=0) == _lib.KISS_HIP_E_INVALID   # BAM needs records
    assert bam(read_rec=None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi_bam_host(None, None, 0, None, 0, out.ctypes.data, None, 0) == _lib.KISS_HIP_E_INVALID
    assert bam(cap=5) == _lib.KISS_HIP_E_INVALID
    assert bam(md=z.ctypes.data, null=("md_index",)) == _lib.KISS_HIP_E_INVALID
    assert bam(Q=3, pairs=z.ctypes.data) == _lib.KISS_HIP_E_INVALID
    assert bam(Q=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED and bam(C=1 << 32) == _lib.KISS_HIP_E_UNSUPPORTED
    assert bam(Q=2, read_index=z.ctypes.data) == _lib.KISS_HIP_E_INVALID
    assert bam(Q=0) == 0 and out[0] == 0 and out[1] == 7

    def bgzf(n, bb, eof, cap, data=z.ctypes.data, dst=out.ctypes.data):
        rep = _lib.BgzfReport()
        return lib.kiss_hip_bgzf_host(data, n, bb, eof, dst, cap, ctypes.byref(rep), 0), int(rep.blocks), int(rep.out_bytes)

    assert bgzf(10, 65506, 0, 64)[0] == _lib.KISS_HIP_E_INVALID and bgzf(10, 1 << 31, 0, 64)[0] == _lib.KISS_HIP_E_INVALID
    assert bgzf(10, 4, 1, 0, dst=None) == (_lib.KISS_HIP_E_INVALID, 3, 10 + 93 + 28)           # the totals, nothing written
    assert bgzf(10, 0, 0, 40) == (_lib.KISS_HIP_E_INVALID, 1, 41)
    assert bgzf(10, 0, 0, 64, data=None)[0] == _lib.KISS_HIP_E_INVALID and bgzf(10, 0, 0, 64, dst=None)[0] == _lib.KISS_HIP_E_INVALID
    assert bgzf(0, 0, 0, 0, data=None, dst=None) == (0, 0, 0)                                  # nothing to write, no device needed
    assert np.all(out[1:] == 7)
