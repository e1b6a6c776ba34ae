"""The compressing BGZF calls in the C ABI, checked without a GPU: include/kiss_hip_deflate.h compiles as C and as C++, both
libraries export the two symbols, the ctypes mirror has the header's size and offsets, DEFLATE_EXPORTED_SYMBOLS is what the header
declares, the host entry refuses what the header refuses before it touches a device, and bam_compress is opt-in in Python."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bam_model as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_deflate.h")
REPORT = ("blocks", "out_bytes", "stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches", "match_bytes", "ms_total", "ms_block",
          "ms_scan", "ms_copy")
COUNTS = {"kiss_hip_bgzf_deflate_dev": 11, "kiss_hip_bgzf_deflate_host": 10}


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.DEFLATE_EXPORTED_SYMBOLS) == sorted(COUNTS)
    others = (_lib.EXPORTED_SYMBOLS + _lib.SAM_EXPORTED_SYMBOLS + _lib.BAM_EXPORTED_SYMBOLS + _lib.READS_EXPORTED_SYMBOLS + _lib.MD_EXPORTED_SYMBOLS
              + _lib.INSERT_EXPORTED_SYMBOLS + _lib.PILEUP_EXPORTED_SYMBOLS)
    assert not set(syms) & set(others)
    assert '#include "kiss_hip_bam.h"' in text
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.HOOKS_LIB_PATH if hooks else _lib.LIB_PATH]).decode()
        for s, count in COUNTS.items():
            assert getattr(lib, s).restype is ctypes.c_int and len(getattr(lib, s).argtypes) == count, s
            params = re.search(s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
            assert len(params.split(",")) == count, s
            assert re.search(r"\bT %s\b" % s, out), s


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirror_matches_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_bgzf_deflate_report, %s));' % f for f in REPORT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_deflate.h"\n'
                   'int main(void){printf("%zu ", sizeof(kiss_hip_bgzf_deflate_report));' + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.BgzfDeflateReport) == got[0] == 80
    assert tuple(f for f, _ in _lib.BgzfDeflateReport._fields_) == REPORT
    assert [getattr(_lib.BgzfDeflateReport, f).offset for f in REPORT] == got[1:]


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    out = np.full(128, 7, np.uint8)
    index = np.full(8, 9, np.uint64)

    def deflate(n, bb, eof, cap, data=z.ctypes.data, dst=out.ctypes.data, idx=None, icap=0):
        rep = _lib.BgzfDeflateReport()
        rc = lib.kiss_hip_bgzf_deflate_host(data, n, bb, eof, dst, cap, idx, icap, ctypes.byref(rep), 0)
        return rc, int(rep.blocks), int(rep.out_bytes)

    bad = _lib.KISS_HIP_E_INVALID
    assert deflate(10, 65506, 0, 64)[0] == bad and deflate(10, 1 << 31, 0, 64)[0] == bad             # block_bytes
    assert deflate(10, 0, 0, 64, data=None)[0] == bad and deflate(10, 0, 0, 64, dst=None)[0] == bad  # NULLs
    assert deflate(10, 0, 0, 40) == (bad, 1, 41)                                                    # one short: the bound, nothing written
    assert deflate(10, 4, 1, 10 + 93 + 27) == (bad, 3, 10 + 93 + 28)
    assert deflate(10, 4, 1, 0, dst=None) == (bad, 3, 10 + 93 + 28)
    assert deflate(10, 4, 0, 128, idx=index.ctypes.data, icap=3)[0] == bad                          # the index one short
    assert deflate(0, 0, 0, 0, data=None, dst=None) == (0, 0, 0)                                    # nothing to do, no device
    assert np.all(out == 7) and np.all(index == 9)
    # the end-of-file block alone and block_index[0] need no device either
    assert deflate(0, 0, 1, 128, data=None, idx=index.ctypes.data, icap=1) == (0, 0, 28)
    assert out[:28].tobytes() == B.BGZF_EOF and np.all(out[28:] == 7) and index[0] == 0 and index[1] == 9


def test_bam_compress_is_opt_in_everywhere():
    import kiss_amd.bam_writer as W
    import kiss_amd.fm_index as fm
    assert not [k for k in vars(kiss_amd) if "bam" in k.lower() and k != "bam_writer"]
    given = dict(min_score=3)
    assert fm.FMIndex._sam_options(given, True, None) is None and given == dict(min_score=3)
    given = dict(bam=True, ref_names=["r"], overlap=1)
    assert fm.FMIndex._sam_options(given, True, [0, 5])["bam_compress"] is False and given == dict(overlap=1)
    given = dict(bam=True, bam_compress=True, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert so["bam"] and so["bam_compress"] is True and given == dict(overlap=1)
    for kw in (dict(bam_compress=True), dict(sam=True, bam_compress=True, ref_names=["r"])):
        with pytest.raises(ValueError):
            fm.FMIndex._sam_options(kw, True, [0, 5])
    for name in ("bgzf_deflate", "bgzf_deflate_dev"):
        assert callable(getattr(W, name)), name
    with pytest.raises(ValueError):
        W.bgzf_deflate(b"abc", 65506)
    assert W.bgzf_deflate(b"") == b"" and W.bgzf_deflate(b"", eof=True) == W.BGZF_EOF   # (no device)
