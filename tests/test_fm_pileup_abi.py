"""The pileup call in the C ABI, checked without a GPU: the header compiles as C and as C++, both libraries export both
symbols, the ctypes mirrors have the sizes and the offsets of include/kiss_hip_pileup.h, PILEUP_EXPORTED_SYMBOLS is what the
header declares, the feature is opt-in everywhere, and the host entry refuses what the header refuses before it touches a
device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib, fm_pileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_pileup.h")
REPORT = ("items", "bad", "filtered", "unmapped", "counted", "columns", "alt_columns", "deleted_bases", "insertions", "clipped",
          "ms_total", "ms_check", "ms_walk", "reserved_")
PARAMS = ("min_mapq", "skip_flags", "proper_only", "reserved_")


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.PILEUP_EXPORTED_SYMBOLS) == ["kiss_hip_fmi_pileup_dev", "kiss_hip_fmi_pileup_host"]
    assert not set(syms) & set(_lib.EXPORTED_SYMBOLS) and not set(syms) & set(_lib.MD_EXPORTED_SYMBOLS)
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in syms:
            assert hasattr(lib, s), s
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_pileup_dev.argtypes) == 22 and len(lib.kiss_hip_fmi_pileup_host.argtypes) == 22
    for name, count in (("kiss_hip_fmi_pileup_dev", 22), ("kiss_hip_fmi_pileup_host", 22)):
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == count, name


@pytest.mark.parametrize("compiler, ext", (("gcc", "c"), ("g++", "cpp")))
def test_the_header_compiles_as_c_and_cpp_and_the_mirrors_match_it(tmp_path, compiler, ext):
    src = tmp_path / ("s." + ext)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_pileup_report, %s));' % f for f in REPORT)
    prints += "".join('printf("%%zu ", offsetof(kiss_hip_pileup_params, %s));' % f for f in PARAMS)
    prints += 'printf("%u %u %u %u ", KISS_HIP_PILEUP_PLANES, KISS_HIP_PILEUP_COV, KISS_HIP_PILEUP_ALT_N, KISS_HIP_PILEUP_INS);'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_pileup.h"\nint main(void){'
                   'printf("%zu %zu ", sizeof(kiss_hip_pileup_report), sizeof(kiss_hip_pileup_params));' + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.PileupReport) == got[0] == 96 and ctypes.sizeof(_lib.PileupParams) == got[1] == 16
    assert tuple(f for f, _ in _lib.PileupReport._fields_) == REPORT and tuple(f for f, _ in _lib.PileupParams._fields_) == PARAMS
    assert [getattr(_lib.PileupReport, f).offset for f in REPORT] == got[2:2 + len(REPORT)]
    assert [getattr(_lib.PileupParams, f).offset for f in PARAMS] == got[2 + len(REPORT):2 + len(REPORT) + 4]
    assert got[-4:] == [8, 0, 5, 7] == [len(fm_pileup.PLANES), fm_pileup.COV, fm_pileup.ALT_N, fm_pileup.INS]


def test_the_pileup_is_opt_in_and_the_module_has_its_entries():
    import kiss_amd.fm_index as fm
    assert "pileup" not in inspect.signature(fm.FMIndex.map).parameters  # (taken out of the keywords, as sam= is)
    assert fm_pileup.PLANES == ("cov", "alt_a", "alt_c", "alt_g", "alt_t", "alt_n", "del", "ins")
    for name in ("pileup", "pileup_dev", "pileup_params", "base_counts"):
        assert callable(getattr(fm_pileup, name)), name
    sig = inspect.signature(fm_pileup.pileup).parameters
    assert list(sig)[:6] == ["text", "reads", "alignments", "chain_index", "cigar", "cigar_index"]
    assert [sig[k].default for k in ("both_strands", "hits", "pairs", "lo", "hi", "counts", "device", "hooks")] == [False, None, None, 0, None, None,
                                                                                                                0, None]


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    ptr = z.ctypes.data
    guard = np.full(8 * 10 + 2, 0xA5A5A5A5, np.uint32)
    names = ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "hits", "pairs", "params", "counts")

    def run(Q=1, n=1000, both=0, H=0, P=0, lo=0, hi=10, null=("hits", "pairs"), ridx=ptr, par=(0, 2, 0, 0), on_device=0):
        a = dict.fromkeys(names, ptr)
        a["ridx"] = ridx
        a["counts"] = guard[1:].ctypes.data
        params = _lib.PileupParams(*par)
        a["params"] = ctypes.pointer(params)
        for k in null:
            a[k] = None
        rc = lib.kiss_hip_fmi_pileup_host(a["text"], n, a["reads"], a["ridx"], Q, both, a["alns"], a["cidx"], a["cigar"], a["oidx"], a["hits"], H,
                                          a["pairs"], P, a["params"], lo, hi, a["counts"], on_device, 0, None, 0)
        assert (guard == 0xA5A5A5A5).all(), "counts was written"
        return rc

    for k in ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "params", "counts"):
        assert run(null=("hits", "pairs", k)) == _lib.KISS_HIP_E_INVALID, k
    assert run(null=("hits",), P=1) == _lib.KISS_HIP_E_INVALID          # pairs without hits
    assert run(lo=11, hi=10) == _lib.KISS_HIP_E_INVALID
    assert run(hi=1001) == _lib.KISS_HIP_E_INVALID
    assert run(par=(0, 2, 0, 1)) == _lib.KISS_HIP_E_INVALID             # reserved_
    assert run(par=(256, 2, 0, 0)) == _lib.KISS_HIP_E_INVALID
    assert run(par=(0, 8, 0, 0)) == _lib.KISS_HIP_E_INVALID
    assert run(n=_lib.MAX_N + 1) == _lib.KISS_HIP_E_UNSUPPORTED
    assert run(Q=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED
    assert run(Q=1 << 30, both=1) == _lib.KISS_HIP_E_UNSUPPORTED        # V = 2^31
    assert run(H=1 << 32, null=("pairs",)) == _lib.KISS_HIP_E_UNSUPPORTED
    assert run(H=1, P=1 << 31, null=()) == _lib.KISS_HIP_E_UNSUPPORTED  # 2 P = 2^32
    assert run(Q=2) == _lib.KISS_HIP_E_INVALID                          # (a read_index of zeros: reads of length 0)
    down = np.array([0, 5, 3], np.uint64)
    assert run(Q=2, ridx=down.ctypes.data) == _lib.KISS_HIP_E_INVALID
