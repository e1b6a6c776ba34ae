"""The SAM call in the C ABI, checked without a GPU: the header compiles as C and as C++, both libraries export both symbols, the
ctypes mirrors have the sizes and the offsets of include/kiss_hip_sam.h, SAM_EXPORTED_SYMBOLS is what the header declares, the
Python defaults leave every existing result alone, and the host entry refuses what the header refuses before it touches a
device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_sam.h")
REPORT = ("lines", "sam_bytes", "unmapped_lines", "longest", "bad", "first_bad", "ms_total", "ms_count", "ms_emit", "reserved_")
INPUT = ("reads", "read_index", "qual", "names", "name_off", "name_len", "alns", "cigar", "cigar_index", "hits", "hit_index", "pairs", "source",
         "md", "md_index", "ref_names", "ref_name_index", "bounds", "Q", "C", "R", "first_alns")


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.SAM_EXPORTED_SYMBOLS) == ["kiss_hip_fmi_sam_dev", "kiss_hip_fmi_sam_host"]
    assert not set(syms) & set(_lib.EXPORTED_SYMBOLS) and not set(syms) & set(_lib.MD_EXPORTED_SYMBOLS)
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in syms:
            assert hasattr(lib, s), s
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_sam_dev.argtypes) == 9 and len(lib.kiss_hip_fmi_sam_host.argtypes) == 8
    for name, count in (("kiss_hip_fmi_sam_dev", 9), ("kiss_hip_fmi_sam_host", 8)):
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == count, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for s in syms:
        assert re.search(r"\bT %s\b" % s, out), s


@pytest.mark.parametrize("compiler,suffix", [("gcc", "c"), ("g++", "cpp")])
def test_the_header_compiles_and_the_ctypes_mirrors_match_it(tmp_path, compiler, suffix):
    src = tmp_path / ("s." + suffix)
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_sam_report, %s));' % f for f in REPORT)
    prints += 'printf("%zu ", sizeof(kiss_hip_sam_input));'
    prints += "".join('printf("%%zu ", offsetof(kiss_hip_sam_input, %s));' % f for f in INPUT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_sam.h"\nint main(void){printf("%zu ", sizeof(kiss_hip_sam_report));'
                   + prints + "return 0;}\n")
    subprocess.check_call([compiler, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    n = len(REPORT)
    assert ctypes.sizeof(_lib.SamReport) == got[0] == 64
    assert tuple(f for f, _ in _lib.SamReport._fields_) == REPORT
    assert [getattr(_lib.SamReport, f).offset for f in REPORT] == got[1:1 + n]
    assert ctypes.sizeof(_lib.SamInput) == got[1 + n] == 8 * len(INPUT)
    assert tuple(f for f, _ in _lib.SamInput._fields_) == INPUT == _lib.SamInput.POINTERS + ("Q", "C", "R", "first_alns")
    assert [getattr(_lib.SamInput, f).offset for f in INPUT] == got[2 + n:]


def test_sam_is_opt_in_everywhere():
    import kiss_amd.fm_index as fm
    # (the new keywords ride in the keyword dicts: the recorded signatures of map and map_pairs stay what they were)
    assert "select_params" in inspect.signature(fm.FMIndex.map).parameters and "pair_params" in inspect.signature(fm.FMIndex.map_pairs).parameters
    given = dict(min_score=3)
    assert fm.FMIndex._sam_options(given, True, None) is None and given == dict(min_score=3)
    given = dict(sam=True, names=["a"], qual=None, ref_names=["r"], overlap=1)
    so = fm.FMIndex._sam_options(given, True, [0, 5])
    assert given == dict(overlap=1) and so["names"] == ["a"] and so["ref_names"] == ["r"] and so["bounds"].tolist() == [0, 5]
    assert "sam_lines" not in vars(kiss_amd) and kiss_amd.sam_writer.__name__ == "kiss_amd.sam_writer"
    assert callable(kiss_amd.sam_writer.sam_lines) and callable(kiss_amd.sam_writer.sam_lines_dev) and callable(kiss_amd.sam_header)
    assert kiss_amd.sam_writer.default_names(4) == [b"0", b"1", b"2", b"3"] and kiss_amd.sam_writer.default_names(4, True) == [b"0", b"0", b"1", b"1"]
    raw, off, ln = kiss_amd.sam_writer.pack_names(["ab", b"", "cde"])
    assert raw.tobytes() == b"abcde" and off.tolist() == [0, 2, 2] and ln.tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        fm.FMIndex._sam_options(dict(names=["a"]), True, None)      # names without sam
    with pytest.raises(ValueError):
        fm.FMIndex._sam_options(dict(sam=True), False, None)       # sam without the ops
    with pytest.raises(ValueError):
        fm.FMIndex._sam_options(dict(sam=True), True, [0, 5, 9])   # bounds without ref_names


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    one = np.array([0, 4], np.uint64)
    out = np.full(8, 7, np.uint64)

    def sam(null=(), Q=1, C=0, R=0, cap=0, sam_ptr=None, read_line=out.ctypes.data, **other):
        ptrs = dict.fromkeys(_lib.SamInput.POINTERS, z.ctypes.data)
        ptrs.update(read_index=one.ctypes.data, pairs=None, source=None, md=None, qual=None)
        ptrs.update(other)
        for k in null:
            ptrs[k] = None
        inp = kiss_amd.sam_writer.sam_input(ptrs, Q, C, R, 0)
        rep = _lib.SamReport()
        return lib.kiss_hip_fmi_sam_host(ctypes.byref(inp), sam_ptr, cap, None, 0, read_line, ctypes.byref(rep), 0)

    for k in ("reads", "read_index", "names", "name_off", "name_len", "alns", "cigar", "cigar_index", "hits", "hit_index"):
        assert sam(null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    assert sam(read_line=None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi_sam_host(None, None, 0, None, 0, out.ctypes.data, None, 0) == _lib.KISS_HIP_E_INVALID
    assert sam(cap=5) == _lib.KISS_HIP_E_INVALID                                  # room named, no sam
    assert sam(md=z.ctypes.data, null=("md_index",)) == _lib.KISS_HIP_E_INVALID
    for k in ("ref_names", "ref_name_index", "bounds"):
        assert sam(R=1, null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    assert sam(Q=3, pairs=z.ctypes.data) == _lib.KISS_HIP_E_INVALID               # Q odd with pairs
    assert sam(Q=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED
    assert sam(C=1 << 32) == _lib.KISS_HIP_E_UNSUPPORTED
    assert sam(Q=2, read_index=z.ctypes.data) == _lib.KISS_HIP_E_INVALID          # reads of length 0
    down = np.array([0, 5, 3], np.uint64)
    assert sam(Q=2, read_index=down.ctypes.data) == _lib.KISS_HIP_E_INVALID
    up = np.array([0, 5, 9], np.uint64)
    assert sam(Q=2, read_index=up.ctypes.data, hit_index=down.ctypes.data) == _lib.KISS_HIP_E_INVALID
    # no reads: nothing to do and no device needed
    assert sam(Q=0) == 0 and out[0] == 0 and out[1] == 7
    with pytest.raises(TypeError):
        kiss_amd.sam_writer.sam_input({"read": 1}, 0, 0, 0, 0)
