"""The MD call in the C ABI, checked without a GPU: both libraries export both symbols, the ctypes mirror has the size and
the offsets of include/kiss_hip_md.h, MD_EXPORTED_SYMBOLS is what the header declares, the Python defaults leave every
existing result alone, and the host entry refuses what the header refuses before it touches a device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

import kiss_amd
from kiss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_md.h")
FIELDS = ("items", "bad", "md_bytes", "mismatch_columns", "deleted_bases", "longest", "ms_total", "ms_count", "ms_emit", "reserved_")


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.MD_EXPORTED_SYMBOLS) == ["kiss_hip_fmi_md_dev", "kiss_hip_fmi_md_host"]
    assert not set(syms) & set(_lib.EXPORTED_SYMBOLS) and not set(syms) & set(_lib.READS_EXPORTED_SYMBOLS)
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in syms:
            assert hasattr(lib, s), s
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_md_dev.argtypes) == 19 and len(lib.kiss_hip_fmi_md_host.argtypes) == 18
        assert lib.kiss_hip_version() == 103
    # the prototypes of the header have as many parameters
    for name, count in (("kiss_hip_fmi_md_dev", 19), ("kiss_hip_fmi_md_host", 18)):
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == count, name


def test_the_ctypes_mirror_matches_the_header(tmp_path):
    src = tmp_path / "s.c"
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_md_report, %s));' % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_md.h"\nint main(void){printf("%zu ", sizeof(kiss_hip_md_report));'
                   + prints + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.MdReport) == got[0] == 64
    assert tuple(f for f, _ in _lib.MdReport._fields_) == FIELDS
    assert [getattr(_lib.MdReport, f).offset for f in FIELDS] == got[1:]


def test_md_is_opt_in_everywhere():
    import kiss_amd.fm_index as fm
    assert inspect.signature(fm.FMIndex.map).parameters["want_md"].default is False
    assert inspect.signature(fm.FMIndex.map_pairs).parameters["want_md"].default is False
    assert inspect.signature(fm.FMIndex.map).parameters["want_cigar"].default is True
    assert callable(kiss_amd.md_tags) and callable(kiss_amd.md_strings) and callable(kiss_amd.fm_md.md_dev)
    assert kiss_amd.md_strings(np.frombuffer(b"100A0", np.uint8), [0, 2, 2, 5]) == ["10", "", "0A0"]


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    ptr = z.ctypes.data
    names = ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "hits", "md", "midx", "counts")

    def md(Q=1, n=1000, both=0, H=0, cap=0, null=("hits", "md", "counts"), ridx=ptr):
        a = dict.fromkeys(names, ptr)
        a["ridx"] = ridx
        for k in null:
            a[k] = None
        return lib.kiss_hip_fmi_md_host(a["text"], n, a["reads"], a["ridx"], Q, both, a["alns"], a["cidx"], a["cigar"], a["oidx"], a["hits"], H,
                                        a["md"], a["midx"], a["counts"], cap, None, 0)

    for k in ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "midx"):
        assert md(null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    assert md(cap=5) == _lib.KISS_HIP_E_INVALID                      # room named, no md
    assert md(n=_lib.MAX_N + 1) == _lib.KISS_HIP_E_UNSUPPORTED
    assert md(Q=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED
    assert md(Q=1 << 30, both=1) == _lib.KISS_HIP_E_UNSUPPORTED      # V = 2^31
    assert md(H=1 << 32, null=("md", "counts")) == _lib.KISS_HIP_E_UNSUPPORTED
    assert md(Q=2) == _lib.KISS_HIP_E_INVALID                        # (a read_index of zeros: reads of length 0)
    down = np.array([0, 5, 3], np.uint64)
    assert md(Q=2, ridx=down.ctypes.data) == _lib.KISS_HIP_E_INVALID
    # no items: nothing to do and no device needed
    ridx = np.array([0, 4], np.uint64)
    one = np.ones(1, np.uint64)
    rep = _lib.MdReport()
    assert lib.kiss_hip_fmi_md_host(ptr, 1000, ptr, ridx.ctypes.data, 1, 0, ptr, ptr, ptr, ptr, None, 0, None, one.ctypes.data, None, 0,
                                    ctypes.byref(rep), 0) == 0
    assert one[0] == 0 and rep.items == 0 and rep.md_bytes == 0
