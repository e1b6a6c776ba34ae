"""The insert call in the C ABI, checked without a GPU: both libraries export both symbols, the ctypes mirrors have the sizes
and the offsets of include/kiss_hip_insert.h, INSERT_EXPORTED_SYMBOLS is what the header declares, the Python defaults leave
every existing result alone, and the host entry refuses what the header refuses before it touches a device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import fm_insert_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kiss_hip_insert.h")
PARAMS = ("min_mapq", "max_insert", "min_samples", "out_mult", "map_mult", "sd_mult")
REPORT = ("P", "unmapped", "bad_input", "low_mapq", "discordant", "too_long", "samples", "used", "flags", "q25", "q50", "q75", "mean",
          "sd", "ins_min", "ins_max", "ins_mean", "ms_total", "ms_hist", "ms_stats")


def test_symbols_are_exported_and_the_prototypes_load():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.INSERT_EXPORTED_SYMBOLS) == ["kiss_hip_fmi_insert_dev", "kiss_hip_fmi_insert_host"]
    for other in (_lib.EXPORTED_SYMBOLS, _lib.READS_EXPORTED_SYMBOLS, _lib.MD_EXPORTED_SYMBOLS):
        assert not set(syms) & set(other)
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in syms:
            assert hasattr(lib, s), s
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_insert_dev.argtypes) == 10 and len(lib.kiss_hip_fmi_insert_host.argtypes) == 9
        assert lib.kiss_hip_version() == 103
    for name, count in (("kiss_hip_fmi_insert_dev", 10), ("kiss_hip_fmi_insert_host", 9)):
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == count, name


def test_the_ctypes_mirrors_match_the_header(tmp_path):
    src = tmp_path / "s.c"
    prints = "".join('printf("%%zu ", offsetof(kiss_hip_insert_params, %s));' % f for f in PARAMS)
    prints += "".join('printf("%%zu ", offsetof(kiss_hip_insert_report, %s));' % f for f in REPORT)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_insert.h"\nint main(void){'
                   'printf("%zu %zu %u %u ", sizeof(kiss_hip_insert_params), sizeof(kiss_hip_insert_report), KISS_HIP_INSERT_MAX, '
                   'KISS_HIP_INSERT_OK);' + prints + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert ctypes.sizeof(_lib.InsertParams) == got[0] == 24
    assert ctypes.sizeof(_lib.InsertReport) == got[1] == 112
    assert (_lib.INSERT_MAX, _lib.INSERT_OK) == (got[2], got[3]) == (im.LIMITS["max_insert"], im.OK)
    assert tuple(f for f, _ in _lib.InsertParams._fields_) == PARAMS and tuple(f for f, _ in _lib.InsertReport._fields_) == REPORT
    assert [getattr(_lib.InsertParams, f).offset for f in PARAMS] + [getattr(_lib.InsertReport, f).offset for f in REPORT] == got[4:]


def test_insert_is_opt_in_and_the_parameters_are_checked():
    import kiss_amd.fm_index as fm
    assert inspect.signature(fm.FMIndex.map_pairs).parameters["insert"].default is None
    assert callable(kiss_amd.estimate_insert) and callable(kiss_amd.fm_insert.insert_dev)
    assert kiss_amd.INSERT_DEFAULTS == im.DEFAULTS and kiss_amd.fm_insert.INSERT_LIMITS == im.LIMITS
    p = kiss_amd.insert_params()
    assert {k: getattr(p, k) for k in PARAMS} == im.DEFAULTS
    assert kiss_amd.insert_params(max_insert=65535, out_mult=255, sd_mult=0).max_insert == 65535
    with pytest.raises(TypeError):
        kiss_amd.insert_params(ins_max=5)
    for bad in (dict(max_insert=0), dict(max_insert=65536), dict(out_mult=256), dict(map_mult=256), dict(sd_mult=256),
                dict(min_mapq=-1), dict(min_samples=1 << 32)):
        with pytest.raises(ValueError):
            kiss_amd.insert_params(**bad)
    with pytest.raises(ValueError):
        kiss_amd.estimate_insert(np.zeros((0, 8)), [0, 0], np.zeros((0, 12)))           # Q odd


def test_the_host_entry_refuses_bad_arguments_before_it_touches_a_device():
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    ptr = z.ctypes.data

    def call(Q=2, hidx=ptr, null=(), rep=True, **kw):
        a = dict(hits=ptr, hidx=hidx, alns=ptr, hist=None)
        for k in null:
            a[k] = None
        p = _lib.InsertParams(**dict(im.DEFAULTS, **kw))
        r = _lib.InsertReport()
        return lib.kiss_hip_fmi_insert_host(a["hits"], a["hidx"], Q, a["alns"], 1, ctypes.byref(p), a["hist"],
                                            ctypes.byref(r) if rep else None, 0), r

    for k in ("hits", "hidx", "alns"):
        assert call(null=(k,))[0] == _lib.KISS_HIP_E_INVALID, k
    assert call(rep=False)[0] == _lib.KISS_HIP_E_INVALID
    r = _lib.InsertReport()
    assert lib.kiss_hip_fmi_insert_host(ptr, ptr, 2, ptr, 1, None, None, ctypes.byref(r), 0) == _lib.KISS_HIP_E_INVALID
    assert call(Q=3)[0] == _lib.KISS_HIP_E_INVALID
    for kw in (dict(max_insert=0), dict(max_insert=65536), dict(out_mult=256), dict(map_mult=256), dict(sd_mult=256)):
        assert call(**kw)[0] == _lib.KISS_HIP_E_INVALID, kw
    assert call(Q=1 << 32)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    down = np.array([0, 5, 3], np.uint64)
    assert call(hidx=down.ctypes.data)[0] == _lib.KISS_HIP_E_INVALID
    top = np.array([0, 1, 0xFFFFFFFF], np.uint64)
    assert call(hidx=top.ctypes.data)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    # no pairs: nothing to do and no device needed
    rc, r = call(Q=0)
    assert rc == 0 and all(v == 0 for v in r.as_dict().values())
    hist = np.full(11, 7, np.uint32)
    p = _lib.InsertParams(**dict(im.DEFAULTS, max_insert=10))
    assert lib.kiss_hip_fmi_insert_host(ptr, ptr, 0, ptr, 0, ctypes.byref(p), hist.ctypes.data, ctypes.byref(r), 0) == 0
    assert not hist.any()
