"""The pair call in the C ABI, checked without a GPU: the symbols are exported by both libraries, the ctypes mirrors have the
header's sizes and offsets, the flag macros their values, and the Python defaults and limits are the model's."""
import ctypes

import pytest

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi_pair_dev", "kiss_hip_fmi_pair_host")


def _offset_from_header(struct_name, field):
    return _sizeof_from_header("char[__builtin_offsetof(%s, %s)]" % (struct_name, field))


def test_symbols_are_exported_and_the_prototypes_load():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_pair_dev.argtypes) == 10 and len(lib.kiss_hip_fmi_pair_host.argtypes) == 9
    import kiss_amd.fm_index as fm
    assert callable(fm.FMIndex.map_pairs)
    assert callable(kiss_amd.pair_hits) and callable(kiss_amd.pair_params)


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.Pair) == _sizeof_from_header("kiss_hip_pair") == 40
    assert ctypes.sizeof(_lib.PairParams) == _sizeof_from_header("kiss_hip_pair_params") == 28
    assert ctypes.sizeof(_lib.PairReport) == _sizeof_from_header("kiss_hip_pair_report") == 88
    for mirror, name in ((_lib.Pair, "kiss_hip_pair"), (_lib.PairParams, "kiss_hip_pair_params"), (_lib.PairReport, "kiss_hip_pair_report")):
        for field, _ in mirror._fields_:
            assert getattr(mirror, field).offset == _offset_from_header(name, field), (name, field)
    assert [f for f, _ in _lib.Pair._fields_] == list(kiss_amd.fm_pair.PAIR_FIELDS)
    assert kiss_amd.fm_pair.PAIR_DTYPE.itemsize == 40


def test_flags_defaults_and_limits_are_the_documented_ones():
    from kiss_amd import fm_pair
    from tests import fm_pair_model as pm
    for name, value in (("PROPER", 1), ("MATE1_MAPPED", 2), ("MATE2_MAPPED", 4), ("SAME_REF", 8), ("PROMOTED1", 16), ("PROMOTED2", 32),
                        ("BAD_INPUT", 64)):
        assert getattr(fm_pair, "PAIR_" + name) == getattr(pm, name) == _sizeof_from_header("char[KISS_HIP_PAIR_%s]" % name) == value
    assert fm_pair.PAIR_NONE == pm.NONE == 0xFFFFFFFF
    assert _sizeof_from_header("char[KISS_HIP_PAIR_NONE == 0xFFFFFFFFu ? 7 : 1]") == 7
    assert fm_pair.PAIR_DEFAULTS == kiss_amd.PAIR_DEFAULTS == pm.DEFAULTS == dict(ins_min=0, ins_max=1000, ins_mean=400, pen_coef=8, pen_max=20,
                                                                              mapq_coef=120, mapq_max=60)
    assert fm_pair.PAIR_LIMITS == pm.LIMITS == dict(pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255)
    assert tuple(fm_pair.PAIR_FIELDS) == tuple(pm.PAIR_FIELDS)
    p = fm_pair.pair_params(ins_min=7, ins_max=7, pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255)
    assert (p.ins_min, p.ins_max, p.ins_mean, p.pen_coef, p.pen_max, p.mapq_coef, p.mapq_max) == (7, 7, 400, 65535, 65535, 65535, 255)


@pytest.mark.parametrize("bad", (dict(pen_coef=65536), dict(pen_max=65536), dict(mapq_coef=65536), dict(mapq_max=256), dict(ins_min=-1),
                                 dict(ins_max=1 << 32), dict(ins_min=1001), dict(ins_min=5, ins_max=4)))
def test_pair_params_refuses_values_out_of_range(bad):
    with pytest.raises(ValueError):
        kiss_amd.pair_params(**bad)


def test_pair_params_refuses_unknown_names():
    with pytest.raises(TypeError):
        kiss_amd.pair_params(overlap=3)
