"""The select call in the C ABI, checked without a GPU: the symbols are exported by both libraries, the ctypes mirrors have the
header's sizes and offsets, the flag macros their values, and the Python defaults are the model's."""
import ctypes

import pytest

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi_select_dev", "kiss_hip_fmi_select_host")


def _offset_from_header(struct_name, field):
    return _sizeof_from_header("char[__builtin_offsetof(%s, %s)]" % (struct_name, field))


def test_symbols_are_exported_and_the_prototypes_load():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_select_dev.argtypes) == 14 and len(lib.kiss_hip_fmi_select_host.argtypes) == 13
    import kiss_amd.fm_index as fm
    assert callable(fm.FMIndex.map)
    assert callable(kiss_amd.select_alignments) and callable(kiss_amd.select_params)
    assert kiss_amd.load().kiss_hip_version() == 103


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.Hit) == _sizeof_from_header("kiss_hip_hit") == 32
    assert ctypes.sizeof(_lib.SelectParams) == _sizeof_from_header("kiss_hip_select_params") == 20
    assert ctypes.sizeof(_lib.SelectReport) == _sizeof_from_header("kiss_hip_select_report") == 96
    for mirror, name in ((_lib.Hit, "kiss_hip_hit"), (_lib.SelectParams, "kiss_hip_select_params"),
                         (_lib.SelectReport, "kiss_hip_select_report")):
        for field, _ in mirror._fields_:
            assert getattr(mirror, field).offset == _offset_from_header(name, field), (name, field)
    assert [f for f, _ in _lib.Hit._fields_] == list(kiss_amd.fm_select.HIT_FIELDS)
    assert kiss_amd.fm_select.HIT_DTYPE.itemsize == 32


def test_flags_and_defaults_are_the_documented_ones():
    from kiss_amd import fm_select
    from tests import fm_select_model as sm
    assert fm_select.HIT_REVERSE == sm.HIT_REVERSE == _sizeof_from_header("char[KISS_HIP_HIT_REVERSE]") == 1
    assert fm_select.HIT_SECONDARY == sm.HIT_SECONDARY == _sizeof_from_header("char[KISS_HIP_HIT_SECONDARY]") == 2
    assert fm_select.HIT_SUPPLEMENTARY == sm.HIT_SUPPLEMENTARY == _sizeof_from_header("char[KISS_HIP_HIT_SUPPLEMENTARY]") == 4
    assert fm_select.SELECT_DEFAULTS == kiss_amd.SELECT_DEFAULTS == sm.DEFAULTS == dict(min_score=30, overlap=128, mapq_coef=120,
                                                                                      mapq_max=60, max_hits=0)
    assert fm_select.SELECT_LIMITS == sm.LIMITS
    assert tuple(fm_select.HIT_FIELDS) == tuple(sm.HIT_FIELDS)
    p = fm_select.select_params(overlap=256, mapq_coef=65535, mapq_max=255, max_hits=7)
    assert (p.min_score, p.overlap, p.mapq_coef, p.mapq_max, p.max_hits) == (30, 256, 65535, 255, 7)


@pytest.mark.parametrize("bad", (dict(overlap=257), dict(mapq_coef=65536), dict(mapq_max=256), dict(min_score=-1), dict(max_hits=1 << 32)))
def test_select_params_refuses_values_out_of_range(bad):
    with pytest.raises(ValueError):
        kiss_amd.select_params(**bad)


def test_select_params_refuses_unknown_names():
    with pytest.raises(TypeError):
        kiss_amd.select_params(band=3)
