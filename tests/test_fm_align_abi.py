"""The align call in the C ABI, checked without a GPU: the symbols are exported by both libraries, the ctypes mirrors have the
header's sizes and offsets, and the Python defaults are the model's."""
import ctypes

import pytest

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi_align_dev", "kiss_hip_fmi_align_host")


def _offset_from_header(struct_name, field):
    return _sizeof_from_header("char[__builtin_offsetof(%s, %s)]" % (struct_name, field))


def test_symbols_are_exported():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
    import kiss_amd.fm_index as fm
    assert callable(fm.FMIndex.align)
    assert callable(kiss_amd.align_chains) and callable(kiss_amd.align_params)
    assert kiss_amd.load().kiss_hip_version() == 103


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.Aln) == _sizeof_from_header("kiss_hip_aln") == 48
    assert ctypes.sizeof(_lib.AlignParams) == _sizeof_from_header("kiss_hip_align_params") == 20
    assert ctypes.sizeof(_lib.AlignReport) == _sizeof_from_header("kiss_hip_align_report") == 72
    for mirror, name in ((_lib.Aln, "kiss_hip_aln"), (_lib.AlignParams, "kiss_hip_align_params"),
                         (_lib.AlignReport, "kiss_hip_align_report")):
        for field, _ in mirror._fields_:
            assert getattr(mirror, field).offset == _offset_from_header(name, "del" if field == "del" else field), (name, field)
    assert [f for f, _ in _lib.Aln._fields_] == list(kiss_amd.fm_align.ALN_FIELDS)
    assert kiss_amd.fm_align.ALN_DTYPE.itemsize == 48


def test_python_defaults_are_the_documented_ones():
    from kiss_amd import fm_align
    from tests import fm_align_model as am
    assert fm_align.ALIGN_DEFAULTS == kiss_amd.ALIGN_DEFAULTS == am.DEFAULTS == dict(match=1, mismatch=4, gap_open=6, gap_extend=1, band=32)
    assert fm_align.ALIGN_MAX_BAND == am.MAX_BAND == _sizeof_from_header("char[KISS_HIP_ALIGN_MAX_BAND]") == 1024
    assert fm_align.ALIGN_CELLS_PER_N == am.CELLS_PER_N == _sizeof_from_header("char[KISS_HIP_ALIGN_CELLS_PER_N]")
    assert fm_align.ALN_BAND_TOO_WIDE == am.BAND_TOO_WIDE == _sizeof_from_header("char[KISS_HIP_ALN_BAND_TOO_WIDE]")
    assert tuple(fm_align.ALN_FIELDS) == tuple(am.FIELDS)
    p = fm_align.align_params(band=7, mismatch=2)
    assert (p.match, p.mismatch, p.gap_open, p.gap_extend, p.band) == (1, 2, 6, 1, 7)
    p = fm_align.align_params(match=65535, mismatch=65535, gap_open=65535, gap_extend=65535, band=(1 << 31) - 1)
    assert (p.match, p.band) == (65535, (1 << 31) - 1)


@pytest.mark.parametrize("bad", (dict(match=0), dict(match=65536), dict(mismatch=65536), dict(gap_open=65536), dict(gap_extend=65536),
                                 dict(band=1 << 31), dict(mismatch=-1), dict(band=-1)))
def test_align_params_refuses_values_out_of_range(bad):
    with pytest.raises(ValueError):
        kiss_amd.align_params(**bad)


def test_align_params_refuses_unknown_names():
    with pytest.raises(TypeError):
        kiss_amd.align_params(min_score=3)
