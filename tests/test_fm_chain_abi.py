"""The chain call in the C ABI, checked without a GPU: the symbols are exported by both libraries and the ctypes mirrors have
the header's sizes."""
import ctypes

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi_chain_dev", "kiss_hip_fmi_chain_host")


def test_symbols_are_exported():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
    import kiss_amd.fm_index as fm
    assert callable(fm.FMIndex.chains)
    assert callable(kiss_amd.chain_seeds)


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.Chain) == _sizeof_from_header("kiss_hip_chain") == 24
    assert ctypes.sizeof(_lib.ChainAnchor) == _sizeof_from_header("kiss_hip_chain_anchor") == 12
    assert ctypes.sizeof(_lib.ChainParams) == _sizeof_from_header("kiss_hip_chain_params") == 20
    assert ctypes.sizeof(_lib.ChainReport) == _sizeof_from_header("kiss_hip_chain_report")
    assert _lib.Chain.tend.offset == 20 and _lib.ChainAnchor.len.offset == 8 and _lib.ChainParams.min_score.offset == 16
    assert _lib.ChainReport.dp_pairs.offset == 32 and _lib.ChainReport.max_anchors.offset == 40
    assert _lib.ChainReport.ms_total.offset == 48 and _lib.ChainReport.ms_emit.offset == 60


def test_python_defaults_are_the_documented_ones():
    from kiss_amd import fm_chain
    from tests import fm_chain_model as cm
    assert fm_chain.CHAIN_DEFAULTS == cm.DEFAULTS == dict(max_gap=5000, band=500, gap_cost=2, max_lookback=64, min_score=40)
    p = fm_chain.chain_params(band=7)
    assert (p.max_gap, p.band, p.gap_cost, p.max_lookback, p.min_score) == (5000, 7, 2, 64, 40)
    for bad in (dict(max_gap=1 << 31), dict(band=1 << 31), dict(gap_cost=65536), dict(min_score=-1)):
        try:
            fm_chain.chain_params(**bad)
        except ValueError:
            continue
        raise AssertionError(bad)
