"""The seed call in the C ABI, checked without a GPU: the symbols are exported by both libraries and the ctypes mirrors have
the header's sizes."""
import ctypes

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi_seeds_dev", "kiss_hip_fmi_seeds_host")


def test_symbols_are_exported():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
    import kiss_amd.fm_index as fm
    assert callable(fm.FMIndex.seeds)


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.FmiSeed) == _sizeof_from_header("kiss_hip_fmi_seed") == 16
    assert ctypes.sizeof(_lib.FmiSeedReport) == _sizeof_from_header("kiss_hip_fmi_seed_report")
    assert _lib.FmiSeed.sa_end.offset == 12
    assert _lib.FmiSeedReport.max_ms.offset == 72 and _lib.FmiSeedReport.ms_total.offset == 80
    assert _lib.FmiSeedReport.ms_sort.offset == 96
