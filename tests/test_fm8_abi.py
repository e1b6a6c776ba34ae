"""The byte FM-index in the C ABI, checked without a GPU: the symbols are exported, the ctypes mirrors have the header's
sizes, and the host-only size arithmetic equals the model's."""
import ctypes

import pytest

import kiss_amd
from kiss_amd import _lib
from tests import fm8_model
from tests.test_abi import _sizeof_from_header

SYMBOLS = ("kiss_hip_fmi8_sizes_for", "kiss_hip_fmi8_build_dev", "kiss_hip_fmi8_build_host", "kiss_hip_fmi8_query_dev",
           "kiss_hip_fmi8_query_host")


def test_symbols_are_exported():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
    assert kiss_amd.FMIndexBytes is kiss_amd.fm_index_bytes.FMIndexBytes


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.Fmi8View) == _sizeof_from_header("kiss_hip_fmi8_view")
    assert ctypes.sizeof(_lib.Fmi8Sizes) == _sizeof_from_header("kiss_hip_fmi8_sizes")
    assert ctypes.sizeof(_lib.Fmi8Report) == _sizeof_from_header("kiss_hip_fmi8_report")
    assert _lib.Fmi8View.b_occ.offset == ctypes.sizeof(_lib.Fmi8View) - 8
    assert _lib.Fmi8Report.ms_sort.offset == ctypes.sizeof(_lib.Fmi8Report) - 4


@pytest.mark.parametrize("sigma", (1, 4, 256))
@pytest.mark.parametrize("sa_intv", (1, 4, 32))
def test_sizes_for_equals_the_model(sa_intv, sigma):
    lib = kiss_amd.load()
    for n in (0, 1, 2, 254, 255, 256, 257, 65534, 65535, 65536, 65537, 3 * 2 ** 20 + 5):
        z = _lib.Fmi8Sizes()
        assert lib.kiss_hip_fmi8_sizes_for(n, sa_intv, sigma, ctypes.byref(z)) == 0
        assert z.as_dict() == fm8_model.sizes(n, sa_intv, sigma), (n, sa_intv, sigma)


def test_sizes_for_limits():
    lib = kiss_amd.load()
    z = _lib.Fmi8Sizes()
    for bad in (0, 33):
        assert lib.kiss_hip_fmi8_sizes_for(10, bad, 4, ctypes.byref(z)) == _lib.KISS_HIP_E_UNSUPPORTED
    assert lib.kiss_hip_fmi8_sizes_for(10, 4, 257, ctypes.byref(z)) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi8_sizes_for(_lib.MAX_N + 1, 4, 4, ctypes.byref(z)) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi8_sizes_for(10, 4, 4, None) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi8_sizes_for(0, 4, 0, ctypes.byref(z)) == 0 and z.n_sa == 1 and z.occ1_entries == 0
