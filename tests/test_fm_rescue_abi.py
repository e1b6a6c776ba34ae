"""The rescue plan and the merge call in the C ABI, checked without a GPU: the symbols are exported by both libraries, the
ctypes mirrors have the header's sizes and offsets, the Python defaults and limits are the model's, and the parameter checks
refuse what the header refuses."""
import ctypes

import pytest

import kiss_amd
from kiss_amd import _lib
from tests.test_abi import _sizeof_from_header
from tests.test_fm_pair_abi import _offset_from_header

SYMBOLS = ("kiss_hip_fmi_rescue_dev", "kiss_hip_fmi_rescue_host", "kiss_hip_fmi_aln_merge_dev", "kiss_hip_fmi_aln_merge_host")


def test_symbols_are_exported_and_the_prototypes_load():
    for hooks in (False, True):
        lib = kiss_amd.load(hooks)
        for s in SYMBOLS:
            assert hasattr(lib, s), s
            assert s in _lib.EXPORTED_SYMBOLS
            assert getattr(lib, s).restype is ctypes.c_int
        assert len(lib.kiss_hip_fmi_rescue_dev.argtypes) == 18 and len(lib.kiss_hip_fmi_rescue_host.argtypes) == 17
        assert len(lib.kiss_hip_fmi_aln_merge_dev.argtypes) == 19 and len(lib.kiss_hip_fmi_aln_merge_host.argtypes) == 18
        assert lib.kiss_hip_version() == 103
    import inspect
    import kiss_amd.fm_index as fm
    assert inspect.signature(fm.FMIndex.map_pairs).parameters["rescue"].default is None
    assert callable(kiss_amd.plan_rescue) and callable(kiss_amd.merge_alignments) and callable(kiss_amd.rescue_params)
    assert callable(kiss_amd.fm_rescue.rescue_dev) and callable(kiss_amd.fm_rescue.merge_dev)


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.RescueParams) == _sizeof_from_header("kiss_hip_rescue_params") == 20
    assert ctypes.sizeof(_lib.RescueReport) == _sizeof_from_header("kiss_hip_rescue_report") == 80
    assert ctypes.sizeof(_lib.MergeReport) == _sizeof_from_header("kiss_hip_merge_report") == 56
    for mirror, name in ((_lib.RescueParams, "kiss_hip_rescue_params"), (_lib.RescueReport, "kiss_hip_rescue_report"),
                         (_lib.MergeReport, "kiss_hip_merge_report")):
        for field, _ in mirror._fields_:
            assert getattr(mirror, field).offset == _offset_from_header(name, field), (name, field)
    # a rescue chain is a kiss_hip_chain
    assert kiss_amd.fm_chain.CHAIN_DTYPE.itemsize == _sizeof_from_header("kiss_hip_chain") == 24


def test_defaults_and_limits_are_the_documented_ones():
    from kiss_amd import fm_rescue
    from tests import fm_rescue_model as rm
    assert fm_rescue.RESCUE_DEFAULTS == kiss_amd.RESCUE_DEFAULTS == rm.DEFAULTS == dict(ins_min=0, ins_max=1000, max_anchors=4,
                                                                                        min_anchor_score=0, max_width=960)
    assert fm_rescue.RESCUE_LIMITS["max_width"] == rm.MAX_WIDTH_TOP == _sizeof_from_header("char[KISS_HIP_ALIGN_MAX_BAND]") == 1024
    # the default piece and the default band of the align call fill the widest band exactly
    assert rm.DEFAULTS["max_width"] - 1 + 2 * kiss_amd.ALIGN_DEFAULTS["band"] + 1 == 1024
    assert fm_rescue.RESCUE_DEFAULTS["ins_min"] == kiss_amd.PAIR_DEFAULTS["ins_min"]
    assert fm_rescue.RESCUE_DEFAULTS["ins_max"] == kiss_amd.PAIR_DEFAULTS["ins_max"]
    assert tuple(f for f, _ in _lib.RescueReport._fields_)[:8] == rm.REPORT_COUNTS
    p = fm_rescue.rescue_params(ins_min=7, ins_max=7, max_anchors=0xFFFFFFFF, min_anchor_score=0xFFFFFFFF, max_width=1024)
    assert (p.ins_min, p.ins_max, p.max_anchors, p.min_anchor_score, p.max_width) == (7, 7, 0xFFFFFFFF, 0xFFFFFFFF, 1024)
    assert fm_rescue.chain_room(10, 1000, fm_rescue.rescue_params()) == 10 * 4 * 2
    assert fm_rescue.chain_room(10, 3, fm_rescue.rescue_params(ins_max=959)) == 3


@pytest.mark.parametrize("bad", (dict(max_anchors=0), dict(max_width=0), dict(max_width=1025), dict(ins_min=-1), dict(ins_max=1 << 32),
                                 dict(ins_min=1001), dict(ins_min=5, ins_max=4), dict(min_anchor_score=1 << 32)))
def test_rescue_params_refuses_values_out_of_range(bad):
    with pytest.raises(ValueError):
        kiss_amd.rescue_params(**bad)


def test_rescue_params_refuses_unknown_names():
    with pytest.raises(TypeError):
        kiss_amd.rescue_params(ins_mean=3)


def test_the_host_entries_refuse_bad_arguments_before_they_touch_a_device():
    """what the C calls check themselves: NULL pointers, Q odd, parameters out of range, the limits"""
    import numpy as np
    lib = kiss_amd.load()
    z = np.zeros(64, np.uint64)
    ptr = z.ctypes.data
    ok = _lib.RescueParams(0, 1000, 4, 0, 960)

    def plan(Q=2, params=ok, n=1000, null=(), R=0, bounds=None):
        a = dict(pairs=ptr, hits=ptr, hidx=ptr, alns=ptr, ridx=ptr, chains=ptr, cidx=ptr)
        for k in null:
            a[k] = None
        return lib.kiss_hip_fmi_rescue_host(a["pairs"], a["hits"], a["hidx"], Q, a["alns"], 0, a["ridx"], n, bounds, R,
                                            ctypes.byref(params) if params is not None else None, a["chains"], a["cidx"], None, 0, None, 0)

    for k in ("pairs", "hits", "hidx", "alns", "ridx", "chains", "cidx"):
        assert plan(null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    assert plan(params=None) == _lib.KISS_HIP_E_INVALID
    assert plan(Q=3) == _lib.KISS_HIP_E_INVALID
    assert plan(bounds=ptr, R=0) == _lib.KISS_HIP_E_INVALID
    for p in (_lib.RescueParams(5, 4, 4, 0, 960), _lib.RescueParams(0, 9, 0, 0, 960), _lib.RescueParams(0, 9, 4, 0, 0),
              _lib.RescueParams(0, 9, 4, 0, 1025)):
        assert plan(params=p) == _lib.KISS_HIP_E_INVALID
    assert plan(Q=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED
    assert plan(n=_lib.MAX_N + 1) == _lib.KISS_HIP_E_UNSUPPORTED
    assert plan(Q=2) == _lib.KISS_HIP_E_INVALID  # (a read_index of zeros: reads of length 0)
    one = np.ones(1, np.uint64)
    assert lib.kiss_hip_fmi_rescue_host(ptr, ptr, ptr, 0, ptr, 0, ptr, 1000, None, 0, ctypes.byref(ok), ptr, one.ctypes.data, None, 0, None,
                                        0) == 0 and one[0] == 0

    def merge(null=(), V=2, cig=(None, None, None, None, None, None), ocap=0):
        a = dict(alns_a=ptr, cidx_a=ptr, alns_b=ptr, cidx_b=ptr, alns=ptr, cidx=ptr)
        for k in null:
            a[k] = None
        return lib.kiss_hip_fmi_aln_merge_host(a["alns_a"], a["cidx_a"], cig[0], cig[1], a["alns_b"], a["cidx_b"], cig[2], cig[3], V,
                                               a["alns"], 0, a["cidx"], None, cig[4], cig[5], ocap, None, 0)

    for k in ("alns_a", "cidx_a", "alns_b", "cidx_b", "alns", "cidx"):
        assert merge(null=(k,)) == _lib.KISS_HIP_E_INVALID, k
    # the ops of one set only, of both without room for them, room without ops, half a pair of pointers
    for cig in ((ptr, ptr, None, None, ptr, ptr), (None, None, ptr, ptr, ptr, ptr), (ptr, ptr, ptr, ptr, None, None),
                (None, None, None, None, ptr, ptr), (ptr, None, ptr, ptr, ptr, ptr), (ptr, ptr, ptr, ptr, ptr, None)):
        assert merge(cig=cig) == _lib.KISS_HIP_E_INVALID, cig
    assert merge(ocap=5) == _lib.KISS_HIP_E_INVALID
    assert merge(V=1 << 31) == _lib.KISS_HIP_E_UNSUPPORTED
