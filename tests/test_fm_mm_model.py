"""CPU tests of the FM-index search with mismatches: the numpy model of the FM route (tests/fm_mm_model.py) against the
text itself, what an index that was not built from an exact suffix array does to it, and the C ABI of the call
(struct size, behaviour without a device)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_mm_model as mm
from tests import gen
from tests.fm_model import FmModel

TEXTS = {
    "genome": lambda: gen.genome_like(6000, 3),
    "periodic": lambda: gen.periodic(5000, 7, 1, mutations=12),
    "iid": lambda: gen.iid(4000, 2),
    "allA": lambda: np.zeros(600, np.uint8),
}
LENGTHS = (12, 20, 26, 29, 32, 40)


@functools.lru_cache(maxsize=None)
def text(name):
    return TEXTS[name]()


@functools.lru_cache(maxsize=None)
def model(name, order, sa_intv):
    S = text(name)
    SA = mm.exact_sa(S) if order == "exact" else mm.k_ordered_sa(S, 32, 5)
    return FmModel(S, SA, sa_intv, 0, with_lookup=False)


def test_brute_is_the_definition():
    S = np.array([0, 1, 2, 3, 0, 1, 2, 0], np.uint8)
    c, p, m = mm.brute(S, [0, 1, 2], 1)
    # every window, by hand
    want = [(i, int(np.sum(S[i:i + 3] != np.array([0, 1, 2])))) for i in range(S.size - 2)]
    want = [(i, d) for i, d in want if d <= 1]
    assert list(zip(p.tolist(), m.tolist())) == want
    assert c.tolist() == [sum(1 for _, d in want if d == j) for j in (0, 1)]
    assert mm.brute(S, [0] * 9, 3)[1].size == 0  # L > n
    assert mm.brute(S, [4, 5, 6], 0)[1].tolist() == [0, 4]  # pattern bytes & 3


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("e", (0, 1, 2))
def test_fm_route_equals_brute_on_an_exact_suffix_array(name, e):
    S = text(name)
    for L in LENGTHS:
        pats = mm.patterns_for(S, 4, L, e, 100 * e + L)
        for sa_intv in (4, 8):
            fm = model(name, "exact", sa_intv)
            for P in pats:
                c, p, m = mm.brute(S, P, e)
                r = mm.fm_search(fm, P, e)
                assert r["walk_failures"] == 0
                assert np.array_equal(r["counts"], c), (name, L, e)
                assert np.array_equal(r["positions"], p) and np.array_equal(r["mismatches"], m), (name, L, e, sa_intv)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_counts_survive_a_32_ordered_suffix_array_up_to_length_32(name):
    # the worst case of what FMIndex::build's k = 32 sort allows: ties broken at random.  Counts are a property of the
    # ranges, and the range of a string of length <= 32 is the same set of rows in every 32-ordered suffix array
    S = text(name)
    fm = model(name, "k32", 4)
    for e in (0, 1, 2):
        for L in (12, 20, 32):
            for P in mm.patterns_for(S, 3, L, e, 7 * e + L):
                c, _, _ = mm.brute(S, P, e)
                assert np.array_equal(mm.fm_search(fm, P, e, want_positions=False)["counts"], c), (name, L, e)


def test_positions_need_the_exact_order():
    # on a repetitive text the LF walk of a tied row of a 32-ordered suffix array runs past the bound or reports another
    # suffix: positions are defined for the exact order only, and the bounded walk never loops
    S = text("periodic")
    fm = model("periodic", "k32", 4)
    bad = 0
    for P in mm.patterns_for(S, 6, 12, 1, 3):
        c, p, m = mm.brute(S, P, 1)
        r = mm.fm_search(fm, P, 1)
        assert np.array_equal(r["counts"], c)
        assert r["positions"].size + r["walk_failures"] == int(c.sum())
        bad += r["walk_failures"] > 0 or not np.array_equal(r["positions"], p)
    assert bad > 0


def test_report_struct_matches_the_header():
    from kiss_amd import _lib
    from tests.test_abi import _sizeof_from_header
    assert ctypes.sizeof(_lib.FmiMmReport) == _sizeof_from_header("kiss_hip_fmi_mm_report") == 96
    assert _lib.FmiMmReport.ms_sort.offset == 92 and _lib.FmiMmReport.hits.offset == 16


def test_host_call_checks_its_arguments_and_fails_loudly_without_a_device():
    import torch
    import kiss_amd
    from kiss_amd import _lib
    lib = kiss_amd.load()
    S = gen.iid(300, 1)
    fm = FmModel(S, mm.exact_sa(S), 4, 0)
    blob = fm.serialize()
    from tests.fm_model import sections
    sec, N = sections(blob, 4)
    arr = {k: np.frombuffer(blob, np.uint8, count=v[2], offset=v[0]).copy() for k, v in sec.items()}
    v = _lib.FmiView()
    v.n_sa = N
    for c in range(4):
        v.cnt[c] = int(fm.cnt[c])
    v.pri, v.sa_intv = fm.pri, 4
    for k in ("bwt", "occ1", "occ2", "sa", "b", "b_occ"):
        setattr(v, k, arr[k].ctypes.data)
    pats = mm.patterns_for(S, 5, 10, 1, 1)
    counts = np.zeros((5, 2), np.uint32)
    rep = _lib.FmiMmReport()

    def call(e, L=10, pat=pats, positions=None, mism=None, index=None, cap=0):
        p = lambda a: ctypes.c_void_p(a.ctypes.data if a is not None else None)  # noqa: E731
        return lib.kiss_hip_fmi_query_mm_host(ctypes.byref(v), p(pat), L, 5, e, p(counts), p(positions), p(mism), p(index),
                                              cap, ctypes.byref(rep), 0)
    assert call(4) == _lib.KISS_HIP_E_UNSUPPORTED
    assert call(1, L=0) == _lib.KISS_HIP_E_INVALID
    assert call(1, pat=None) == _lib.KISS_HIP_E_INVALID
    assert call(1, positions=np.zeros(8, np.uint32), cap=8) == _lib.KISS_HIP_E_INVALID  # positions without mismatches / index
    v.sa_intv = 33
    assert call(1) == _lib.KISS_HIP_E_UNSUPPORTED
    v.sa_intv = 4
    if torch.cuda.is_available():
        assert call(1) == _lib.KISS_HIP_OK
        want = mm.brute_batch(S, pats, 1)[0]
        assert np.array_equal(counts, want)
        return
    assert call(1) == _lib.KISS_HIP_E_NO_DEVICE  # no silent CPU fallback
