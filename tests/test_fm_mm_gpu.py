"""GPU tests of the FM-index search with up to 3 mismatches (FMIndex.query_mismatch / kiss_hip_fmi_query_mm_dev) against
the text itself (tests/fm_mm_model.py: brute-force Hamming distance).  No tolerances: counts, positions, mismatch counts,
index, totals and checksum are compared element by element."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_mm_model as mm
from tests import gen

pytestmark = pytest.mark.gpu

TEXTS = {
    "genome": lambda: gen.genome_like(200_000, 5),
    "periodic": lambda: gen.periodic(50_000, 7, 1, mutations=40),
    "iid": lambda: gen.iid(100_000, 2),
    "allA": lambda: np.zeros(10_000, np.uint8),
    "n0": lambda: np.zeros(0, np.uint8),
    "n1": lambda: np.array([2], np.uint8),
    "n5": lambda: np.array([0, 1, 0, 1, 3], np.uint8),
}
LENGTHS = (1, 8, 20, 32, 33, 64, 200)
SA_INTVS = (1, 4, 7, 32)
Q_PER_CASE = 9


@functools.lru_cache(maxsize=None)
def text(name):
    return TEXTS[name]()


@functools.lru_cache(maxsize=None)
def exact_sa(name):
    import kiss_amd
    S = text(name)
    with kiss_amd.Context(max_n=max(S.size, 1 << 20)) as ctx:
        return ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)


_indexes = {}


def index_of(name, sa_intv, hooks=None):
    """the index of a text from its exact suffix array, kept for the session (28 of them)"""
    import kiss_amd.fm_index as fm
    key = (name, sa_intv, hooks)
    if key not in _indexes:
        _indexes[key] = fm.FMIndex(sa_intv=sa_intv, hooks=hooks).build(text(name), sa=exact_sa(name), exact_sa=True)
    return _indexes[key]


@functools.lru_cache(maxsize=None)
def case(name, L, e):
    """patterns of one (text, L, e) and what the text says about them"""
    S = text(name)
    pats = mm.patterns_for(S, Q_PER_CASE, L, e, 1000 * e + L)
    return pats, mm.brute_batch(S, pats, e)


def check(res, want, e):
    counts, pos, mis, idx = want
    assert res["counts"].shape == counts.shape
    assert np.array_equal(res["counts"].astype(np.int64), counts)
    assert res["hits_by_mismatch"] == counts.sum(axis=0).tolist()
    assert res["total_hits"] == int(counts.sum())
    if "positions" in res:
        assert np.array_equal(res["index"].astype(np.int64), idx)
        assert np.array_equal(res["positions"].astype(np.int64), pos)
        assert np.array_equal(res["mismatches"].astype(np.int64), mis)
        assert res["checksum"] == int(pos.sum())
        assert res["report"]["walk_failures"] == 0


@pytest.mark.parametrize("sa_intv", SA_INTVS)
@pytest.mark.parametrize("e", (0, 1, 2, 3))
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_hits_equal_brute_force(name, L, e, sa_intv):
    pats, want = case(name, L, e)
    f = index_of(name, sa_intv)
    check(f.query_mismatch(pats, e), want, e)
    if sa_intv == 4:
        check(f.query_mismatch(pats, e, want_positions=False), want, e)


@pytest.mark.parametrize("name,L,e", [("genome", 20, 2), ("periodic", 32, 3), ("iid", 8, 1), ("allA", 64, 1), ("n5", 1, 1),
                                      ("genome", 33, 0)])
def test_hooks_library_and_its_one_wave_per_pattern_form(name, L, e, monkeypatch):
    # libkiss_hip_hooks.so: as shipped (a wave per pattern for a batch this small), then the one-wave-per-pattern form
    # forced (the A-B switch of DESIGN.md 4.6), then one lane per pattern with a bound
    pats, want = case(name, L, e)
    f = index_of(name, 4, hooks=True)
    monkeypatch.delenv("KISS_HIP_FM_MM_WAVE", raising=False)
    a = f.query_mismatch(pats, e)
    check(a, want, e)
    monkeypatch.setenv("KISS_HIP_FM_MM_WAVE", "1")
    b = f.query_mismatch(pats, e)
    check(b, want, e)
    assert a["report"]["ranges"] == b["report"]["ranges"] and a["report"]["ranges"] > 0
    # and the hand-over between the two: lanes that give a pattern up after 48 pairs, a wave for each of those
    monkeypatch.delenv("KISS_HIP_FM_MM_WAVE")
    monkeypatch.setenv("KISS_HIP_FM_MM_BUDGET", "48")
    c = f.query_mismatch(pats, e)
    check(c, want, e)
    assert c["report"]["ranges"] == a["report"]["ranges"]
    if e and name != "n5":
        assert c["report"]["lf_pairs"] > a["report"]["lf_pairs"]  # (some patterns were searched twice)


@pytest.mark.parametrize("name", ("genome", "periodic", "allA"))
def test_zero_mismatches_is_the_exact_query(name):
    # a cross-check against code the library already had: totals and the sorted positions of query_batch
    S = text(name)
    f = index_of(name, 4)
    for L in (8, 20, 40):
        pats = mm.patterns_for(S, 200, L, 0, L) & 3
        a = f.query_mismatch(pats, 0)
        b = f.query_batch(pats)
        assert a["total_hits"] == b["total_hits"] and a["checksum"] == b["checksum"]
        assert np.array_equal(a["counts"][:, 0], b["end"] - b["beg"])
        assert np.array_equal(a["index"], b["offsets_index"])
        for q in range(pats.shape[0]):
            lo, hi = int(a["index"][q]), int(a["index"][q + 1])
            assert np.array_equal(a["positions"][lo:hi], np.sort(b["offsets"][lo:hi]))
        assert not a["mismatches"].any()


@pytest.mark.parametrize("name", ("periodic", "genome", "allA"))
def test_default_build_counts_up_to_length_32_and_refuses_positions(name):
    import kiss_amd.fm_index as fm
    S = text(name)
    f = fm.FMIndex().build(S)  # k = 32, like the reference
    assert not f.exact_sa
    for L, e in ((8, 1), (20, 2), (32, 2), (32, 0), (12, 3)):
        pats, want = case(name, L, e)
        check(f.query_mismatch(pats, e, want_positions=False), want, e)
    with pytest.raises(ValueError, match="exact=True"):
        f.query_mismatch(case(name, 20, 1)[0], 1)
    f.close()
    g = fm.FMIndex().build(S, exact=True)
    assert g.exact_sa
    pats, want = case(name, 20, 2)
    check(g.query_mismatch(pats, 2), want, 2)
    assert g.to_bytes() == index_of(name, 4).to_bytes()
    g.close()


def raw_call(f, pats, e, want_positions=True, capacity=None):
    """kiss_hip_fmi_query_mm_dev itself on the arrays of index f -> rc, report, counts, positions, mismatches, index"""
    import torch
    from kiss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", f.device)
    d_p = torch.from_numpy(np.ascontiguousarray(pats, np.uint8)).to(dev)
    Q, L = pats.shape
    ctx = f._context(max(f.N, 4 * Q))
    view = f._view()
    counts = torch.zeros((Q, e + 1 if e <= 3 else 1), dtype=torch.int32, device=dev)
    rep = _lib.FmiMmReport()
    vp = ctypes.c_void_p
    if not want_positions:
        rc = lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), vp(d_p.data_ptr()), L, Q, e, vp(counts.data_ptr()), None,
                                           None, None, 0, ctypes.byref(rep), None)
        return rc, rep, counts.cpu().numpy().view(np.uint32), None, None, None
    if capacity is None:
        rc, r0, *_ = raw_call(f, pats, e, want_positions=False)
        assert rc == 0
        capacity = sum(int(x) for x in r0.hits)
    pos = torch.zeros(max(capacity, 1), dtype=torch.int32, device=dev)
    mis = torch.zeros(max(capacity, 1), dtype=torch.uint8, device=dev)
    idx = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    rc = lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), vp(d_p.data_ptr()), L, Q, e, vp(counts.data_ptr()),
                                       vp(pos.data_ptr()), vp(mis.data_ptr()), vp(idx.data_ptr()), capacity, ctypes.byref(rep),
                                       None)
    return (rc, rep, counts.cpu().numpy().view(np.uint32), pos.cpu().numpy().view(np.uint32), mis.cpu().numpy(),
            idx.cpu().numpy().view(np.uint64))


def test_error_contract_of_the_c_call():
    import kiss_amd.fm_index as fm
    from kiss_amd import _lib
    f = index_of("genome", 4)
    pats, want = case("genome", 20, 2)
    total = int(want[0].sum())
    assert total > 2
    rc, rep, *_ = raw_call(f, pats, 2, capacity=total - 1)  # short capacity: the total comes back
    assert rc == _lib.KISS_HIP_E_INVALID and sum(int(x) for x in rep.hits) == total
    rc, rep, counts, pos, mis, idx = raw_call(f, pats, 2, capacity=total)
    assert rc == 0 and np.array_equal(pos[:total].astype(np.int64), want[1]) and rep.checksum == int(want[1].sum())
    assert rep.ranges > 0 and rep.lf_pairs >= rep.ranges and rep.Q == pats.shape[0] and rep.L == 20
    assert raw_call(f, pats, 4, want_positions=False)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    assert raw_call(f, pats[:0], 2, want_positions=False)[0] == 0  # Q = 0
    # longer than the text: no hits
    tiny = index_of("n5", 4)
    rc, rep, counts, *_ = raw_call(tiny, np.zeros((3, 9), np.uint8), 3, capacity=4)
    assert rc == 0 and not counts.any() and sum(int(x) for x in rep.hits) == 0
    # The arrays of a k = 32 index with positions: the call always returns, with OK or E_INVALID, and walk_failures says
    # which; counts stay right (L <= 32)
    for name in ("periodic", "allA", "genome"):
        g = fm.FMIndex().build(text(name))
        for L, e in ((12, 1), (32, 2)):
            p, w = case(name, L, e)
            rc, rep, counts, pos, mis, idx = raw_call(g, p, e)
            assert rc in (0, _lib.KISS_HIP_E_INVALID)
            assert (rc == _lib.KISS_HIP_E_INVALID) == (rep.walk_failures > 0)
            assert np.array_equal(counts.astype(np.int64), w[0])
            assert np.array_equal(idx.astype(np.int64), w[3])
        g.close()


def host_view(f):
    """the arrays of index f in host memory and a kiss_hip_fmi_view over them (sa_intv == 1: no b / b_occ) -> view, arrays"""
    from kiss_amd import _lib
    v = _lib.FmiView()
    v.n_sa, v.pri, v.sa_intv = f.N, f.pri, f.sa_intv
    for c in range(4):
        v.cnt[c] = int(f.cnt[c])
    arrays = {k: getattr(f, k).cpu().numpy() for k in ("bwt", "occ1", "occ2", "sa", "b", "b_occ") if getattr(f, k) is not None}
    for k, a in arrays.items():
        setattr(v, k, a.ctypes.data)
    return v, arrays


@pytest.mark.parametrize("sa_intv", (1, 4))
def test_host_entry_empty_batch_counts_alone_and_size_then_fill(sa_intv):
    """kiss_hip_fmi_query_mm_host on host copies of the index (with and without the sampling bit-vector) against the text"""
    from kiss_amd import _lib
    lib = _lib.load()
    f = index_of("genome", sa_intv)
    pats, want = case("genome", 20, 2)
    pats = np.ascontiguousarray(pats, np.uint8)
    Q, L = pats.shape
    total = int(want[0].sum())
    assert total > 2 and (want[0].sum(axis=1) == 0).any() and (want[0].sum(axis=1) > 1).any()  # no hit; several
    v, arrays = host_view(f)

    def call(Q, capacity):
        """capacity None: counts alone"""
        counts, idx = np.full((Q, 3), 7, np.uint32), np.full(Q + 1, 7, np.uint64)
        pos, mis = np.zeros(max(capacity or 0, 1), np.uint32), np.zeros(max(capacity or 0, 1), np.uint8)
        rep = _lib.FmiMmReport()
        outs = (pos.ctypes.data, mis.ctypes.data, idx.ctypes.data, capacity) if capacity is not None else (None, None, None, 0)
        rc = lib.kiss_hip_fmi_query_mm_host(ctypes.byref(v), pats.ctypes.data if Q else None, L, Q, 2, counts.ctypes.data if Q else None,
                                            *outs, ctypes.byref(rep), 0)
        return rc, rep, counts, pos, mis, idx

    rc, rep, counts, pos, mis, idx = call(0, 0)  # the empty batch: index[0] = 0
    assert rc == 0 and idx.tolist() == [0] and sum(int(x) for x in rep.hits) == 0
    rc, rep, counts, *_ = call(Q, None)
    assert rc == 0 and np.array_equal(counts.astype(np.int64), want[0]) and [int(x) for x in rep.hits][:3] == want[0].sum(axis=0).tolist()
    rc, rep, *_ = call(Q, 0)  # the sizing call: the totals come back
    assert rc == _lib.KISS_HIP_E_INVALID and sum(int(x) for x in rep.hits) == total
    rc, rep, counts, pos, mis, idx = call(Q, total)
    assert rc == 0 and rep.walk_failures == 0 and rep.checksum == int(want[1].sum())
    assert np.array_equal(counts.astype(np.int64), want[0]) and np.array_equal(idx.astype(np.int64), want[3])
    assert np.array_equal(pos.astype(np.int64), want[1]) and np.array_equal(mis.astype(np.int64), want[2])


@functools.lru_cache(maxsize=None)
def large():
    import kiss_amd
    import kiss_amd.fm_index as fm
    S = gen.genome_like(2_000_000, 9)
    with kiss_amd.Context(max_n=S.size) as ctx:
        SA = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    return S, fm.FMIndex().build(S, sa=SA, exact_sa=True)


def test_two_million_bases_twenty_thousand_patterns():
    S, f = large()
    Q, L, e = 20_000, 24, 2
    rng = np.random.default_rng(4)
    planted = rng.integers(0, S.size - L + 1, Q)
    pats = S[planted[:, None] + np.arange(L)[None, :]].copy()
    nsub = rng.integers(0, e + 1, Q)  # 0 .. e substitutions: the planted position stays a hit
    for k in range(e):
        rows = np.flatnonzero(nsub > k)
        cols = rng.integers(0, L, rows.size)
        pats[rows, cols] = (pats[rows, cols] + 1 + rng.integers(0, 3, rows.size)) & 3
    r = f.query_mismatch(pats, e)
    idx, pos, mis = r["index"].astype(np.int64), r["positions"].astype(np.int64), r["mismatches"].astype(np.int64)
    assert idx[0] == 0 and idx[-1] == pos.size == r["total_hits"] and np.all(np.diff(idx) >= 1)
    # every returned hit against the text: the distance is the stated one, the order ascending inside a pattern
    owner = np.repeat(np.arange(Q), np.diff(idx))
    assert pos.max() <= S.size - L
    d = np.zeros(pos.size, np.int64)
    for j in range(L):
        d += S[pos + j] != pats[owner, j]
    assert np.array_equal(d, mis) and d.max() <= e
    inner = np.ones(pos.size, bool)
    inner[idx[:-1]] = False
    assert np.all(np.diff(pos)[inner[1:]] > 0)
    assert np.array_equal(r["counts"].astype(np.int64),
                          np.stack([np.bincount(owner[mis == j], minlength=Q) for j in range(e + 1)], axis=1))
    assert r["checksum"] == int(pos.sum())
    # the planted position is among the hits of its pattern
    key = owner * (1 << 32) + pos
    assert np.all(np.isin(np.arange(Q) * (1 << 32) + planted, key))
    # 50 patterns in full
    for q in rng.choice(Q, 50, replace=False).tolist():
        c, p, m = mm.brute(S, pats[q], e)
        assert np.array_equal(pos[idx[q]:idx[q + 1]], p) and np.array_equal(mis[idx[q]:idx[q + 1]], m)
        assert np.array_equal(r["counts"][q].astype(np.int64), c)


def test_a_batch_with_more_hits_than_one_call_sorts_is_split():
    S, f = large()
    e, L = 2, 6
    pats = mm.patterns_for(S, 24, L, e, 11)
    want = mm.brute_batch(S, pats, e)
    assert int(want[0].sum()) > 700_000  # more than the LMS arrays of a context for 2 * 10^6 bases hold
    r = f.query_mismatch(pats, e)
    check(r, want, e)
    assert r["report"]["calls"] > 1


def test_a_batch_of_more_than_65536_patterns_runs_the_lanes_first_and_says_the_same():
    # up to 65 536 patterns of a call go to a wave each; a larger batch goes to one lane per pattern, then a wave for each
    # pattern a lane gave up.  The same patterns both ways, and a sample of them against the text.
    S, f = large()
    Q, L, e = 70_000, 24, 2
    rng = np.random.default_rng(6)
    planted = rng.integers(0, S.size - L + 1, Q)
    pats = S[planted[:, None] + np.arange(L)[None, :]].copy()
    rows = np.flatnonzero(rng.integers(0, 2, Q))
    cols = rng.integers(0, L, rows.size)
    pats[rows, cols] = (pats[rows, cols] + 1 + rng.integers(0, 3, rows.size)) & 3
    pats[::7, :8] = 0  # patterns that begin with AAAAAAAA, and a few of nothing else: wide ranges, long walks
    pats[::7000] = 0
    whole = f.query_mismatch(pats, e)
    halves = [f.query_mismatch(pats[:Q // 2], e), f.query_mismatch(pats[Q // 2:], e)]
    assert np.array_equal(whole["counts"], np.concatenate([h["counts"] for h in halves]))
    assert np.array_equal(whole["positions"], np.concatenate([h["positions"] for h in halves]))
    assert np.array_equal(whole["mismatches"], np.concatenate([h["mismatches"] for h in halves]))
    assert np.array_equal(np.diff(whole["index"].astype(np.int64)),
                          np.concatenate([np.diff(h["index"].astype(np.int64)) for h in halves]))
    assert whole["report"]["lf_pairs"] >= sum(h["report"]["lf_pairs"] for h in halves)  # (a pattern given up is searched twice)
    assert np.array_equal(whole["counts"], f.query_mismatch(pats, e, want_positions=False)["counts"])
    idx = whole["index"].astype(np.int64)
    for q in [0, 7, 7000] + rng.choice(Q, 20, replace=False).tolist():
        c, p, m = mm.brute(S, pats[q], e)
        assert np.array_equal(whole["counts"][q].astype(np.int64), c)
        assert np.array_equal(whole["positions"][idx[q]:idx[q + 1]].astype(np.int64), p)
        assert np.array_equal(whole["mismatches"][idx[q]:idx[q + 1]].astype(np.int64), m)
