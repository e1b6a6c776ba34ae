"""GPU tests of the maximal exact match seeds (FMIndex.seeds / kiss_hip_fmi_seeds_dev) against the text itself
(tests/fm_seed_model.py: bytes.find).  No tolerances: ms of every end, seed_index, every seed, pos_index, every position,
the checksum and the report's totals are compared element by element."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_seed_model as sm
from tests import gen
from tests.test_fm_mm_gpu import TEXTS, exact_sa, text

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 31, 63, 64, 65, 150, 257, 1000)
PARAMS = ((1, 0, 0), (19, 0, 500), (12, 32, 3), (7, 7, 0))  # (min_len, max_len, max_occ)
SA_INTVS = (1, 4, 7, 32)

_indexes = {}


def index_of(name, sa_intv, hooks=None):
    """the index of a text from its exact suffix array, kept for the session"""
    import kiss_amd.fm_index as fm
    key = (name, sa_intv, hooks)
    if key not in _indexes:
        _indexes[key] = fm.FMIndex(sa_intv=sa_intv, hooks=hooks).build(text(name), sa=exact_sa(name), exact_sa=True)
    return _indexes[key]


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """one ragged batch per text: per length a read cut from the text, one with about L / 40 substitutions, a random one,
    the read at text position 0 (the primary row), the read that ends at n, reads with a no-base in the middle, at either
    end and everywhere, and a read of C only (absent from the allA text)"""
    S = text(name)
    n = S.size
    rng = np.random.default_rng(17)
    out = []
    for L in LENGTHS:
        rnd = rng.integers(0, 4, L, dtype=np.uint8)
        out.append(rnd)
        if n >= L:
            p = int(rng.integers(0, n - L + 1))
            cut = S[p:p + L].copy()
            out.append(cut)
            sub = cut.copy()
            for _ in range(max(1, L // 40)):
                j = int(rng.integers(0, L))
                sub[j] = (sub[j] + 1 + rng.integers(0, 3)) & 3
            out.append(sub)
            out.append(S[:L].copy())
            out.append(S[n - L:].copy())
        else:
            cut = rng.integers(0, 4, L, dtype=np.uint8)
        mid = cut.copy()
        mid[L // 2] = 78  # 'N'
        out.append(mid)
        ends = cut.copy()
        ends[0] = 4
        ends[-1] = 255
        out.append(ends)
        out.append(np.full(L, 4 + (L & 3), np.uint8))
        out.append(np.ones(L, np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def model(name, max_len, both):
    """searched once per text (both strands, no cap); the other forms are cut from it (fm_seed_model.Batch)"""
    if not both:
        return model(name, max_len, True).forward_only()
    if max_len:
        return model(name, 0, True).capped(max_len)
    return sm.Batch(text(name), reads_of(name), True)


@functools.lru_cache(maxsize=None)
def model_seeds(name, params, both):
    min_len, max_len, max_occ = params
    return model(name, max_len, both).seeds(min_len, max_occ)


def check(res, b, want, positions=True):
    rep = res["report"]
    if "ms" in res:
        assert np.array_equal(res["ms"].astype(np.int64), b.ms)
    assert np.array_equal(res["seed_index"].astype(np.int64), want["seed_index"])
    assert np.array_equal(res["seeds"]["start"].astype(np.int64), want["start"])
    assert np.array_equal(res["seeds"]["len"].astype(np.int64), want["len"])
    assert np.array_equal(res["count"].astype(np.int64), want["count"])
    assert (rep["Q"], rep["V"], rep["bases"]) == (b.Q, b.V, b.bases)
    assert rep["seeds"] == want["len"].size and rep["located_seeds"] == want["located_seeds"]
    assert rep["positions"] == want["positions"].size
    assert rep["lf_pairs"] == b.lf_pairs
    assert rep["max_ms"] == (int(b.ms.max()) if b.bases else 0)
    if positions:
        assert np.array_equal(res["pos_index"].astype(np.int64), want["pos_index"])
        assert res["positions"].size == want["positions"].size and np.array_equal(res["positions"], want["positions"])
        assert rep["checksum"] == want["checksum"]
        assert rep["walk_failures"] == 0


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("sa_intv", SA_INTVS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_seeds_equal_the_model(name, sa_intv, both):
    f = index_of(name, sa_intv)
    reads = reads_of(name)
    for params in PARAMS:
        min_len, max_len, max_occ = params
        res = f.seeds(reads, min_len, max_len, max_occ, both_strands=both, want_ms=True)
        check(res, model(name, max_len, both), model_seeds(name, params, both))
    if sa_intv == 4:  # without positions, and from (concatenated, index) with an index that does not start at 0
        params = PARAMS[1]
        cat = np.concatenate([np.full(3, 9, np.uint8)] + reads)
        index = np.concatenate([[3], 3 + np.cumsum([r.size for r in reads])]).astype(np.uint64)
        res = f.seeds((cat, index), *params, both_strands=both, want_positions=False)
        assert "positions" not in res and "ms" not in res
        check(res, model(name, params[1], both), model_seeds(name, params, both), positions=False)


@pytest.mark.parametrize("params", (PARAMS[0], PARAMS[2]))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_ranges_equal_get_range_of_the_seed_strings(name, params):
    # a cross-check against code the library already had: the exact query (kiss_hip_fmi_query_ex_dev) on the same index
    f = index_of(name, 7)
    reads = reads_of(name)
    res = f.seeds(reads, *params, both_strands=True, want_positions=False)
    vreads = sm.virtual_reads(reads, True)
    owner = np.repeat(np.arange(len(vreads)), np.diff(res["seed_index"].astype(np.int64)))
    seeds = res["seeds"]
    for L in np.unique(seeds["len"]).tolist():
        rows = np.flatnonzero(seeds["len"] == L)
        pats = np.stack([vreads[owner[i]][int(seeds["start"][i]):int(seeds["start"][i]) + L] for i in rows])
        assert pats.max() < 4
        r = f.query_batch(pats, want_offsets=False)
        assert np.array_equal(r["beg"], seeds["sa_beg"][rows]) and np.array_equal(r["end"], seeds["sa_end"][rows])


def test_a_seed_over_max_occ_reports_its_range_and_no_positions():
    f = index_of("allA", 4)
    res = f.seeds([np.zeros(100, np.uint8)], min_len=19, max_len=0, max_occ=3)
    assert res["seed_index"].tolist() == [0, 1]
    assert (int(res["seeds"]["start"][0]), int(res["seeds"]["len"][0])) == (0, 100)
    assert int(res["count"][0]) == 10_000 - 100 + 1
    assert res["pos_index"].tolist() == [0, 0] and res["positions"].size == 0
    assert res["report"]["located_seeds"] == 0 and res["report"]["positions"] == 0
    # and the C read against the same text: a symbol the text does not have
    res = f.seeds([np.ones(100, np.uint8)], min_len=1, both_strands=False)
    assert res["seeds"].size == 0 and res["seed_index"].tolist() == [0, 0] and res["report"]["max_ms"] == 0


@pytest.mark.parametrize("name", ("periodic", "genome", "allA"))
def test_default_build_with_max_len_32_says_the_same_and_refuses_the_rest(name):
    import kiss_amd.fm_index as fm
    f = fm.FMIndex().build(text(name))  # k = 32, like the reference
    assert not f.exact_sa
    reads = reads_of(name)
    params = PARAMS[2]
    for both in (False, True):
        res = f.seeds(reads, *params, both_strands=both, want_positions=False, want_ms=True)
        check(res, model(name, 32, both), model_seeds(name, params, both), positions=False)
    exact = index_of(name, 4).seeds(reads, *params, both_strands=True, want_positions=False)
    assert np.array_equal(res["seeds"], exact["seeds"])  # the ranges too
    with pytest.raises(ValueError, match="exact=True"):
        f.seeds(reads, *params)
    for max_len in (0, 33):
        with pytest.raises(ValueError, match="exact=True"):
            f.seeds(reads, 12, max_len, 3, want_positions=False)
    f.close()


@pytest.mark.parametrize("name,params,both", [("genome", PARAMS[1], True), ("periodic", PARAMS[0], False), ("n5", PARAMS[0], True),
                                              ("allA", PARAMS[3], True)])
def test_hooks_library_says_the_same(name, params, both):
    f = index_of(name, 4, hooks=True)
    res = f.seeds(reads_of(name), *params, both_strands=both, want_ms=True)
    check(res, model(name, params[1], both), model_seeds(name, params, both))


def raw_call(f, cat, index, params, both, seed_capacity, pos_capacity=None, min_len=None):
    """kiss_hip_fmi_seeds_dev itself on the arrays of index f -> rc, report, seeds (n x 4), seed_index, positions, pos_index"""
    import torch
    from kiss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", f.device)
    vp = ctypes.c_void_p
    Q = len(index) - 1
    V = 2 * Q if both else Q
    d_reads = torch.from_numpy(np.ascontiguousarray(cat, np.uint8)).to(dev) if len(cat) else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_index = torch.from_numpy(np.asarray(index, np.int64)).to(dev)
    ctx = f._context(max(f.N, 1 << 20))
    vex = _lib.FmiViewEx()
    vex.base = f._view()
    vex.lookup_len = 0
    vex.lookup = None  # (the search does not use it)
    d_seeds = torch.zeros((max(seed_capacity, 1), 4), dtype=torch.int32, device=dev)
    d_sidx = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    d_pos = d_pidx = None
    if pos_capacity is not None:
        d_pos = torch.zeros(max(pos_capacity, 1), dtype=torch.int32, device=dev)
        d_pidx = torch.full((max(seed_capacity, 0) + 1,), -1, dtype=torch.int64, device=dev)
    rep = _lib.FmiSeedReport()
    rc = lib.kiss_hip_fmi_seeds_dev(ctx._ctx, ctypes.byref(vex), vp(d_reads.data_ptr()), vp(d_index.data_ptr()), Q,
                                    params[0] if min_len is None else min_len, params[1], params[2], 1 if both else 0, None,
                                    vp(d_seeds.data_ptr()), vp(d_sidx.data_ptr()), seed_capacity,
                                    vp(d_pos.data_ptr()) if d_pos is not None else None,
                                    vp(d_pidx.data_ptr()) if d_pidx is not None else None,
                                    pos_capacity or 0, ctypes.byref(rep), None)
    return (rc, rep, d_seeds.cpu().numpy().view(np.uint32), d_sidx.cpu().numpy(),
            d_pos.cpu().numpy().view(np.uint32) if d_pos is not None else None,
            d_pidx.cpu().numpy() if d_pidx is not None else None)


def test_error_contract_of_the_c_call():
    from kiss_amd import _lib
    name, params, both = "genome", PARAMS[1], True
    f = index_of(name, 4)
    reads = reads_of(name)
    want = model_seeds(name, params, both)
    b = model(name, params[1], both)
    cat = np.concatenate(reads)
    index = np.concatenate([[0], np.cumsum([r.size for r in reads])])
    nseeds, npos = int(want["len"].size), int(want["positions"].size)
    assert nseeds > 2 and npos > 2
    # capacities one too small: E_INVALID with the totals, and the call with room succeeds
    rc, rep, *_ = raw_call(f, cat, index, params, both, nseeds - 1)
    assert rc == _lib.KISS_HIP_E_INVALID and rep.seeds == nseeds and rep.positions == npos and rep.bases == b.bases
    rc, rep, *_ = raw_call(f, cat, index, params, both, nseeds, npos - 1)
    assert rc == _lib.KISS_HIP_E_INVALID and rep.seeds == nseeds and rep.positions == npos
    rc, rep, seeds, sidx, pos, pidx = raw_call(f, cat, index, params, both, nseeds, npos)
    assert rc == 0 and rep.walk_failures == 0 and rep.checksum == want["checksum"]
    assert np.array_equal(sidx, want["seed_index"]) and np.array_equal(pidx, want["pos_index"])
    assert np.array_equal(seeds[:, 0], want["start"]) and np.array_equal(seeds[:, 1], want["len"])
    assert np.array_equal((seeds[:, 3] - seeds[:, 2]).astype(np.int64), want["count"])
    assert np.array_equal(pos[:npos].astype(np.int64), want["positions"])
    # min_len = 0, a read of length zero, an index that decreases, positions without their index
    assert raw_call(f, cat, index, params, both, b.bases, min_len=0)[0] == _lib.KISS_HIP_E_INVALID
    empty = index.copy()
    empty[5] = empty[4]
    assert raw_call(f, cat, empty, params, both, b.bases)[0] == _lib.KISS_HIP_E_INVALID
    down = index.copy()
    down[5] = down[4] - 1
    assert raw_call(f, cat, down, params, both, b.bases)[0] == _lib.KISS_HIP_E_INVALID
    # Q = 0: OK, nothing found
    rc, rep, seeds, sidx, pos, pidx = raw_call(f, cat[:0], index[:1], params, both, 0, 0)
    assert rc == 0 and rep.seeds == 0 and rep.bases == 0 and sidx.tolist() == [0] and pidx.tolist() == [0]
    res = f.seeds([], *params, both_strands=both)
    assert res["seeds"].size == 0 and res["seed_index"].tolist() == [0] and res["pos_index"].tolist() == [0]
    with pytest.raises(ValueError):
        f.seeds(reads, 0)
    with pytest.raises(ValueError):
        f.seeds([np.zeros(0, np.uint8)])


@pytest.mark.parametrize("sa_intv", (1, 4))
def test_host_entry_equals_the_device_call(sa_intv):
    """kiss_hip_fmi_seeds_host on host copies of the index (with and without the sampling bit-vector): the empty batch, the sizing
    call, the fill call with every optional output behind a read index that does not start at 0, and the call without them"""
    from kiss_amd import _lib
    from tests.test_fm_mm_gpu import host_view
    lib = _lib.load()
    name, params = "genome", PARAMS[1]
    f = index_of(name, sa_intv)
    reads = [r for r in reads_of(name) if 2 <= r.size <= 150]
    want = f.seeds(reads, *params, both_strands=True, want_ms=True)
    per_read = np.diff(want["seed_index"].astype(np.int64))
    nseeds, npos = int(want["seeds"].size), int(want["positions"].size)
    assert len(reads) <= 64 and (per_read == 0).any() and (per_read > 1).any() and nseeds > 2 and npos > 2
    lead = 5
    cat = np.concatenate([np.full(lead, 9, np.uint8)] + reads)
    index = (lead + np.concatenate([[0], np.cumsum([r.size for r in reads])])).astype(np.uint64)
    bases = 2 * int(index[-1] - index[0])
    vex = _lib.FmiViewEx()
    vex.base, arrays = host_view(f)
    vex.lookup_len, vex.lookup = 0, None

    def call(Q, seed_capacity, pos_capacity, want_ms):
        """pos_capacity None: no positions"""
        seeds, sidx = np.zeros((max(seed_capacity, 1), 4), np.uint32), np.full(2 * Q + 1, 7, np.uint64)
        pos, pidx = np.zeros(max(pos_capacity or 0, 1), np.uint32), np.full(seed_capacity + 1, 7, np.uint64)
        ms = np.full(max(bases, 1), 7, np.uint32)
        rep = _lib.FmiSeedReport()
        outs = (pos.ctypes.data, pidx.ctypes.data, pos_capacity) if pos_capacity is not None else (None, None, 0)
        rc = lib.kiss_hip_fmi_seeds_host(ctypes.byref(vex), cat.ctypes.data if Q else None, index.ctypes.data if Q else None, Q, params[0],
                                         params[1], params[2], 1, ms.ctypes.data if want_ms else None, seeds.ctypes.data, sidx.ctypes.data,
                                         seed_capacity, *outs, ctypes.byref(rep), 0)
        return rc, rep, seeds, sidx, pos, pidx, ms

    def same_seeds(seeds, sidx):
        assert np.array_equal(sidx, want["seed_index"])
        for j, k in enumerate(("start", "len", "sa_beg", "sa_end")):
            assert np.array_equal(seeds[:nseeds, j], want["seeds"][k]), k

    rc, rep, seeds, sidx, pos, pidx, ms = call(0, 0, 0, False)  # the empty batch: seed_index[0] = pos_index[0] = 0
    assert rc == 0 and sidx.tolist() == [0] and pidx.tolist() == [0] and rep.seeds == 0
    rc, rep, *_ = call(len(reads), 0, 0, False)  # the sizing call: the totals come back
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.seeds, rep.positions) == (nseeds, npos)
    rc, rep, seeds, sidx, pos, pidx, ms = call(len(reads), nseeds, npos, True)
    assert rc == 0
    same_seeds(seeds, sidx)
    assert np.array_equal(pidx, want["pos_index"]) and np.array_equal(pos[:npos], want["positions"])
    assert np.array_equal(ms[:bases], want["ms"])
    assert {k: x for k, x in rep.as_dict().items() if not k.startswith("ms_")} == \
        {k: x for k, x in want["report"].items() if not k.startswith("ms_")}
    rc, rep, seeds, sidx, pos, pidx, ms = call(len(reads), nseeds, None, False)
    assert rc == 0 and (ms == 7).all()
    same_seeds(seeds, sidx)
