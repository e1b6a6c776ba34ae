"""GPU tests of the chaining (kiss_amd.chain_seeds / FMIndex.chains / kiss_hip_fmi_chain_dev) against the plain restatement
of the definition (tests/fm_chain_model.py).  No tolerances: every chain record, chain_index, every chain anchor,
anchor_index and the report's totals are compared element by element.
(a) synthetic anchors straight into chain_seeds; (b) FMIndex.chains on the texts of the other FM-index tests, against the
model run on fm_seed_model's seeds and positions."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_chain_model as cm
from tests import fm_seed_model as sm
from tests.test_fm_mm_gpu import TEXTS, exact_sa, text

pytestmark = pytest.mark.gpu

CHAIN_FIELDS = ("score", "anchors", "rbeg", "rend", "tbeg", "tend")


def arrays_of(reads):
    """reads: per virtual read a list of seeds (start, len, [positions]) -> start, len, seed_index, positions, pos_index"""
    start, length, sidx, pos, pidx = [], [], [0], [], [0]
    for seeds in reads:
        for s, l, ps in seeds:
            start.append(s)
            length.append(l)
            pos.extend(ps)
            pidx.append(len(pos))
        sidx.append(len(start))
    return (np.array(start, np.int64), np.array(length, np.int64), np.array(sidx, np.int64), np.array(pos, np.int64),
            np.array(pidx, np.int64))


def check(res, want, anchors=True):
    rep = res["report"]
    assert np.array_equal(res["chain_index"].astype(np.int64), want["chain_index"])
    got = np.stack([res["chains"][k].astype(np.int64) for k in CHAIN_FIELDS], axis=1) if res["chains"].size else np.zeros((0, 6), np.int64)
    assert got.shape == want["chains"].shape and np.array_equal(got, want["chains"])
    assert (rep["V"], rep["anchors"], rep["chains"]) == (want["V"], want["n_anchors"], want["chains"].shape[0])
    assert rep["chain_anchors"] == want["anchors"].shape[0]
    assert rep["dp_pairs"] == want["dp_pairs"] and rep["max_anchors"] == want["max_anchors"]
    assert rep["best_score"] == want["best_score"]
    if anchors:
        assert np.array_equal(res["anchor_index"].astype(np.int64), want["anchor_index"])
        ga = np.stack([res["anchors"][k].astype(np.int64) for k in ("rstart", "tpos", "len")], axis=1) if res["anchors"].size \
            else np.zeros((0, 3), np.int64)
        assert ga.shape == want["anchors"].shape and np.array_equal(ga, want["anchors"])


def run(reads, **params):
    """chain_seeds on synthetic reads, compared with the model; returns the model's result"""
    import kiss_amd
    start, length, sidx, pos, pidx = arrays_of(reads)
    want = cm.chain(start, length, sidx, pos, pidx, **params)
    res = kiss_amd.chain_seeds(np.stack([start, length], axis=1), sidx, pos, pidx, **params)
    check(res, want)
    return want


def single(anchors):
    """one virtual read, one seed with one position per anchor (r, t, l)"""
    return [[(r, l, [t]) for r, t, l in anchors]]


def diagonals(n, K, t0=1000):
    """n anchors on K interleaved diagonals 7 apart: anchor m is step m // K of diagonal m % K, at r = 700 step and
    t = t0 + 700 step + 7 diagonal.  In (t, slot) order the anchor before it on its own diagonal is K back."""
    return [(700 * (m // K), t0 + 700 * (m // K) + 7 * (m % K), 5 + m % 3) for m in range(n)]


def test_no_virtual_reads_and_reads_without_seeds():
    import kiss_amd
    res = kiss_amd.chain_seeds(np.zeros((0, 2), np.int64), [0], [], [0])
    assert res["chain_index"].tolist() == [0] and res["chains"].size == 0 and res["anchor_index"].tolist() == [0]
    assert res["report"]["V"] == 0 and res["report"]["chains"] == 0
    one = [(0, 30, [100]), (40, 30, [140])]
    for reads in ([[], one, one], [one, [], one], [one, one, []], [[], [], one, [], []], [[], []]):
        want = run(reads, min_score=1)
        assert want["V"] == len(reads)
    assert run([[], one, []])["chain_index"].tolist() == [0, 0, 1, 1]


def test_a_seed_with_an_empty_position_segment_and_a_single_anchor():
    over = (10, 25, [])  # over max_occ: it reports its range and no positions
    want = run([[over, (0, 30, [100]), over, (40, 30, [140]), over], [over], [(3, 50, [7])]])
    assert want["n_anchors"] == 3 and want["chain_index"].tolist() == [0, 1, 1, 2]
    assert want["chains"].tolist() == [[60, 2, 0, 70, 100, 170], [50, 1, 3, 53, 7, 57]]
    want = run(single([(5, 9, 40)]))  # A = 1
    assert want["chains"].tolist() == [[40, 1, 5, 45, 9, 49]] and want["dp_pairs"] == 0 and want["max_anchors"] == 1
    assert run(single([(5, 9, 39)]))["chains"].shape[0] == 0  # under min_score


@pytest.mark.parametrize("n", (63, 64, 65, 129, 1000))
def test_runs_on_diagonals_under_every_lookback(n):
    # K = 1: the nearest predecessor is the one before; K = 2, 70: it is K back, beyond a lookback of 1 or of 64; with a
    # band of 10 the neighbouring diagonals compete at a cost
    for K in (1, 2, 70):
        for look in (64, 1, 100, 0):
            for band, cost in ((3, 2), (10, 9)):
                want = run(single(diagonals(n, K)), max_gap=800, band=band, gap_cost=cost, max_lookback=look, min_score=12)
                if K == 1:
                    assert want["chains"].shape[0] == 1 and want["chains"][0, 1] == n
                elif band == 3 and look != 0 and look < K:  # the anchor before it on its diagonal is out of reach
                    assert want["chains"].shape[0] == 0


def test_steps_exactly_at_max_gap_and_at_the_band():
    G, B = 300, 20
    for d, joined in ((G, True), (G + 1, False)):
        # dt = dr = d; dr = d with dt at the limit; dt = d with dr at the limit
        for a in ((d, 100 + d), (d, 100 + G), (G, 100 + d)):
            want = run(single([(0, 100, 20), (a[0], a[1], 20)]), max_gap=G, band=B, min_score=1)
            assert want["chains"].shape[0] == (1 if joined else 2)
    for g, joined in ((B, True), (B + 1, False)):
        for a in ((50, 150 + g), (50 + g, 150)):
            want = run(single([(0, 100, 20), (a[0], a[1], 20)]), max_gap=G, band=B, min_score=1)
            assert want["chains"].shape[0] == (1 if joined else 2)
            assert want["chains"][0, 0] == (40 - (g * 2) // 8 if joined else 20)


def test_equal_t_and_equal_r():
    # equal t with different r: dt = 0, slot order, every anchor its own chain
    want = run([[(40 - 10 * k, 30, [500]) for k in range(5)]], min_score=1)
    assert want["chains"].shape[0] == 5 and want["anchors"][:, 0].tolist() == [40, 30, 20, 10, 0]
    # equal r with different t (one seed, five positions): dr = 0
    want = run([[(8, 30, [100, 140, 180, 220, 260])]], min_score=1)
    assert want["chains"].shape[0] == 5 and want["chains"][:, 1].tolist() == [1] * 5
    # both among anchors that do chain
    run([[(0, 30, [100, 140]), (40, 30, [140, 180, 180 + 3]), (80, 25, [180, 220])]], min_score=1)


def test_min_score_exactly_at_a_score_and_one_above():
    reads = single(diagonals(40, 3)) + single([(0, 100, 33), (50, 150, 9)])
    base = dict(max_gap=800, band=3)
    want = run(reads, min_score=0, **base)
    scores = sorted(set(want["chains"][:, 0].tolist()))
    assert len(scores) >= 3
    for s in scores:
        at, above = run(reads, min_score=s, **base), run(reads, min_score=s + 1, **base)
        assert (at["chains"][:, 0] >= s).all() and (at["chains"][:, 0] == s).any()
        assert above["chains"].shape[0] == at["chains"].shape[0] - int((at["chains"][:, 0] == s).sum())


def test_positions_at_the_top_of_u32():
    top = 4294963199  # + a length of 4096 = 2^32 - 1
    run_ = [(10 * i, top - 10 * (29 - i), 8) for i in range(30)]
    low = [(0, 5, 30), (7, 12, 4096)]
    for params in (dict(), dict(max_gap=(1 << 31) - 1, band=(1 << 31) - 1, gap_cost=1), dict(max_lookback=0, min_score=1)):
        want = run(single(low + run_[:-1] + [(290, top, 4096)]), **params)
        assert want["chains"][-1, 5] == 4294967295 and want["chains"][-2, 1] == 29  # (its 4096 bases beat joining the run)
    want = run(single(low + run_), max_gap=(1 << 31) - 1, band=(1 << 31) - 1, gap_cost=0, min_score=1)
    assert want["chains"][:, 1].tolist() == [1, 1, 30]  # 2^32 - 4096 - 5 is more than 2^31 - 1 away: no chain across


@pytest.mark.parametrize("cost", (0, 65535))
def test_gap_cost_at_both_ends(cost):
    for look in (64, 0):
        run(single(diagonals(200, 4)), max_gap=800, band=30, gap_cost=cost, max_lookback=look, min_score=1)
    rng = np.random.default_rng(cost)
    run([random_read(rng, 150, 900)], max_gap=200, band=150, gap_cost=cost, max_lookback=0, min_score=1)


def random_read(rng, nseeds, spread):
    """seeds with one to three positions each near a few diagonals, many equal coordinates"""
    out = []
    for _ in range(nseeds):
        r = int(rng.integers(0, spread))
        ps = sorted(int(r + 1000 * rng.integers(0, 2) + 4 * rng.integers(-3, 4)) + 100 for _ in range(int(rng.integers(1, 4))))
        out.append((r, int(rng.integers(1, 40)), ps))
    return out


@pytest.mark.parametrize("look", (64, 5, 200, 0))
def test_random_anchor_sets(look):
    rng = np.random.default_rng(100 + look)
    reads = [random_read(rng, int(rng.integers(0, 120)), int(rng.integers(5, 400))) for _ in range(60)]
    want = run(reads, max_gap=int(rng.integers(20, 300)), band=int(rng.integers(0, 40)), gap_cost=int(rng.integers(0, 20)),
               max_lookback=look, min_score=int(rng.integers(1, 60)))
    assert want["chains"].shape[0] > 20 and (want["chains"][:, 1] > 3).any()
    assert want["max_anchors"] > 130  # more than two chunks of 64 in one read


def test_small_reads_mixed_with_one_of_5000_anchors():
    rng = np.random.default_rng(9)
    reads = []
    for k in range(40):
        reads.append([(int(rng.integers(0, 100)) + 30 * j, 25, [5000 * k + 30 * j + int(rng.integers(0, 3))]) for j in range(1 + k % 5)])
    big = [(3 * (m // 5), 20, sorted(100_000 + 3 * (m // 5) + 7000 * d + int(rng.integers(0, 2)) for d in range(5))) for m in range(0, 5000, 5)]
    reads.insert(17, big)
    for look in (64, 0):
        want = run(reads, max_lookback=look, min_score=30)
        assert want["max_anchors"] == 5000 and want["V"] == 41 and want["chains"].shape[0] > 10


def raw_dev(start, length, sidx, pos, pidx, chain_capacity, anchor_capacity=None, **params):
    """kiss_hip_fmi_chain_dev itself -> rc, report, chains (n x 6), chain_index, anchors (m x 3), anchor_index"""
    import torch
    import kiss_amd
    from kiss_amd import _lib, fm_chain
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p
    seeds = np.zeros((max(len(start), 1), 4), np.int32)
    seeds[:len(start), 0], seeds[:len(start), 1] = start, length
    V = len(sidx) - 1
    d_seeds = torch.from_numpy(seeds).to(dev)
    d_sidx = torch.from_numpy(np.asarray(sidx, np.int64)).to(dev)
    d_pos = torch.from_numpy(np.concatenate([np.asarray(pos, np.int64), [0]]).astype(np.uint32).view(np.int32)).to(dev)
    d_pidx = torch.from_numpy(np.asarray(pidx, np.int64)).to(dev)
    d_chains = torch.full((max(chain_capacity, 1), 6), -1, dtype=torch.int32, device=dev)
    d_cidx = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    d_anc = d_aidx = None
    if anchor_capacity is not None:
        d_anc = torch.full((max(anchor_capacity, 1), 3), -1, dtype=torch.int32, device=dev)
        d_aidx = torch.full((max(chain_capacity, 0) + 1,), -1, dtype=torch.int64, device=dev)
    rep = _lib.ChainReport()
    p = fm_chain.chain_params(**params)
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        rc = lib.kiss_hip_fmi_chain_dev(ctx._ctx, vp(d_seeds.data_ptr()), vp(d_sidx.data_ptr()), V, vp(d_pos.data_ptr()),
                                        vp(d_pidx.data_ptr()), ctypes.byref(p), vp(d_chains.data_ptr()), vp(d_cidx.data_ptr()),
                                        chain_capacity, vp(d_anc.data_ptr()) if d_anc is not None else None,
                                        vp(d_aidx.data_ptr()) if d_aidx is not None else None, anchor_capacity or 0,
                                        ctypes.byref(rep), None)
    return (rc, rep, d_chains.cpu().numpy(), d_cidx.cpu().numpy(), d_anc.cpu().numpy() if d_anc is not None else None,
            d_aidx.cpu().numpy() if d_aidx is not None else None)


def test_error_contract_of_the_c_call():
    import kiss_amd
    from kiss_amd import _lib
    rng = np.random.default_rng(2)
    reads = [random_read(rng, 40, 200) for _ in range(5)]
    params = dict(max_gap=300, band=30, min_score=20)
    start, length, sidx, pos, pidx = arrays_of(reads)
    want = cm.chain(start, length, sidx, pos, pidx, **params)
    n, m = want["chains"].shape[0], want["anchors"].shape[0]
    assert n > 2 and m > n
    # capacities one short: E_INVALID with the totals in the report, and nothing written
    rc, rep, chains, cidx, anc, aidx = raw_dev(start, length, sidx, pos, pidx, n - 1, m, **params)
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.chains, rep.chain_anchors, rep.anchors) == (n, m, want["n_anchors"])
    assert (chains == -1).all() and (cidx == -1).all() and (anc == -1).all() and (aidx == -1).all()
    rc, rep, chains, cidx, anc, aidx = raw_dev(start, length, sidx, pos, pidx, n, m - 1, **params)
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.chains, rep.chain_anchors) == (n, m)
    assert (chains == -1).all() and (anc == -1).all()
    # with room, and without the anchors
    rc, rep, chains, cidx, anc, aidx = raw_dev(start, length, sidx, pos, pidx, n, m, **params)
    assert rc == 0 and np.array_equal(chains.view(np.uint32).astype(np.int64), want["chains"])
    assert np.array_equal(cidx, want["chain_index"]) and np.array_equal(aidx, want["anchor_index"])
    assert np.array_equal(anc.view(np.uint32).astype(np.int64), want["anchors"])
    assert rep.dp_pairs == want["dp_pairs"] and rep.best_score == want["best_score"] and rep.ms_total > 0
    rc, rep, chains, cidx, anc, aidx = raw_dev(start, length, sidx, pos, pidx, n, None, **params)
    assert rc == 0 and anc is None and np.array_equal(chains.view(np.uint32).astype(np.int64), want["chains"])
    res = kiss_amd.chain_seeds(np.stack([start, length], axis=1), sidx, pos, pidx, want_anchors=False, **params)  # (the host entry)
    assert "anchors" not in res and "anchor_index" not in res
    check(res, want, anchors=False)
    # a seed_index that decreases, a pos_index that decreases, a located seed of length 0
    down = sidx.copy()
    down[2] = down[1] - 1
    assert raw_dev(start, length, down, pos, pidx, n, m, **params)[0] == _lib.KISS_HIP_E_INVALID
    down = pidx.copy()
    down[7] = down[6] - 1
    assert raw_dev(start, length, sidx, pos, down, n, m, **params)[0] == _lib.KISS_HIP_E_INVALID
    zero = length.copy()
    zero[11] = 0
    assert raw_dev(start, zero, sidx, pos, pidx, n, m, **params)[0] == _lib.KISS_HIP_E_INVALID
    # (a seed of length 0 that is not located is not looked at)
    reads[0][3] = (reads[0][3][0], 0, [])
    assert raw_dev(*arrays_of(reads), len(pos), len(pos), **params)[0] == 0
    # the host entry says the same, and the parameters out of range are refused
    for bad in (down, None):
        with pytest.raises(kiss_amd.KissHipError) as e:
            if bad is not None:
                kiss_amd.chain_seeds(np.stack([start, length], axis=1), sidx, pos, bad, **params)
            else:
                kiss_amd.chain_seeds(np.stack([start, zero], axis=1), sidx, pos, pidx, **params)
        assert e.value.status == _lib.KISS_HIP_E_INVALID
    lib = _lib.load()
    buf = np.zeros(64, np.uint64)
    for p in (_lib.ChainParams(max_gap=1 << 31), _lib.ChainParams(band=1 << 31), _lib.ChainParams(gap_cost=65536)):
        assert lib.kiss_hip_fmi_chain_host(buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, ctypes.byref(p),
                                           buf.ctypes.data, buf.ctypes.data, 1, None, None, 0, None, 0) == _lib.KISS_HIP_E_INVALID
    p = _lib.ChainParams()
    assert lib.kiss_hip_fmi_chain_host(buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, ctypes.byref(p),
                                       buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, None, 0, None, 0) == _lib.KISS_HIP_E_INVALID


# ---- (b) FMIndex.chains on the texts ---------------------------------------------------------------------------------------
LENGTHS = (1, 2, 31, 64, 65, 150, 257)
# (min_len, max_len, max_occ) of the seeds, the chain parameters, which reads of the batch
SETS = (((19, 0, 500), dict(), slice(None)),
        ((3, 0, 0), dict(max_gap=400, band=40, gap_cost=5, max_lookback=100, min_score=25), slice(8, 13)))
SA_INTVS = (1, 4, 32)

_indexes = {}


def index_of(name, sa_intv):
    import kiss_amd.fm_index as fm
    if (name, sa_intv) not in _indexes:
        _indexes[(name, sa_intv)] = fm.FMIndex(sa_intv=sa_intv).build(text(name), sa=exact_sa(name), exact_sa=True)
    return _indexes[(name, sa_intv)]


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """a ragged batch per text: per length a random read, one cut from the text, one with substitutions, one with a
    no-base in the middle"""
    S = text(name)
    n = S.size
    rng = np.random.default_rng(23)
    out = []
    for L in LENGTHS:
        out.append(rng.integers(0, 4, L, dtype=np.uint8))
        if n >= L:
            p = int(rng.integers(0, n - L + 1))
            cut = S[p:p + L].copy()
        else:
            cut = rng.integers(0, 4, L, dtype=np.uint8)
        out.append(cut)
        sub = cut.copy()
        for _ in range(max(1, L // 40)):
            j = int(rng.integers(0, L))
            sub[j] = (sub[j] + 1 + rng.integers(0, 3)) & 3
        out.append(sub)
        mid = cut.copy()
        mid[L // 2] = 78  # 'N'
        out.append(mid)
    return out


@functools.lru_cache(maxsize=None)
def model(name, which, both):
    (min_len, max_len, max_occ), params, pick = SETS[which]
    sd = sm.Batch(text(name), reads_of(name)[pick], both, max_len).seeds(min_len, max_occ)
    return cm.chain(sd["start"], sd["len"], sd["seed_index"], sd["positions"], sd["pos_index"], **params), sd


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("sa_intv", SA_INTVS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_chains_of_reads_equal_the_model(name, sa_intv, both):
    f = index_of(name, sa_intv)
    for which, (seed_params, params, pick) in enumerate(SETS):
        want, sd = model(name, which, both)
        res = f.chains(reads_of(name)[pick], *seed_params, both_strands=both, want_anchors=True, **params)
        check(res, want)
        assert res["seed_report"]["seeds"] == sd["len"].size and res["seed_report"]["positions"] == sd["positions"].size
        if which == 0 and sa_intv == 4:  # without the anchors
            res = f.chains(reads_of(name)[pick], *seed_params, both_strands=both, **params)
            assert "anchors" not in res and "anchor_index" not in res
            check(res, want, anchors=False)


def test_the_repeat_texts_give_thousands_of_anchors_per_read():
    for name in ("allA", "periodic"):
        want, _ = model(name, 1, False)
        assert want["max_anchors"] > 2000
    assert model("genome", 0, True)[0]["chains"].shape[0] > 5


def test_chains_need_an_exact_index():
    import kiss_amd.fm_index as fm
    f = fm.FMIndex().build(text("genome"))  # k = 32, like the reference
    with pytest.raises(ValueError, match="exact=True"):
        f.chains(reads_of("genome"))
    f.close()
    with pytest.raises(TypeError):
        index_of("genome", 4).chains(reads_of("genome"), bandwidth=3)
