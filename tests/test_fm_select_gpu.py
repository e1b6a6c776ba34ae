"""kiss_hip_fmi_select_dev / _host against tests/fm_select_model.py, field by field: (a) synthetic alignment records through
kiss_amd.select_alignments, (b) the error contract of the raw device call, (c) FMIndex.map on the texts of the FM tests, the
hits compared with the model run on the alignments the device returned, and one check against the truth."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_select_model as sm
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 257, 5000)
BAND_TOO_WIDE = 1


def check(res, want, key="report"):
    got = np.stack([res["hits"][k].astype(np.int64) for k in sm.HIT_FIELDS], axis=1).reshape(-1, 8)
    assert np.array_equal(np.asarray(res["hit_index"]).astype(np.int64), want["hit_index"]), (res["hit_index"][:8], want["hit_index"][:8])
    assert got.shape == want["hits"].shape, (got.shape, want["hits"].shape)
    for h in np.flatnonzero((got != want["hits"]).any(axis=1))[:3]:
        raise AssertionError("hit %d: %s, the model says %s" % (h, dict(zip(sm.HIT_FIELDS, got[h])), dict(zip(sm.HIT_FIELDS, want["hits"][h]))))
    rep = res[key]
    print({k: rep[k] for k in sm.REPORT_COUNTS})
    assert {k: rep[k] for k in sm.REPORT_COUNTS} == want["report"]


def run(rows, cidx, lens, both=False, bounds=None, alns=None, **params):
    """model and device on the same arrays; alns: what the device gets when it is not `rows` (records in front of the call's)"""
    import kiss_amd
    want = sm.select(rows, cidx, lens, both_strands=both, bounds=bounds, **params)
    res = kiss_amd.select_alignments(np.asarray(rows if alns is None else alns, np.int64).reshape(-1, 12), cidx, lens,
                                     both_strands=both, bounds=bounds, **params)
    check(res, want)
    return want


def rec(score, rbeg, rend, tbeg, tend, flags=0):
    return (score, flags, rbeg, rend, tbeg, tend, 0, 0, 0, 0, 0, 65)


def random_read(rng, count, L, many_heads=False, scores=(40, 50, 60)):
    """`count` records of one read: text starts drawn from a stretch of 8 bases per record, so that most are redundant to an
    earlier one and the kept ones still fill several chunks of 64; many_heads: short read intervals in a long read"""
    out = []
    for _ in range(count):
        if many_heads:
            rb = int(rng.integers(0, L - 30))
            re = rb + int(rng.integers(10, 31))
        else:
            rb = int(rng.integers(0, L // 2))
            re = int(rng.integers(rb + L // 4, L + 1))
        tb = int(rng.integers(0, (2 if many_heads else 8) * count + 200))
        out.append(rec(int(rng.choice(scores)), rb, re, tb, tb + (re - rb) + int(rng.integers(0, 3))))
    return out


@functools.lru_cache(maxsize=None)
def counts_batch(both, many_heads):
    """one read per entry of COUNTS; with both strands the records of a read are split between its two virtual reads"""
    rng = np.random.default_rng(3 + both + 2 * many_heads)
    rows, cidx, lens = [], [0], []
    for c in COUNTS:
        L = 20000 if many_heads else 150
        lens.append(L)
        rows += random_read(rng, c, L, many_heads)
        if both:
            cidx.append(cidx[-1] + int(rng.integers(0, c + 1)))
        cidx.append(len(rows))
    want = sm.select(rows, cidx, lens, both_strands=both, min_score=30)
    return rows, cidx, lens, want


@pytest.mark.parametrize("many_heads", (False, True))
@pytest.mark.parametrize("both", (False, True))
def test_candidate_counts_around_the_chunk_of_64_and_a_read_of_5000(both, many_heads):
    import kiss_amd
    rows, cidx, lens, want = counts_batch(both, many_heads)
    res = kiss_amd.select_alignments(np.array(rows, np.int64), cidx, lens, both_strands=both)
    check(res, want)
    assert want["report"]["max_candidates"] == 5000 and want["report"]["redundant"] > 1000
    per_read = np.diff(want["hit_index"])
    assert per_read[0] == 0 and per_read[1] == 1 and per_read[-1] > 128  # (kept hits in more than two chunks)
    last = want["hits"][want["hit_index"][-2]:]
    if many_heads:  # heads beyond the first chunk, and secondaries that belong to them
        assert ((last[:, 1] & sm.HIT_SECONDARY) == 0).sum() > 64 and (last[(last[:, 1] & sm.HIT_SECONDARY) != 0, 6] >= 64).any()
    else:  # secondaries that arrive after their head's chunk was put away
        assert (last[:64, 5] > 0).any() and ((last[64:, 1] & sm.HIT_SECONDARY) != 0).any()


def test_the_same_batch_behind_a_chain_index_that_does_not_start_at_0():
    import kiss_amd
    rows, cidx, lens, want = counts_batch(True, False)
    res = kiss_amd.select_alignments(np.array(rows, np.int64), [c + 7 for c in cidx], lens, both_strands=True)
    check(res, want)
    # the index form of the read lengths
    ridx = np.concatenate([[5], 5 + np.cumsum(lens)])
    res = kiss_amd.select_alignments(np.array(rows, np.int64), cidx, ("index", ridx), both_strands=True)
    check(res, want)


def test_ten_thousand_light_reads_beside_one_of_5000():
    rng = np.random.default_rng(8)
    rows, cidx, lens = [], [0], []
    for q in range(10001):
        c = 5000 if q == 6000 else int(rng.integers(1, 6))
        lens.append(int(rng.integers(100, 200)))
        rows += random_read(rng, c, lens[-1])
        cidx.append(cidx[-1] + int(rng.integers(0, c + 1)))
        cidx.append(len(rows))
    want = run(rows, cidx, lens, both=True)
    assert want["report"]["mapped"] == 10001 and want["report"]["max_candidates"] == 5000


@pytest.mark.parametrize("share", (0, 1, 128, 255, 256))
def test_overlap_exactly_at_the_threshold(share):
    """intervals of 256 bases, so ov * 256 == share * min exactly when ov == share; the text rule and the read rule apart"""
    rows, cidx, lens = [], [0], []
    expect = []
    for more in (0, 1):
        ov = share + more
        if ov > 256:
            continue
        # text rule: same strand, read intervals apart, text intervals share ov bases
        rows += [rec(60, 0, 256, 1000, 1256), rec(50, 600, 900, 1256 - ov, 1256 - ov + 300)]
        expect.append("redundant" if more else "head")
        # read rule: text intervals apart, read intervals share ov bases
        rows += [rec(60, 0, 256, 1000, 1256), rec(50, 256 - ov, 256 - ov + 300, 5000, 5300)]
        expect.append("secondary" if more else "head")
        lens += [1000, 1000]
        cidx += [len(rows) - 2, len(rows)]
    want = run(rows, cidx, lens, overlap=share)
    for q, what in enumerate(expect):
        mine = want["hits"][want["hit_index"][q]:want["hit_index"][q + 1]]
        if what == "redundant":
            assert len(mine) == 1
        else:
            assert len(mine) == 2 and bool(mine[1][1] & sm.HIT_SECONDARY) == (what == "secondary")
            assert bool(mine[1][1] & sm.HIT_SUPPLEMENTARY) == (what == "head")
    # opposite strands never make each other redundant, and do share the read
    rows = [rec(60, 0, 256, 1000, 1256), rec(50, 0, 256, 1000, 1256)]
    want = run(rows, [0, 1, 2], [256], both=True, overlap=share)
    assert len(want["hits"]) == 2 and bool(want["hits"][1][1] & sm.HIT_SECONDARY) == (share < 256)


def test_order_dependence_two_heads_and_the_reverse_frame():
    rows, cidx, lens = [], [0], []
    # A > B > C: B is redundant to A, C overlaps only B in the text: C is kept
    rows += [rec(60, 0, 10, 100, 120), rec(50, 0, 10, 115, 135), rec(40, 0, 10, 128, 148)]
    lens.append(50)
    cidx += [3, 3]
    # a secondary that overlaps two heads belongs to the first in hit order, not in read order
    rows += [rec(50, 0, 50, 1000, 1050), rec(60, 60, 110, 2000, 2050), rec(40, 20, 90, 3000, 3070)]
    lens.append(150)
    cidx += [6, 6]
    # L = 150: forward [0, 50) and reverse virtual [0, 50) are two heads, reverse virtual [100, 150) is a secondary
    rows += [rec(50, 0, 50, 1000, 1050), rec(45, 0, 50, 5000, 5050), rec(40, 100, 150, 9000, 9050)]
    lens.append(150)
    cidx += [7, 9]
    want = run(rows, cidx, lens, both=True, overlap=0, min_score=1)
    h = want["hits"]
    assert [list(r[:2]) for r in h[0:2]] == [[0, 0], [2, sm.HIT_SECONDARY]] and want["report"]["redundant"] == 1
    assert [list(r[(0, 1, 6),]) for r in h[2:5]] == [[4, 0, 0], [3, sm.HIT_SUPPLEMENTARY, 1], [5, sm.HIT_SECONDARY, 0]]
    assert [list(r[(0, 1, 6),]) for r in h[5:8]] == [[6, 0, 0], [7, sm.HIT_REVERSE | sm.HIT_SUPPLEMENTARY, 1],
                                                     [8, sm.HIT_REVERSE | sm.HIT_SECONDARY, 0]]
    want = run(rows, cidx, lens, both=True, overlap=128, min_score=1)
    assert [list(r[(0, 1, 6),]) for r in want["hits"][3:6]] == [[4, 0, 0], [3, sm.HIT_SUPPLEMENTARY, 1], [5, sm.HIT_SECONDARY, 0]]


def test_records_that_are_skipped():
    rows = [rec(0, 0, 0, 0, 0, flags=BAND_TOO_WIDE), rec(0, 0, 0, 0, 0), rec(29, 0, 100, 500, 600), rec(30, 0, 100, 900, 1000),
            rec(500, 0, 100, 100, 200, flags=BAND_TOO_WIDE), rec(0, 0, 0, 0, 0)]
    want = run(rows, [0, 5, 6], [100, 100])
    assert [int(r[0]) for r in want["hits"]] == [3] and list(want["hit_index"]) == [0, 1, 1] and want["report"]["candidates"] == 1
    want = run(rows, [0, 5, 6], [100, 100], min_score=0)  # a score of 0 is never a candidate
    assert [int(r[0]) for r in want["hits"]] == [3, 2] and want["report"]["mapped"] == 1


def test_bounds():
    top = (1 << 32) - 4097
    # R = 1: the whole text is one record
    rows = [rec(50, 0, 100, 0, 100), rec(45, 0, 100, 900, 1000), rec(44, 0, 100, 901, 1001), rec(43, 0, 100, 1000, 1100)]
    want = run(rows, [0, 4], [100], bounds=[0, 1000])
    assert want["report"]["spanning"] == 2 and [int(r[0]) for r in want["hits"]] == [0, 1]
    # R = 2: tend == bounds[rho + 1] is kept, one more base is spanning; tbeg == bounds[rho] belongs to rho
    rows = [rec(50, 0, 100, 400, 500), rec(49, 0, 100, 401, 501), rec(48, 0, 100, 500, 600), rec(47, 0, 100, 499, 599),
            rec(46, 0, 100, top - 100, top), rec(45, 0, 100, top - 99, top + 1), rec(44, 0, 100, top, top + 50)]
    want = run(rows, [0, 7], [100], bounds=[0, 500, top])
    assert [(int(r[0]), int(r[7])) for r in want["hits"]] == [(0, 0), (2, 1), (4, 1)] and want["report"]["spanning"] == 4
    # R = 1000 (but for cuts drawn twice), the records end at 2^32 - 4097
    rng = np.random.default_rng(5)
    bounds = [0] + [int(c) for c in np.unique(rng.integers(1, top, 999))] + [top]
    R = len(bounds) - 1
    rows, cidx, lens = [], [0], []
    for q in range(300):
        for _ in range(int(rng.integers(1, 6))):
            rho = int(rng.integers(0, R))
            edge = int(rng.integers(0, 5))
            width = min(100, bounds[rho + 1] - bounds[rho])
            tb = (bounds[rho], bounds[rho + 1] - width, bounds[rho + 1] - width + 1, max(0, bounds[rho] - 1),
                  int(rng.integers(bounds[rho], bounds[rho + 1])))[edge]
            rows.append(rec(int(rng.integers(30, 90)), 0, 100, tb, tb + width))
        lens.append(100)
        cidx.append(len(rows))
    want = run(rows, cidx, lens, bounds=bounds)
    assert want["report"]["spanning"] > 50 and len(set(int(r[7]) for r in want["hits"])) > 100 and R > 990


def test_mapq():
    big = (1 << 30) - 1
    rows = [rec(big, 0, 10, 0, 10), rec(big // 2, 0, 10, 50, 60), rec(big, 20, 30, 100, 110), rec(big, 20, 30, 200, 210),
            rec(big - 1, 40, 50, 300, 310), rec(big - 2, 40, 50, 400, 410), rec(77, 60, 70, 500, 510)]
    want = run(rows, [0, 7], [80], mapq_coef=65535, mapq_max=255)
    by_aln = {int(r[0]): r for r in want["hits"]}
    assert int(by_aln[0][2]) == 255 and int(by_aln[2][2]) == 0 and int(by_aln[4][2]) == 0 and int(by_aln[6][2]) == 255
    want = run(rows, [0, 7], [80], mapq_coef=65535, mapq_max=0)
    assert not want["hits"][:, 2].any()
    want = run(rows, [0, 7], [80], mapq_coef=0, mapq_max=60)
    assert not want["hits"][:, 2].any()
    want = run(rows, [0, 7], [80], mapq_coef=3, mapq_max=60)  # (no secondary: min(mapq_max, mapq_coef))
    assert int({int(r[0]): r for r in want["hits"]}[6][2]) == 3


@pytest.mark.parametrize("max_hits", (0, 1, 2, 1000))
def test_max_hits(max_hits):
    rows, cidx, lens, full = counts_batch(True, False)
    sub = slice(0, cidx[2 * 8])  # the reads of 0 .. 129 candidates
    want = run(rows[sub], cidx[:2 * 8 + 1], lens[:8], both=True, max_hits=max_hits)
    for q in range(8):
        a, b = full["hit_index"][q], full["hit_index"][q + 1]
        n = min(b - a, max_hits) if max_hits else b - a
        assert want["hit_index"][q + 1] - want["hit_index"][q] == n
        assert np.array_equal(want["hits"][want["hit_index"][q]:want["hit_index"][q + 1]], full["hits"][a:a + n])


# ---- (b) the error contract of the C call ------------------------------------------------------------------------------------
def raw_dev(rows, cidx, ridx, Q, hit_capacity, both=False, bounds=None, params=None, null=(), **kw):
    """kiss_hip_fmi_select_dev itself -> rc, report, hits (n x 8), hit_index"""
    import torch
    import kiss_amd
    from kiss_amd import _lib, fm_select
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p
    al = np.asarray(rows, np.int64).reshape(-1, 12).astype(np.uint32)
    if al.shape[0] == 0:
        al = np.zeros((1, 12), np.uint32)
    d_alns = torch.from_numpy(al.view(np.int32)).to(dev)
    d_cidx = torch.from_numpy(np.asarray(cidx, np.int64)).to(dev)
    d_ridx = torch.from_numpy(np.asarray(ridx, np.int64)).to(dev)
    d_bounds = torch.from_numpy(np.asarray(bounds, np.uint64).view(np.int64)).to(dev) if bounds is not None else None
    d_hits = torch.full((max(hit_capacity, 1), 8), -1, dtype=torch.int32, device=dev)
    d_hidx = torch.full((Q + 1,), -1, dtype=torch.int64, device=dev)
    rep = _lib.SelectReport()
    p = params if params is not None else fm_select.select_params(**kw)
    ptr = dict(alns=vp(d_alns.data_ptr()), cidx=vp(d_cidx.data_ptr()), ridx=vp(d_ridx.data_ptr()), hits=vp(d_hits.data_ptr()),
               hidx=vp(d_hidx.data_ptr()))
    for k in null:
        ptr[k] = None
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        rc = lib.kiss_hip_fmi_select_dev(ctx._ctx, ptr["alns"], ptr["cidx"], ptr["ridx"], Q, 1 if both else 0,
                                         vp(d_bounds.data_ptr()) if d_bounds is not None else None,
                                         len(bounds) - 1 if bounds is not None else 0, ctypes.byref(p) if "params" not in null else None,
                                         ptr["hits"], ptr["hidx"], hit_capacity, ctypes.byref(rep), None)
    return rc, rep, d_hits.cpu().numpy(), d_hidx.cpu().numpy()


def test_error_contract_of_the_c_call():
    import kiss_amd
    from kiss_amd import _lib
    rng = np.random.default_rng(21)
    rows, cidx, lens = [], [0], []
    for c in (3, 0, 70, 5):
        lens.append(150)
        rows += random_read(rng, c, 150)
        cidx.append(len(rows))
    ridx = [0, 150, 300, 450, 600]
    want = sm.select(rows, cidx, lens)
    total = int(want["report"]["hits"])
    assert total > 8
    # capacity one short: E_INVALID with the totals in the report, and nothing written
    rc, rep, hits, hidx = raw_dev(rows, cidx, ridx, 4, total - 1)
    assert rc == _lib.KISS_HIP_E_INVALID
    assert {k: getattr(rep, k) for k in sm.REPORT_COUNTS} == want["report"]
    assert (hits == -1).all() and (hidx == -1).all()
    # with room
    rc, rep, hits, hidx = raw_dev(rows, cidx, ridx, 4, total)
    assert rc == 0 and np.array_equal(hits[:total].view(np.uint32).astype(np.int64), want["hits"])
    assert np.array_equal(hidx, want["hit_index"]) and rep.ms_total > 0 and rep.ms_walk > 0
    rc, rep, hits, hidx = raw_dev(rows, cidx, ridx, 4, total + 5)
    assert rc == 0 and (hits[total:] == -1).all()
    # a chain_index that decreases, a read_index that decreases, a read of length 0
    assert raw_dev(rows, [0, 3, 2, 73, 78], ridx, 4, total)[0] == _lib.KISS_HIP_E_INVALID
    assert raw_dev(rows, cidx, [0, 150, 100, 450, 600], 4, total)[0] == _lib.KISS_HIP_E_INVALID
    assert raw_dev(rows, cidx, [0, 150, 150, 450, 600], 4, total)[0] == _lib.KISS_HIP_E_INVALID
    with pytest.raises(kiss_amd.KissHipError) as e:
        kiss_amd.select_alignments(np.array(rows, np.int64), [0, 3, 2, 73, 78], lens)
    assert e.value.status == _lib.KISS_HIP_E_INVALID
    # bounds that do not start at 0, that do not ascend strictly
    assert raw_dev(rows, cidx, ridx, 4, total, bounds=[0, 5000, 50000])[0] == 0
    assert raw_dev(rows, cidx, ridx, 4, total, bounds=[1, 5000, 50000])[0] == _lib.KISS_HIP_E_INVALID
    assert raw_dev(rows, cidx, ridx, 4, total, bounds=[0, 5000, 5000])[0] == _lib.KISS_HIP_E_INVALID
    assert raw_dev(rows, cidx, ridx, 4, total, bounds=[0, 5000, 4000, 50000])[0] == _lib.KISS_HIP_E_INVALID
    # a required pointer NULL, a parameter over its limit
    for k in ("alns", "cidx", "ridx", "hits", "hidx", "params"):
        assert raw_dev(rows, cidx, ridx, 4, total, null=(k,))[0] == _lib.KISS_HIP_E_INVALID, k
    for p in (_lib.SelectParams(overlap=257), _lib.SelectParams(mapq_coef=65536), _lib.SelectParams(mapq_max=256)):
        rc, rep, hits, hidx = raw_dev(rows, cidx, ridx, 4, total, params=p)
        assert rc == _lib.KISS_HIP_E_INVALID and (hits == -1).all() and (hidx == -1).all()
    # no reads, no alignments
    rc, rep, hits, hidx = raw_dev([], [0], [0], 0, 0)
    assert rc == 0 and list(hidx) == [0] and rep.hits == 0
    rc, rep, hits, hidx = raw_dev([], [9, 9, 9, 9, 9], ridx, 4, 0)
    assert rc == 0 and list(hidx) == [0] * 5 and (rep.alignments, rep.hits, rep.Q) == (0, 0, 4)
    res = kiss_amd.select_alignments(np.zeros((0, 12), np.int64), [0], [], both_strands=True)
    assert res["hits"].shape == (0,) and list(res["hit_index"]) == [0] and res["report"]["V"] == 0


# ---- (c) FMIndex.map -----------------------------------------------------------------------------------------------------------
SELECT_SETS = (dict(), dict(min_score=20, overlap=64, mapq_coef=200, mapq_max=100, max_hits=3))


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_hits_of_reads_equal_the_model_on_the_alignments_of_the_device(name, both):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    f = index_of(name, 4)
    S = text(name)
    reads = reads_of(name)
    lens = [r.size for r in reads]
    for params in SELECT_SETS:
        res = f.map(reads, S, 15, 0, 200, both_strands=both, chain_params=dict(min_score=25, band=100), **params)
        want = sm.select(res["alignments"], res["chain_index"], lens, both_strands=both, **params)
        check(res, want, key="select_report")
        assert res["select_report"]["alignments"] == res["alignments"].shape[0] == res["align_report"]["chains"]
        assert "cigar" in res and "seed_report" in res
    if name in ("genome", "iid"):
        assert res["select_report"]["mapped"] >= 4


def revcomp(R):
    return (3 - np.asarray(R, np.uint8)[::-1]).astype(np.uint8)


TRUTH_SEED = 17


@functools.lru_cache(maxsize=None)
def truth_case(kind):
    """a random text of 20 000 bases ("unique"), or one that holds a 500-base block twice, 10 000 bases apart ("repeat");
    40 reads of 150 bases with 2 % substitutions, every second one reverse-complemented -> text, reads, true starts"""
    rng = np.random.default_rng(TRUTH_SEED)
    S = rng.integers(0, 4, 20000, dtype=np.uint8)
    if kind == "repeat":
        S[12000:12500] = S[2000:2500]
    reads, starts = [], []
    for q in range(40):
        p = int(rng.integers(2000, 2351)) if kind == "repeat" else int(rng.integers(0, S.size - 150))
        R = S[p:p + 150].copy()
        for j in rng.choice(150, 3, replace=False):
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        reads.append(revcomp(R) if q % 2 else R)
        starts.append(p)
    return S, reads, starts


def test_against_the_truth_unique_reads_and_a_block_that_occurs_twice():
    """Every read of the random text: the primary has the true strand, starts within the align band (32) of the true start
    and has mapq = mapq_max.  Every read from the block that occurs twice: mapq 0 and a secondary.  The conditions hold
    on this seed in the four CPU models composed: tests/test_fm_select_truth_model.py."""
    import kiss_amd.fm_index as fm
    import kiss_amd
    for kind in ("unique", "repeat"):
        S, reads, starts = truth_case(kind)
        with kiss_amd.Context(max_n=1 << 20) as ctx:
            sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
        f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
        res = f.map(reads, S, both_strands=True)
        hits, hidx = res["hits"], res["hit_index"]
        want = sm.select(res["alignments"], res["chain_index"], [150] * len(reads), both_strands=True)
        check(res, want, key="select_report")
        for q, p in enumerate(starts):
            mine = hits[int(hidx[q]):int(hidx[q + 1])]
            assert len(mine) >= 1, (kind, q)
            first = mine[0]
            assert first["flags"] & ~np.uint32(sm.HIT_REVERSE) == 0 and bool(first["flags"] & sm.HIT_REVERSE) == bool(q % 2), (kind, q)
            tbeg = int(res["alignments"]["tbeg"][first["aln"]])
            if kind == "unique":
                assert abs(tbeg - p) <= 32 and first["mapq"] == 60 and first["n_sec"] == 0, (kind, q, tbeg, p, first)
            else:
                assert min(abs(tbeg - p), abs(tbeg - p - 10000)) <= 32 and first["mapq"] == 0 and first["n_sec"] >= 1, (kind, q, first)
        f.close()
