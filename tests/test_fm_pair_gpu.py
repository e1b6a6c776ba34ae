"""kiss_hip_fmi_pair_dev / _host against tests/fm_pair_model.py, every field of every record and the report's counts: (a)
synthetic hit and alignment arrays through kiss_amd.pair_hits, (b) the error contract of the raw device call, (c)
FMIndex.map_pairs on the texts of the FM tests, the pairs compared with the model run on the hits and alignments the device
returned, and one check against the truth: mates from a block that occurs twice, anchored by their partners."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_pair_model as pm
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 300)
TOP = (1 << 32) - 4097
BIG = (1 << 30) - 1
F = dict(zip(pm.PAIR_FIELDS, range(10)))


def check(res, want, key="report"):
    got = np.stack([res["pairs"][k].astype(np.int64) for k in pm.PAIR_FIELDS], axis=1).reshape(-1, 10)
    assert got.shape == want["pairs"].shape, (got.shape, want["pairs"].shape)
    for p in np.flatnonzero((got != want["pairs"]).any(axis=1))[:3]:
        raise AssertionError("pair %d: %s, the model says %s" % (p, dict(zip(pm.PAIR_FIELDS, got[p])), dict(zip(pm.PAIR_FIELDS, want["pairs"][p]))))
    rep = res[key]
    print({k: rep[k] for k in pm.REPORT_COUNTS})
    assert {k: rep[k] for k in pm.REPORT_COUNTS} == want["report"]


def run(pairs, first_aln=0, **params):
    """model and device on the same arrays -> what the model says"""
    import kiss_amd
    hits, hidx, alns = pm.batch_of(pairs, first_aln)
    want = pm.pair(hits, hidx, alns, **params)
    res = kiss_amd.pair_hits(np.array(hits, np.int64).reshape(-1, 8), hidx, np.array(alns, np.int64).reshape(-1, 12), **params)
    check(res, want)
    return want


def records(want):
    return [dict(zip(pm.PAIR_FIELDS, (int(v) for v in r))) for r in want["pairs"]]


def random_mate(rng, count, forward, span=1500, extra=0):
    """`count` eligible hits, most of them on the strand `forward` says, and `extra` that never pair (supplementary heads,
    their secondaries, empty intervals) at places other than hit number 0"""
    out = []
    for i in range(count):
        tb = int(rng.integers(0, span))
        rev = int(rng.random() < 0.15) ^ (0 if forward else 1)
        out.append((tb, tb + int(rng.integers(1, 160)), rev, int(rng.choice((40, 50, 60, 61))), int(rng.random() < 0.2), 0,
                    int(rng.integers(0, 61)) if i == 0 else 0))
    for _ in range(extra if count else 0):
        at = int(rng.integers(1, len(out) + 1))
        tb = int(rng.integers(0, span))
        kind = int(rng.integers(0, 2))
        out.insert(at, (tb, tb + 100, int(rng.integers(0, 2)), 150, 0, at, 0) if kind == 0 else (tb + 50, tb, int(rng.integers(0, 2)), 150, 0, 0, 0))
    # a head field says where the head is: keep the ones written above pointing at something that is not hit 0
    return [h if h[5] == 0 else h[:5] + (max(1, min(h[5], len(out) - 1)),) + h[6:] for h in out]


@functools.lru_cache(maxsize=None)
def crossed_batch():
    rng = np.random.default_rng(12)
    pairs = []
    for c1 in COUNTS:
        for c2 in COUNTS:
            pairs.append((random_mate(rng, c1, True, extra=2 if c1 in (3, 64, 300) else 0),
                          random_mate(rng, c2, False, extra=3 if c2 in (2, 65, 129) else 0)))
    hits, hidx, alns = pm.batch_of(pairs)
    return hits, hidx, alns, pm.pair(hits, hidx, alns)


def test_eligible_counts_around_the_chunk_of_64_crossed():
    import kiss_amd
    hits, hidx, alns, want = crossed_batch()
    res = kiss_amd.pair_hits(np.array(hits, np.int64), hidx, np.array(alns, np.int64))
    check(res, want)
    rep = want["report"]
    assert rep["max_combinations"] == 300 * 300 and rep["proper"] >= 60 and rep["promoted"] > 60 and rep["lifted"] > 30
    rec = records(want)
    big = rec[-1]
    first1, first2 = hidx[-3], hidx[-2]
    assert big["flags"] & pm.PROPER and big["n_conc"] > 5000 and big["sub1"] == big["sub2"] == big["score"]
    # somewhere the best combination lies in a chunk after the first, on either side
    assert any(r["flags"] & pm.PROPER and r["hit1"] - hidx[2 * p] >= 64 for p, r in enumerate(rec))
    assert any(r["flags"] & pm.PROPER and r["hit2"] - hidx[2 * p + 1] >= 64 for p, r in enumerate(rec))
    assert first2 - first1 >= 300


def test_the_same_batch_behind_a_hit_index_that_does_not_start_at_0_and_structured_input():
    import kiss_amd
    from kiss_amd.fm_align import ALN_DTYPE
    from kiss_amd.fm_select import HIT_DTYPE
    hits, hidx, alns, want = crossed_batch()
    lead = 5
    ht = np.zeros(lead + len(hits), HIT_DTYPE)
    ht[lead:] = np.array(hits, np.uint32).view(HIT_DTYPE).reshape(-1)
    ht["aln"][:lead] = 0xFFFFFFFF  # (hits in front of the first segment are nobody's)
    al = np.array(alns, np.uint32).view(ALN_DTYPE).reshape(-1)
    res = kiss_amd.pair_hits(ht, [h + lead for h in hidx], al)
    moved = want["pairs"].copy()
    for k in ("hit1", "hit2"):
        col = moved[:, F[k]]
        col[col != pm.NONE] += lead
    check(res, dict(pairs=moved, report=want["report"]))


def test_ten_thousand_light_pairs_beside_one_of_300_by_300():
    rng = np.random.default_rng(14)
    pairs = []
    for p in range(10001):
        if p == 7000:
            pairs.append((random_mate(rng, 300, True), random_mate(rng, 300, False)))
        else:
            pairs.append((random_mate(rng, int(rng.integers(0, 4)), p % 2 == 0, span=600), random_mate(rng, int(rng.integers(0, 4)), p % 2 == 1, span=600)))
    want = run(pairs)
    assert want["report"]["P"] == 10001 and want["report"]["max_combinations"] == 90000 and want["report"]["proper"] > 1000


def test_ties_and_the_chunk_the_best_and_the_subs_come_from():
    fw = lambda tb, s, rev=0: (tb, tb + 150, rev, s)  # noqa: E731
    # ties in S: four equal combinations, then a tie that only y breaks, then one that only x breaks
    t1 = ([fw(1000, 140), fw(1000, 140)], [fw(1250, 145, 1), fw(1250, 145, 1)])
    t2 = ([fw(1000, 140)], [fw(1250, 100, 1), fw(1250, 145, 1), fw(1250, 145, 1)])
    t3 = ([fw(9000, 10), fw(1000, 140), fw(1000, 140)], [fw(1250, 145, 1)])
    # mate 1 with 200 hits, mate 2 with 140: the only good combination is (x, y) = (150, 139); the second best pairs of x' != x
    # and of y' != y lie in the first chunks: sub1 from (3, 139), sub2 from (150, 70)
    m1 = [fw(50000 + 400 * i, 60) for i in range(200)]
    m2 = [fw(900000 + 2000 * i, 60, 1) for i in range(140)]  # (far from every forward hit)
    m1[150] = fw(20000, 140)
    m2[139] = fw(20250, 145, 1)
    m1[3] = fw(20010, 100)
    m2[70] = fw(20260, 90, 1)
    t4 = (m1, m2)
    want = run([t1, t2, t3, t4])
    r = records(want)
    hidx = pm.batch_of([t1, t2, t3, t4])[1]
    assert (r[0]["hit1"], r[0]["hit2"], r[0]["n_conc"], r[0]["sub1"], r[0]["sub2"], r[0]["mapq1"]) == (0, 2, 4, 285, 285, 0)
    assert (r[1]["hit1"] - hidx[2], r[1]["hit2"] - hidx[3], r[1]["sub1"], r[1]["sub2"]) == (0, 1, 0, 285)
    assert (r[2]["hit1"] - hidx[4], r[2]["hit2"] - hidx[5], r[2]["sub1"], r[2]["sub2"]) == (1, 0, 285, 0)
    assert (r[3]["hit1"] - hidx[6], r[3]["hit2"] - hidx[7]) == (150, 139) and r[3]["score"] == 285 and r[3]["n_conc"] == 4
    assert r[3]["sub1"] == 245 and r[3]["sub2"] == 230 and r[3]["flags"] & (pm.PROMOTED1 | pm.PROMOTED2) == pm.PROMOTED1 | pm.PROMOTED2


def test_what_keeps_two_hits_from_pairing_and_the_edges_of_the_number_formats():
    pairs = [
        ([(1000, 1150, 0, 100, 0)], [(1250, 1400, 1, 100, 1)]),                 # another record
        ([(1000, 1150, 0, 100)], [(1250, 1400, 0, 100)]),                       # equal strands, forward
        ([(1000, 1150, 1, 100)], [(1250, 1400, 1, 100)]),                       # equal strands, reverse
        ([(1000, 1400, 0, 100)], [(1100, 1300, 1, 100)]),                       # the reverse hit inside the forward one: f.tend > r.tend
        ([(1100, 1300, 0, 100)], [(1000, 1400, 1, 100)]),                       # f.tbeg > r.tbeg
        ([(1000, 1150, 1, 100)], [(1250, 1400, 0, 100)]),                       # the mates face away from each other
        ([(1250, 1400, 1, 100)], [(1000, 1150, 0, 100)]),                       # mate 2 forward, mate 1 reverse: proper
        ([(TOP - 400, TOP - 250, 0, 100)], [(TOP - 150, TOP, 1, 100)]),         # the end of the largest text
        ([(TOP - 400, TOP - 250, 0, BIG)], [(TOP - 150, TOP, 1, BIG)]),         # the largest scores
        ([(0, 150, 0, BIG)], [(TOP - 150, TOP, 1, BIG)]),                       # T = TOP: too long
        ([(1000, 1150, 0, 100), (1000, 1150, 0, 150, 0, 1)], [(1250, 1400, 1, 100), (1250, 1400, 1, 150, 0, 1), (1250, 1400, 1, 150, 0, 1)]),  # heads 1
        ([(1150, 1000, 0, 100), (1000, 1150, 0, 90)], [(1400, 1400, 1, 100), (1250, 1400, 1, 80)]),  # tend <= tbeg in hit 0
        ([(1500, 1000, 0, 100)], [(1400, 1250, 1, 100)]),                       # ... and nothing else: max(tend) < min(tbeg), tlen 0
        ([], []), ([(1000, 1150, 0, 100, 2, 0, 33)], []), ([], [(1000, 1150, 1, 100, 0, 0, 44)]),
    ]
    want = run(pairs, first_aln=3)
    r = records(want)
    proper = [bool(x["flags"] & pm.PROPER) for x in r]
    assert proper == [False] * 6 + [True] * 3 + [False] + [True, True] + [False] * 4
    assert r[0]["flags"] == pm.MATE1_MAPPED | pm.MATE2_MAPPED and r[0]["tlen"] == 0 and r[1]["tlen"] == 400
    assert r[7]["tlen"] == 400 and r[8]["score"] == 2 * BIG and r[8]["mapq1"] == 60 and r[9]["tlen"] == TOP
    assert r[10]["score"] == 200 and r[10]["n_conc"] == 1 and not r[10]["flags"] & (pm.PROMOTED1 | pm.PROMOTED2)
    assert r[11]["score"] == 170 and r[11]["flags"] & pm.PROMOTED1 and r[11]["flags"] & pm.PROMOTED2
    assert r[12]["tlen"] == 0 and r[12]["score"] == 200
    assert (r[13]["hit1"], r[13]["hit2"], r[13]["flags"]) == (pm.NONE, pm.NONE, 0)
    assert (r[14]["hit2"], r[14]["flags"], r[14]["mapq1"], r[14]["score"]) == (pm.NONE, pm.MATE1_MAPPED, 33, 100)
    assert (r[15]["hit1"], r[15]["flags"], r[15]["mapq2"]) == (pm.NONE, pm.MATE2_MAPPED, 44)


def test_bad_input_spoils_its_own_pair_only():
    import kiss_amd
    rng = np.random.default_rng(15)
    pairs = [(random_mate(rng, c1, True), random_mate(rng, c2, False)) for c1, c2 in ((3, 3), (70, 2), (2, 70), (1, 1), (3, 3), (3, 3))]
    hits, hidx, alns = pm.batch_of(pairs)
    hits = [list(h) for h in hits]
    hits[hidx[2] + 68][0] = len(alns)            # pair 1: an aln one past the end, in the second chunk of mate 1
    hits[hidx[5] + 69][0] = 0xFFFFFFFF           # pair 2: far out, mate 2
    hits[hidx[6]][3] = 1 << 30                   # pair 3: a score select never writes
    hits[hidx[9] + 1][0] = len(alns)             # pair 4: a hit that would not be eligible (made a supplementary head) still counts
    hits[hidx[9] + 1][6] = 1
    want = pm.pair(hits, hidx, alns)
    res = kiss_amd.pair_hits(np.array(hits, np.int64), hidx, np.array(alns, np.int64))
    check(res, want)
    assert [int(f) for f in want["pairs"][:, F["flags"]]][1:5] == [pm.BAD_INPUT] * 4 and want["report"]["bad_input"] == 4
    assert not want["pairs"][0][F["flags"]] & pm.BAD_INPUT and not want["pairs"][5][F["flags"]] & pm.BAD_INPUT
    assert want["report"]["eligible"] == 12
    assert not want["pairs"][1:5, (0, 1, 3, 4, 5, 6, 7, 8, 9)].any()


PARAM_SETS = (dict(), dict(pen_coef=0), dict(ins_min=400, ins_max=400), dict(ins_min=100, ins_max=700, ins_mean=250, pen_coef=300, pen_max=45),
              dict(ins_max=0xFFFFFFFF, ins_mean=0xFFFFFFFF, pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255))


@pytest.mark.parametrize("which", range(len(PARAM_SETS)))
def test_parameter_sets(which):
    rng = np.random.default_rng(16)
    pairs = [(random_mate(rng, c1, p % 2 == 0, span=700, extra=p % 3), random_mate(rng, c2, p % 2 == 1, span=700))
             for p, (c1, c2) in enumerate(((1, 1), (2, 3), (5, 4), (9, 9), (66, 3), (4, 70), (20, 20), (0, 3)))]
    # inserts of exactly 400 among them
    pairs += [([(3000, 3150, 0, 90), (5000, 5150, 0, 90)], [(3250, 3400, 1, 95), (5251, 5401, 1, 95)])]
    want = run(pairs, **PARAM_SETS[which])
    assert want["report"]["proper"] >= (1 if which == 2 else 5)


# ---- (b) the error contract of the C call, and _dev against _host -----------------------------------------------------------------
def raw_dev(hits, hidx, alns, Q, params=None, null=(), aln_count=None, **kw):
    """kiss_hip_fmi_pair_dev itself -> rc, report, pairs (P x 10, -1 where nothing was written)"""
    import torch
    import kiss_amd
    from kiss_amd import _lib, fm_pair
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p
    ht = np.asarray(hits, np.int64).reshape(-1, 8).astype(np.uint32)
    al = np.asarray(alns, np.int64).reshape(-1, 12).astype(np.uint32)
    n_aln = al.shape[0] if aln_count is None else aln_count
    d_hits = torch.from_numpy((ht if ht.size else np.zeros((1, 8), np.uint32)).view(np.int32)).to(dev)
    d_alns = torch.from_numpy((al if al.size else np.zeros((1, 12), np.uint32)).view(np.int32)).to(dev)
    d_hidx = torch.from_numpy(np.asarray(hidx, np.int64)).to(dev)
    d_pairs = torch.full((max(Q // 2, 1), 10), -1, dtype=torch.int32, device=dev)
    rep = _lib.PairReport()
    p = params if params is not None else fm_pair.pair_params(**kw)
    ptr = dict(hits=vp(d_hits.data_ptr()), hidx=vp(d_hidx.data_ptr()), alns=vp(d_alns.data_ptr()), pairs=vp(d_pairs.data_ptr()))
    for k in null:
        ptr[k] = None
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        rc = lib.kiss_hip_fmi_pair_dev(ctx._ctx, ptr["hits"], ptr["hidx"], Q, ptr["alns"], n_aln, ctypes.byref(p) if "params" not in null else None,
                                       ptr["pairs"], ctypes.byref(rep), None)
    return rc, rep, d_pairs.cpu().numpy()


def test_error_contract_of_the_c_call_and_dev_equals_host():
    import kiss_amd
    from kiss_amd import _lib
    rng = np.random.default_rng(22)
    pairs = [(random_mate(rng, c1, True, extra=1), random_mate(rng, c2, False)) for c1, c2 in ((3, 2), (0, 4), (70, 5), (2, 2))]
    hits, hidx, alns = pm.batch_of(pairs)
    want = pm.pair(hits, hidx, alns)
    assert want["report"]["proper"] >= 2
    # with everything in order: the records of the model, the report, the times; the host entry gives the same
    rc, rep, got = raw_dev(hits, hidx, alns, 8)
    assert rc == 0 and np.array_equal(got.view(np.uint32).astype(np.int64), want["pairs"])
    assert {k: getattr(rep, k) for k in pm.REPORT_COUNTS} == want["report"] and rep.ms_total > 0 and rep.ms_pair > 0
    host = kiss_amd.pair_hits(np.array(hits, np.int64), hidx, np.array(alns, np.int64))
    check(host, want)
    assert np.array_equal(np.stack([host["pairs"][k] for k in pm.PAIR_FIELDS], axis=1), got.view(np.uint32))
    # Q odd, a hit_index that decreases: nothing written
    for bad_q, bad_idx in ((7, hidx[:8]), (8, hidx[:3] + [hidx[3] - 1] + hidx[4:]), (8, [hidx[0] + 1] + hidx[1:2] + [0] + hidx[3:])):
        rc, rep, got = raw_dev(hits, bad_idx, alns, bad_q)
        assert rc == _lib.KISS_HIP_E_INVALID and (got == -1).all(), (bad_q, bad_idx)
    with pytest.raises(kiss_amd.KissHipError) as e:
        kiss_amd.pair_hits(np.array(hits, np.int64), hidx[:3] + [hidx[3] - 1] + hidx[4:], np.array(alns, np.int64))
    assert e.value.status == _lib.KISS_HIP_E_INVALID
    with pytest.raises(ValueError):
        kiss_amd.pair_hits(np.array(hits, np.int64), hidx[:8], np.array(alns, np.int64))
    # a required pointer NULL, a parameter over its limit, ins_min > ins_max
    for k in ("hits", "hidx", "alns", "pairs", "params"):
        assert raw_dev(hits, hidx, alns, 8, null=(k,))[0] == _lib.KISS_HIP_E_INVALID, k
    for p in (_lib.PairParams(ins_max=9, pen_coef=65536), _lib.PairParams(ins_max=9, pen_max=65536), _lib.PairParams(ins_max=9, mapq_coef=65536),
              _lib.PairParams(ins_max=9, mapq_max=256), _lib.PairParams(ins_min=10, ins_max=9)):
        rc, rep, got = raw_dev(hits, hidx, alns, 8, params=p)
        assert rc == _lib.KISS_HIP_E_INVALID and (got == -1).all()
    assert raw_dev(hits, hidx, alns, 8, params=_lib.PairParams(ins_min=9, ins_max=9, pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255))[0] == 0
    # aln_count is what bounds the reads of alns: with fewer records than the hits name, those pairs are bad input
    rc, rep, got = raw_dev(hits, hidx, alns, 8, aln_count=len(alns) - 6)
    short = pm.pair(hits, hidx, alns[:-6])
    assert rc == 0 and np.array_equal(got.view(np.uint32).astype(np.int64), short["pairs"]) and rep.bad_input == short["report"]["bad_input"] >= 1
    # no reads
    rc, rep, got = raw_dev([], [0], [], 0)
    assert rc == 0 and (got == -1).all() and rep.P == 0
    res = kiss_amd.pair_hits(np.zeros((0, 8), np.int64), [0], np.zeros((0, 12), np.int64))
    assert res["pairs"].shape == (0,) and res["report"]["P"] == 0
    # reads without hits
    rc, rep, got = raw_dev([], [0, 0, 0, 0, 0], [], 4)
    assert rc == 0 and [list(r) for r in got.view(np.uint32)] == [[pm.NONE, pm.NONE, 0, 0, 0, 0, 0, 0, 0, 0]] * 2


# ---- (c) FMIndex.map_pairs ----------------------------------------------------------------------------------------------------------
def revcomp(R):
    return (3 - np.asarray(R, np.uint8)[::-1]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mates_of(name):
    """the reads of the align tests paired as they come, and, where the text is long enough, fragments cut from it"""
    from tests.test_fm_align_gpu import reads_of
    S = text(name)
    reads = list(reads_of(name))
    reads = reads[:len(reads) & ~1]
    m1, m2 = reads[0::2], reads[1::2]
    rng = np.random.default_rng(33)
    if S.size >= 2000:
        for i in range(6):
            frag = int(rng.integers(250, 600))
            p = int(rng.integers(0, S.size - frag))
            a, b = S[p:p + 100].copy(), revcomp(S[p + frag - 100:p + frag])
            a[50] = (a[50] + 1) & 3
            m1.append(b if i % 2 else a)
            m2.append(a if i % 2 else b)
    return m1, m2


PAIR_SETS = (dict(), dict(ins_min=200, ins_max=500, ins_mean=300, pen_coef=64, pen_max=30, mapq_coef=200, mapq_max=100))


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_pairs_of_reads_equal_the_model_on_the_hits_of_the_device(name):
    from tests.test_fm_chain_gpu import index_of
    f = index_of(name, 4)
    S = text(name)
    m1, m2 = mates_of(name)
    for params in PAIR_SETS:
        res = f.map_pairs(m1, m2, S, 15, 0, 200, chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), **params)
        want = pm.pair(res["hits"], res["hit_index"], res["alignments"], **params)
        check(res, want, key="pair_report")
        assert res["pair_report"]["P"] == len(m1) and res["hit_index"].size == 2 * len(m1) + 1 and "select_report" in res and "cigar" in res
    if name in ("genome", "iid"):
        assert res["pair_report"]["proper"] >= 3
    with pytest.raises(ValueError):
        f.map_pairs(m1, m2[:-1] if m2 else [np.zeros(5, np.uint8)], S)
    with pytest.raises(TypeError):
        f.map_pairs(m1, m2, S, overlap=3)


TRUTH_SEED = 17


@functools.lru_cache(maxsize=None)
def pair_truth_case():
    """a random text of 20 000 bases that holds a 500-base block twice, 10 000 bases apart; 20 pairs of 150-base mates with
    three substitutions each (not in the outer 20 bases, where an end would rather be clipped), fragments of 350..450 bases.
    Mate 1 lies wholly inside the block, its true copy alternating between the two in twos; mate 2 lies wholly in the unique
    flank: to the right and reverse-complemented for even pairs, to the left and forward (mate 1 reverse-complemented) for odd
    pairs -> text, mates 1, mates 2, [(true start of mate 1, true start of mate 2, fragment length)]"""
    rng = np.random.default_rng(TRUTH_SEED)
    S = rng.integers(0, 4, 20000, dtype=np.uint8)
    S[12000:12500] = S[2000:2500]

    def cut(p):
        R = S[p:p + 150].copy()
        for j in rng.choice(np.arange(20, 130), 3, replace=False):
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        return R

    m1, m2, truth = [], [], []
    for p in range(20):
        B = 12000 if (p // 2) % 2 else 2000
        frag = int(rng.integers(350, 451))
        if p % 2 == 0:
            a = int(rng.integers(B + 650 - frag, B + 351))  # mate 1 [a, a + 150) in the block, mate 2 [a + frag - 150, a + frag) behind it
            b = a + frag - 150
            assert B <= a and a + 150 <= B + 500 and b >= B + 500
            m1.append(cut(a))
            m2.append(revcomp(cut(b)))
        else:
            e = int(rng.integers(B + 150, B + frag - 149))  # mate 1 [e - 150, e) in the block, mate 2 [e - frag, e - frag + 150) in front of it
            a, b = e - 150, e - frag
            assert B <= a and e <= B + 500 and b + 150 <= B
            m1.append(revcomp(cut(a)))
            m2.append(cut(b))
        truth.append((a, b, frag))
    return S, m1, m2, truth


def assert_truth(res, truth, tbeg_of):
    """the conditions of the issue, for EVERY pair; res: pairs (rows of PAIR_FIELDS), hits (rows of HIT_FIELDS), hit_index"""
    pairs, hits, hidx = res
    promoted = lifted = 0
    for p, (a, b, frag) in enumerate(truth):
        r = dict(zip(pm.PAIR_FIELDS, (int(v) for v in pairs[p])))
        assert r["flags"] & pm.PROPER and r["n_conc"] == 1, (p, r)
        h1, h2 = hits[r["hit1"]], hits[r["hit2"]]
        assert abs(tbeg_of(h1) - a) <= 32, (p, tbeg_of(h1), a)
        assert r["mapq1"] == 60 and int(hits[int(hidx[2 * p])][2]) == 0, (p, r)   # (select alone: MAPQ 0)
        assert tbeg_of(h2) == b and r["mapq2"] == 60, (p, tbeg_of(h2), b, r)
        assert abs(r["tlen"] - frag) <= 64, (p, r, frag)
        promoted += bool(r["flags"] & pm.PROMOTED1) + bool(r["flags"] & pm.PROMOTED2)
        lifted += (r["mapq1"] > int(h1[2])) + (r["mapq2"] > int(h2[2]))
    assert promoted == 10 and lifted == 20


def test_against_the_truth_a_mate_in_a_repeat_is_anchored_by_its_partner():
    """Every pair: proper, one concordant combination, mate 1 at its true copy with MAPQ 60 although select alone gives it 0,
    mate 2 at its true start with MAPQ 60, TLEN within 64 of the fragment; over the batch 10 mates promoted from select's
    secondary and 20 lifted.  The conditions hold on this seed in the five CPU models composed:
    tests/test_fm_pair_truth_model.py."""
    import kiss_amd
    import kiss_amd.fm_index as fm
    S, m1, m2, truth = pair_truth_case()
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    res = f.map_pairs(m1, m2, S)
    f.close()
    want = pm.pair(res["hits"], res["hit_index"], res["alignments"])
    check(res, want, key="pair_report")
    hits = [tuple(int(h[k]) for k in pm.HIT_FIELDS) for h in res["hits"]]
    assert_truth((want["pairs"], hits, res["hit_index"]), truth, lambda h: int(res["alignments"]["tbeg"][h[0]]))
    assert res["pair_report"]["promoted"] == 10 and res["pair_report"]["lifted"] == 20 and res["pair_report"]["proper"] == 20
