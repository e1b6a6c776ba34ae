"""tests/fm_pair_model.py held against properties that do not mention its bookkeeping, on small inputs: the four conditions of
a concordant combination over every pair of intervals, the symmetry between the mates, hits that pair with nothing, the
penalty and the insert limits worked by hand, and random batches through an independent second statement.  No GPU."""
import itertools

import numpy as np

from tests import fm_pair_model as pm

F = dict(zip(pm.PAIR_FIELDS, range(10)))


def one(h1, h2, **params):
    hits, hidx, alns = pm.batch_of([(h1, h2)])
    res = pm.pair(hits, hidx, alns, **params)
    return dict(zip(pm.PAIR_FIELDS, (int(v) for v in res["pairs"][0]))), res["report"]


def test_every_pair_of_intervals_on_one_coordinate_for_both_strand_assignments():
    ivs = [(a, b) for a in range(7) for b in range(a + 1, 8)]
    seen = {True: 0, False: 0}
    for (a0, a1), (b0, b1) in itertools.product(ivs, ivs):
        for rev1, rev2 in itertools.product((0, 1), (0, 1)):
            rec, rep = one([(a0, a1, rev1, 50)], [(b0, b1, rev2, 40)], ins_min=2, ins_max=5, ins_mean=3, pen_coef=0)
            # the four conditions, spelt out on the numbers
            if rev1 == rev2:
                want = False
            else:
                (f0, f1), (r0, r1) = ((b0, b1), (a0, a1)) if rev1 else ((a0, a1), (b0, b1))
                want = f0 <= r0 and f1 <= r1 and 2 <= r1 - f0 <= 5
            assert bool(rec["flags"] & pm.PROPER) == want, ((a0, a1, rev1), (b0, b1, rev2))
            assert rec["n_conc"] == (1 if want else 0) and rep["concordant"] == rec["n_conc"] and rep["combinations"] == 1
            if want:
                assert rec["tlen"] == r1 - f0 and rec["score"] == 90 and rec["mapq1"] == rec["mapq2"] == 60
            else:
                assert rec["tlen"] == max(a1, b1) - min(a0, b0) and rec["score"] == 90 and rec["mapq1"] == rec["mapq2"] == 0
            seen[want] += 1
    assert seen[True] > 100 and seen[False] > 1000
    # another record: never
    rec, _ = one([(0, 3, 0, 50, 0)], [(2, 5, 1, 40, 1)], ins_min=0, ins_max=9)
    assert rec["flags"] == pm.MATE1_MAPPED | pm.MATE2_MAPPED and rec["tlen"] == 0


def random_mate(rng, n, span=3000):
    out = []
    for i in range(n):
        tb = int(rng.integers(0, span))
        head = 0 if i == 0 or rng.random() < 0.8 else int(rng.integers(1, i + 1))
        out.append((tb, tb + int(rng.integers(-2, 160)), int(rng.integers(0, 2)), int(rng.integers(30, 151)), int(rng.integers(0, 2)), head,
                    int(rng.integers(0, 61)) if i == 0 else 0))
    return out


def random_batch(rng, pairs=6, most=7):
    return [(random_mate(rng, int(rng.integers(0, most))), random_mate(rng, int(rng.integers(0, most)))) for _ in range(pairs)]


def test_swapping_the_mates_swaps_the_mate_fields_and_nothing_else():
    rng = np.random.default_rng(2)
    checked = 0
    for _ in range(300):
        batch = random_batch(rng)
        a = pm.pair(*pm.batch_of(batch))
        hits_b, hidx_b, alns_b = pm.batch_of([(m2, m1) for m1, m2 in batch])
        b = pm.pair(hits_b, hidx_b, alns_b)
        for p, (ra, rb) in enumerate(zip(a["pairs"], b["pairs"])):
            for k in ("score", "tlen", "n_conc"):
                assert ra[F[k]] == rb[F[k]], (k, batch[p])
            if not ra[F["flags"]] & pm.PROPER:
                continue
            # ties in S go to the smallest x first: the swapped pair may break them the other way
            m1, m2 = batch[p]
            hits, hidx, alns = pm.batch_of([(m1, m2)])
            sole = pm.pair(hits, hidx, alns)["pairs"][0]
            assert list(sole[2:]) == list(ra[2:])
            S = int(ra[F["score"]])
            ties = 0
            for x, hx in enumerate(m1):
                for y, hy in enumerate(m2):
                    if hx[5] == 0 and hy[5] == 0 and hx[0] < hx[1] and hy[0] < hy[1]:
                        T = pm.concordant((hx[0], hx[1], hx[4], hx[2]), (hy[0], hy[1], hy[4], hy[2]), pm.DEFAULTS)
                        if T is not None and pm.pair_score(hx[3], hy[3], T, pm.DEFAULTS) == S:
                            ties += 1
            if ties != 1:
                continue
            checked += 1
            base = sum(len(m[0]) + len(m[1]) for m in batch[:p])  # (the same in both batches)
            x, y = int(ra[F["hit1"]]) - base, int(ra[F["hit2"]]) - base - len(m1)
            assert int(rb[F["hit1"]]) == base + y and int(rb[F["hit2"]]) == base + len(m2) + x
            assert (ra[F["sub1"]], ra[F["sub2"]], ra[F["mapq1"]], ra[F["mapq2"]]) == (rb[F["sub2"]], rb[F["sub1"]], rb[F["mapq2"]], rb[F["mapq1"]])
            fa, fb = int(ra[F["flags"]]), int(rb[F["flags"]])
            assert bool(fa & pm.PROMOTED1) == bool(fb & pm.PROMOTED2) and bool(fa & pm.PROMOTED2) == bool(fb & pm.PROMOTED1)
        for k in ("eligible", "combinations", "concordant", "proper", "max_combinations"):
            assert a["report"][k] == b["report"][k]
    assert checked > 100


def test_a_hit_that_is_concordant_with_nothing_changes_only_the_counts():
    rng = np.random.default_rng(4)
    proper = 0
    for _ in range(200):
        m1, m2 = random_mate(rng, int(rng.integers(1, 6))), random_mate(rng, int(rng.integers(1, 6)))
        before, rep0 = one(m1, m2)
        lone = (1 << 20, (1 << 20) + 100, int(rng.integers(0, 2)), 150, 0, 0)  # far from everything, behind the other hits
        after, rep1 = one(m1 + [lone], m2)
        assert before["hit1"] == after["hit1"] and before["hit2"] + 1 == after["hit2"]  # (mate 2's segment starts one later)
        assert [before[k] for k in pm.PAIR_FIELDS[2:]] == [after[k] for k in pm.PAIR_FIELDS[2:]]
        assert rep1["eligible"] == rep0["eligible"] + 1 and rep1["concordant"] == rep0["concordant"] and rep1["proper"] == rep0["proper"]
        assert rep1["combinations"] >= rep0["combinations"] and (rep1["promoted"], rep1["lifted"]) == (rep0["promoted"], rep0["lifted"])
        proper += rep0["proper"]
        # a supplementary head, or one of its secondaries, in the middle of everything: not even counted
        extra = (m2[0][0], m2[0][1], 1 - m1[0][2], 150, m1[0][4], len(m1))
        sup, rep2 = one(m1 + [extra], m2)
        assert [sup[k] for k in pm.PAIR_FIELDS[2:]] == [before[k] for k in pm.PAIR_FIELDS[2:]] and rep2["eligible"] == rep0["eligible"]
    assert proper > 20


def test_the_penalty_by_hand():
    # forward mate at [1000, 1100), reverse mate ends at 1000 + T; scores 100 + 100; pen_coef 8 / 256 = one point per 32 bases
    def S(T, **kw):
        rec, _ = one([(1000, 1100, 0, 100)], [(1000 + T - 100, 1000 + T, 1, 100)], **kw)
        assert rec["flags"] & pm.PROPER and rec["tlen"] == T
        return rec["score"]
    assert S(400) == 200          # |T - mean| = 0
    assert S(431) == 200 and S(369) == 200   # 31 * 8 / 256 = 0
    assert S(432) == 199 and S(368) == 199   # 32 * 8 / 256 = 1
    assert S(1000) == 200 - 18               # 600 * 8 / 256 = 18.75
    assert S(1039, ins_max=2000) == 200 - 19 and S(1040, ins_max=2000) == 200 - 20 and S(2000, ins_max=2000) == 200 - 20  # pen_max = 20
    assert S(1000, pen_max=5) == 195 and S(1000, pen_coef=0) == 200
    assert S(1000, pen_coef=65535, pen_max=65535) == 1      # max(1, ...)
    assert S(150, ins_mean=0, pen_coef=256, pen_max=65535) == 50


def test_the_insert_limits_are_inclusive():
    def proper(T, **kw):
        rec, _ = one([(1000, 1050, 0, 100)], [(1000 + T - 50, 1000 + T, 1, 100)], **kw)
        return bool(rec["flags"] & pm.PROPER)
    assert proper(300, ins_min=300, ins_max=500) and not proper(299, ins_min=300, ins_max=500)
    assert proper(500, ins_min=300, ins_max=500) and not proper(501, ins_min=300, ins_max=500)
    assert proper(400, ins_min=400, ins_max=400) and not proper(399, ins_min=400, ins_max=400) and not proper(401, ins_min=400, ins_max=400)
    assert proper(1000) and not proper(1001) and proper(50)   # the defaults: 0 .. 1000; T = 50: the mates on top of each other


def test_mapq_promotion_and_the_subs_by_hand():
    # mate 1 in a repeat: select's primary (hit 0) at the wrong copy, its secondary at the right one; mate 2 unique
    rec, rep = one([(5000, 5150, 0, 140, 0, 0, 0), (1000, 1150, 0, 140, 0, 0, 0)], [(1250, 1400, 1, 145, 0, 0, 60)])
    assert rec["flags"] == pm.PROPER | pm.MATE1_MAPPED | pm.MATE2_MAPPED | pm.SAME_REF | pm.PROMOTED1
    assert (rec["hit1"], rec["hit2"], rec["tlen"], rec["score"], rec["sub1"], rec["sub2"], rec["n_conc"]) == (1, 2, 400, 285, 0, 0, 1)
    assert rec["mapq1"] == 60 and rec["mapq2"] == 60 and (rep["promoted"], rep["lifted"]) == (1, 1)
    # both copies have a partner: sub1 is the other copy's pair, mate 2's other hit gives sub2
    rec, _ = one([(1000, 1150, 0, 140), (5000, 5150, 0, 140)], [(1250, 1400, 1, 145, 0, 0, 60), (5314, 5464, 1, 100)])
    assert (rec["score"], rec["sub1"], rec["sub2"], rec["n_conc"]) == (285, 238, 238, 2)
    assert rec["mapq1"] == 120 * (285 - 238) // 285 and rec["mapq2"] == 60  # (mate 2 keeps its own 60)
    # a tie in S: the smallest x, then the smallest y
    rec, _ = one([(1000, 1150, 0, 140), (1000, 1150, 0, 140, 0, 0)], [(1250, 1400, 1, 145), (1250, 1400, 1, 145)])
    assert (rec["hit1"], rec["hit2"], rec["sub1"], rec["sub2"], rec["mapq1"], rec["n_conc"]) == (0, 2, 285, 285, 0, 4)
    # nothing on one side
    rec, _ = one([], [(1250, 1400, 1, 145, 3, 0, 17)])
    assert (rec["hit1"], rec["hit2"], rec["flags"], rec["score"], rec["mapq1"], rec["mapq2"]) == (pm.NONE, 0, pm.MATE2_MAPPED, 145, 0, 17)
    rec, _ = one([], [])
    assert (rec["hit1"], rec["hit2"], rec["flags"], rec["score"]) == (pm.NONE, pm.NONE, 0, 0)
    # an aln that points nowhere, a score select never writes
    hits, hidx, alns = pm.batch_of([([(0, 100, 0, 50)], [(200, 300, 1, 50)]), ([(0, 100, 0, 50)], [(200, 300, 1, 50)])])
    hits[1] = (99,) + hits[1][1:]
    res = pm.pair(hits, hidx, alns)
    assert list(res["pairs"][0]) == [0, 0, pm.BAD_INPUT, 0, 0, 0, 0, 0, 0, 0] and res["pairs"][1][F["flags"]] & pm.PROPER
    assert res["report"]["bad_input"] == 1 and res["report"]["proper"] == 1 and res["report"]["eligible"] == 2


def test_500_random_batches_through_the_windowed_statement():
    rng = np.random.default_rng(9)
    proper = 0
    for i in range(500):
        kw = (dict(), dict(ins_min=100, ins_max=700, ins_mean=300), dict(pen_coef=0), dict(ins_min=250, ins_max=250, pen_coef=64, pen_max=9),
              dict(mapq_coef=65535, mapq_max=255, pen_coef=300, pen_max=40))[i % 5]
        batch = random_batch(rng, pairs=5, most=9)
        hits, hidx, alns = pm.batch_of(batch, first_aln=i % 3)
        a = pm.pair(hits, hidx, alns, **kw)
        b = pm.pair_windowed(hits, hidx, alns, **kw)
        assert np.array_equal(a["pairs"], b), (i, a["pairs"], b)
        proper += a["report"]["proper"]
    assert proper > 300
