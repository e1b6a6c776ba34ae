"""tests/fm_select_model.py held against properties of the definition that do not mention the walk's bookkeeping: small inputs
on the grid 0..6 -- exhaustive over one coordinate for two and for three candidates, thinned for four --, random ones and
hand-worked cases.  No GPU needed."""
import itertools
import random

import pytest

from tests import fm_select_model as sm

L = 6  # read length of the small inputs: coordinates on the grid 0..6


def _intervals():
    return [(a, b) for a in range(L + 1) for b in range(a + 1, L + 1)]


def _check_properties(rows, cidx, lens, both, share, **kw):
    res = sm.select(rows, cidx, lens, both_strands=both, overlap=share, min_score=1, mapq_coef=120, mapq_max=60, **kw)
    hits, hidx, rep = res["hits"], res["hit_index"], res["report"]
    Q = len(lens)
    V = 2 * Q if both else Q
    assert len(hidx) == Q + 1 and hidx[0] == 0 and hidx[-1] == len(hits) == rep["hits"]
    n_red = 0
    for q in range(Q):
        Lq = lens[q]
        mine = hits[hidx[q]:hidx[q + 1]]
        lo, hi = cidx[2 * q if both else q] - cidx[0], cidx[2 * q + 2 if both else q + 1] - cidx[0]
        mid = cidx[2 * q + 1] - cidx[0] if both else hi

        def geom(a):
            score, flags, rb, re, tb, te = rows[a][:6]
            rev = a >= mid
            return dict(a=a, score=score, rev=rev, t=(tb, te), r=(Lq - re, Lq - rb) if rev else (rb, re))

        kept = [geom(int(h[0])) for h in mine]
        kept_ids = [k["a"] for k in kept]
        assert len(set(kept_ids)) == len(kept_ids) and all(lo <= a < hi for a in kept_ids)
        for h, k in zip(mine, kept):
            assert int(h[3]) == k["score"] and bool(h[1] & sm.HIT_REVERSE) == k["rev"]
        # hits are in non-increasing score
        assert all(kept[i]["score"] >= kept[i + 1]["score"] for i in range(len(kept) - 1))
        # no two kept hits of one strand overlap in the text by more than the share
        for x, y in itertools.combinations(kept, 2):
            assert not (x["rev"] == y["rev"] and sm.overlaps(*x["t"], *y["t"], share))
        # every dropped candidate overlaps a kept one that comes before it in the order
        for a in range(lo, hi):
            if a in kept_ids or rows[a][1] != 0 or rows[a][0] < 1:
                continue
            n_red += 1
            d = geom(a)
            assert any(k["rev"] == d["rev"] and sm.overlaps(*d["t"], *k["t"], share) and
                       (k["score"], -k["a"]) > (d["score"], -d["a"]) for k in kept), (rows, a)
        heads = [(i, k) for i, (h, k) in enumerate(zip(mine, kept)) if not h[1] & sm.HIT_SECONDARY]
        # heads pairwise do not overlap in the read by more than the share; the first is the primary, the rest supplementary
        for (i, x), (j, y) in itertools.combinations(heads, 2):
            assert not sm.overlaps(*x["r"], *y["r"], share)
        for n, (i, k) in enumerate(heads):
            assert bool(mine[i][1] & sm.HIT_SUPPLEMENTARY) == (n > 0) and int(mine[i][6]) == i
        if kept:
            assert heads and heads[0][0] == 0
        # every secondary overlaps its head, and no earlier head
        for i, (h, k) in enumerate(zip(mine, kept)):
            if not h[1] & sm.HIT_SECONDARY:
                continue
            g = int(h[6])
            assert g < i and not mine[g][1] & sm.HIT_SECONDARY and not h[1] & sm.HIT_SUPPLEMENTARY
            assert sm.overlaps(*k["r"], *kept[g]["r"], share)
            assert not any(j < g and sm.overlaps(*k["r"], *y["r"], share) for j, y in heads)
            assert int(h[2]) == 0 and int(h[4]) == 0 and int(h[5]) == 0
        # sub is the maximum over the head's secondaries, n_sec their count
        for i, k in heads:
            secs = [kept[j]["score"] for j in range(len(kept)) if mine[j][1] & sm.HIT_SECONDARY and int(mine[j][6]) == i]
            assert int(mine[i][5]) == len(secs) and int(mine[i][4]) == (max(secs) if secs else 0)
            assert int(mine[i][2]) == min(60, 120 * (k["score"] - int(mine[i][4])) // k["score"])
    assert n_red == rep["redundant"]
    return res


def _rows(cands):
    """(score, rbeg, rend, tbeg, tend) -> 12-field records"""
    return [(s, 0, rb, re, tb, te, 0, 0, 0, 0, 0, 1) for (s, rb, re, tb, te) in cands]


# how two read intervals (or two text intervals) of the grid can lie: the same, apart, partly shared, one inside the other
FIXED_PAIRS = (((0, 4), (0, 4)), ((0, 2), (3, 6)), ((0, 4), (2, 6)), ((1, 3), (0, 6)))
STRANDS_2 = ((False, [0, 2]), (True, [0, 1, 2]), (True, [0, 2, 2]), (True, [0, 0, 2]))


def test_every_pair_of_text_intervals_and_every_pair_of_read_intervals():
    """two candidates, exhaustive over one coordinate at a time: all 21 x 21 pairs of text intervals of the grid 0..6 (then all
    pairs of read intervals) under four fixed lies of the other coordinate, the three score orders, the four ways the two
    records can be split between the strands, and the shares 0, 128 and 256"""
    iv = _intervals()
    assert len(iv) == 21
    count = 0
    for share in (0, 128, 256):
        for x0, x1 in itertools.product(iv, iv):
            for f0, f1 in FIXED_PAIRS:
                for s0, s1 in ((1, 1), (1, 2), (2, 1)):
                    text_full = _rows([(s0, *f0, *x0), (s1, *f1, *x1)])
                    read_full = _rows([(s0, *x0, *f0), (s1, *x1, *f1)])
                    for both, cidx in STRANDS_2:
                        _check_properties(text_full, cidx, [L], both, share)
                        _check_properties(read_full, cidx, [L], both, share)
                        count += 2
    assert count == 2 * 3 * 441 * 4 * 3 * 4


@pytest.mark.parametrize("coordinate", ("text", "read"))
def test_every_triple_of_intervals_over_one_coordinate(coordinate):
    """three candidates, all 21^3 triples of intervals of the grid in one coordinate, the other coordinate the same for all
    three (text: every kept one competes for the read; read: apart in the text, so all are kept and the heads decide); the
    scores cycle through all eight patterns of {1, 2}, the split between the strands through all ten, the share through three"""
    iv = _intervals()
    splits = [(False, [0, 3])] + [(True, [0, a, 3]) for a in range(4)]
    patterns = list(itertools.product((1, 2), repeat=3))
    count = 0
    for n, (x0, x1, x2) in enumerate(itertools.product(iv, repeat=3)):
        sc = patterns[n % 8]
        both, cidx = splits[(n // 8) % len(splits)]
        share = (0, 128, 255)[(n // 40) % 3]
        if coordinate == "text":
            rows = _rows([(sc[0], 0, 4, *x0), (sc[1], 0, 4, *x1), (sc[2], 0, 4, *x2)])
        else:
            rows = _rows([(sc[0], *x0, 0, 5), (sc[1], *x1, 10, 15), (sc[2], *x2, 20, 25)])
        _check_properties(rows, cidx, [L], both, share)
        count += 1
    assert count == 21 ** 3


def test_small_inputs_up_to_four_candidates():
    """up to 4 candidates: all interval choices from a THINNED grid in one coordinate (21^4 x 2 coordinates is out of reach),
    the other coordinate, the scores in {1, 2}, the split between the strands and the share drawn at random"""
    rnd = random.Random(5)
    iv = _intervals()
    thin = iv[::5]
    for n in (1, 2, 3, 4):
        for combo in itertools.product(thin, repeat=n):
            scores = [rnd.choice((1, 2)) for _ in range(n)]
            rows = _rows([(scores[i], *rnd.choice(iv), *combo[i]) for i in range(n)])
            rows2 = _rows([(scores[i], *combo[i], *rnd.choice(thin)) for i in range(n)])
            split = rnd.randrange(n + 1)
            for rws in (rows, rows2):
                _check_properties(rws, [0, n], [L], False, rnd.choice((0, 64, 128, 255)))
                _check_properties(rws, [0, split, n], [L], True, rnd.choice((0, 64, 128, 255)))


def test_random_batches():
    rnd = random.Random(11)
    for trial in range(500):
        both = trial % 2 == 1
        Q = rnd.randrange(1, 4)
        lens = [rnd.randrange(4, 40) for _ in range(Q)]
        V = 2 * Q if both else Q
        c0 = rnd.choice((0, 3))
        cidx = [c0]
        rows = []
        for v in range(V):
            Lq = lens[v // 2 if both else v]
            k = rnd.randrange(0, 7)
            for _ in range(k):
                rb = rnd.randrange(Lq)
                re = rnd.randrange(rb + 1, Lq + 1)
                tb = rnd.randrange(60)
                rows.append((rnd.choice((0, 1, 2, 3, 9)), rnd.choice((0, 0, 0, 1)), rb, re, tb, tb + rnd.randrange(1, 30), 0, 0, 0, 0, 0, 1))
            cidx.append(cidx[-1] + k)
        share = rnd.choice((0, 1, 100, 128, 255, 256))
        res = _check_properties(rows, cidx, lens, both, share)
        assert res["report"]["candidates"] == sum(1 for r in rows if r[1] == 0 and r[0] >= 1)
        capped = sm.select(rows, cidx, lens, both_strands=both, overlap=share, min_score=1, max_hits=2)
        for q in range(Q):  # the cap cuts the list and changes nothing in what stays
            a, b = res["hit_index"][q], res["hit_index"][q + 1]
            ca, cb = capped["hit_index"][q], capped["hit_index"][q + 1]
            assert cb - ca == min(2, b - a) and (capped["hits"][ca:cb] == res["hits"][a:a + (cb - ca)]).all()


def test_order_dependence_only_kept_hits_make_others_redundant():
    """A > B > C; B is redundant to A, C overlaps only B in the text: C is kept"""
    rows = _rows([(30, 0, 10, 100, 120), (20, 0, 10, 115, 135), (10, 0, 10, 128, 148)])
    # A-B share 5 of 20 (> 0 with overlap 0), B-C share 7, A-C share nothing
    res = sm.select(rows, [0, 3], [50], overlap=0, min_score=1)
    assert [int(h[0]) for h in res["hits"]] == [0, 2] and res["report"]["redundant"] == 1
    assert [int(h[1]) for h in res["hits"]] == [0, sm.HIT_SECONDARY]  # (C shares its read interval with A)
    assert int(res["hits"][0][4]) == 10 and int(res["hits"][0][5]) == 1


def test_reverse_frame():
    """L = 150: forward [0, 50) and reverse virtual [0, 50) (original [100, 150)) are two heads; reverse virtual [100, 150)
    (original [0, 50)) is a secondary of the forward one"""
    rows = _rows([(50, 0, 50, 1000, 1050), (40, 0, 50, 5000, 5050), (30, 100, 150, 9000, 9050)])
    res = sm.select(rows, [0, 1, 3], [150], both_strands=True, min_score=1)
    flags = [int(h[1]) for h in res["hits"]]
    assert flags == [0, sm.HIT_REVERSE | sm.HIT_SUPPLEMENTARY, sm.HIT_REVERSE | sm.HIT_SECONDARY]
    assert [int(h[6]) for h in res["hits"]] == [0, 1, 0]
    assert res["report"]["heads"] == 2


def test_mapq_formula():
    assert sm.mapq_of(100, 0, 120, 60) == 60
    assert sm.mapq_of(100, 0, 50, 60) == 50
    assert sm.mapq_of(100, 100, 120, 60) == 0
    assert sm.mapq_of(100, 75, 120, 60) == 30
    big = (1 << 30) - 1
    assert sm.mapq_of(big, 0, 65535, 255) == 255
    assert sm.mapq_of(big, big - 1, 65535, 255) == 0
    assert sm.mapq_of(big, big // 2, 65535, 65535) == (65535 * (big - big // 2)) // big == 32767
    rows = _rows([(big, 0, 10, 0, 10), (big // 2, 0, 10, 50, 60), (big, 20, 30, 100, 110), (big, 20, 30, 200, 210)])
    res = sm.select(rows, [0, 4], [40], mapq_coef=65535, mapq_max=255)
    by_aln = {int(h[0]): h for h in res["hits"]}
    assert int(by_aln[0][2]) == 255 and int(by_aln[0][4]) == big // 2
    assert int(by_aln[2][2]) == 0 and int(by_aln[2][4]) == big and int(by_aln[3][1]) == sm.HIT_SECONDARY


def test_bounds_and_spanning():
    b = [0, 100, 250]
    assert sm.record_of(b, 0, 100) == (0, False)
    assert sm.record_of(b, 0, 101) == (0, True)
    assert sm.record_of(b, 100, 250) == (1, False)
    assert sm.record_of(b, 99, 100) == (0, False)
    assert sm.record_of(b, 250, 251) == (0, True)
    rows = _rows([(40, 0, 10, 95, 105), (35, 0, 10, 100, 110)])
    res = sm.select(rows, [0, 2], [10], bounds=b)
    assert res["report"]["spanning"] == 1 and [int(h[0]) for h in res["hits"]] == [1] and int(res["hits"][0][7]) == 1


@pytest.mark.parametrize("share,ov,kept", ((128, 5, True), (128, 6, False), (0, 0, True), (0, 1, False), (256, 10, True),
                                           (255, 9, True), (255, 10, False), (1, 0, True), (1, 1, False)))
def test_overlap_threshold(share, ov, kept):
    """two intervals of 10: ov * 256 > share * 10 decides"""
    assert sm.overlaps(0, 10, 10 - ov, 20 - ov, share) == (not kept)
