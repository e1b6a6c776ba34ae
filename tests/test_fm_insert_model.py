"""tests/fm_insert_model.py held against statements of the definition that do not share its loops (include/kiss_hip_insert.h):
the quartiles by sorting, the mean and the deviation in big-integer arithmetic, the order of the results, the invariances, the
pair model's concordance rule, and cases worked by hand.  No GPU needed."""
import math

import numpy as np
import pytest

from tests import fm_insert_model as im
from tests import fm_pair_model as pm


def random_pairs(rng, P, centre=None):
    """pairs for pm.batch_of(): most of them face each other around `centre`, the rest is one of everything"""
    centre = int(rng.integers(50, 3000)) if centre is None else centre
    spread = int(rng.integers(0, 200))
    out = []
    for _ in range(P):
        kind = rng.integers(0, 12)
        L1, L2 = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        start = int(rng.integers(0, 100000))
        T = max(1, centre + int(rng.integers(-spread, spread + 1)))
        if kind == 11:
            T = int(rng.integers(1, 12000))
        fwd = (start, start + L1, 0, 50, 0, 0, int(rng.choice([60, 60, 60, 20, 19, 0])))
        rev = (start + T - L2, start + T, 1, 50, 0, 0, int(rng.choice([60, 60, 60, 20, 19, 0])))
        if kind == 0:
            rev = rev[:4] + (1,) + rev[5:]                      # another record
        elif kind == 1:
            rev = rev[:2] + (0,) + rev[3:]                      # the same strand
        elif kind == 2:
            fwd, rev = (rev[0], rev[1], 0) + fwd[3:], (fwd[0], fwd[1], 1) + rev[3:]  # the forward hit behind the reverse one
        elif kind == 3:
            rev = (rev[1], rev[1]) + rev[2:]                    # tbeg == tend
        m1, m2 = ([fwd], [rev]) if rng.integers(0, 2) else ([rev], [fwd])
        if kind == 4:
            m1 = []
        elif kind == 5:
            m2 = []
        elif kind == 6:
            m1 = m1 + [(7, 9, 0, 30, 0, 0, 0)]                  # a second hit says nothing
        out.append((m1, m2))
    return out


def batch(rng, P, **kw):
    hits, hidx, alns = pm.batch_of(random_pairs(rng, P, **kw), first_aln=int(rng.integers(0, 3)))
    if hits and rng.integers(0, 3) == 0:  # a hit that names no alignment
        h = int(rng.integers(0, len(hits)))
        hits[h] = (len(alns) + int(rng.integers(0, 2)) * 0xFFFF0000,) + hits[h][1:]
    return hits, hidx, alns


def random_params(rng):
    return dict(min_mapq=int(rng.choice([0, 20, 21, 60])), max_insert=int(rng.choice([1, 500, 4000, 10000, 65535])),
                min_samples=int(rng.choice([0, 1, 5, 25])), out_mult=int(rng.choice([0, 1, 2, 255])),
                map_mult=int(rng.choice([0, 3, 255])), sd_mult=int(rng.choice([0, 4, 255])))


def samples_of(hits, hidx, alns, p):
    """the samples by the pair model's rule: combination (0, 0) concordant under ins_min = 1, ins_max = max_insert, both MAPQs
    pass -- and, because that rule takes eligible hits for granted, no empty interval and no aln outside alns"""
    out = []
    for q in range(0, len(hidx) - 1, 2):
        h1, h2 = hits[hidx[q]:hidx[q + 1]], hits[hidx[q + 1]:hidx[q + 2]]
        if not h1 or not h2 or not all(0 <= h[0][0] < len(alns) for h in (h1, h2)):
            continue
        view = [(alns[h[0][0]][4], alns[h[0][0]][5], h[0][7], h[0][1] & 1) for h in (h1, h2)]
        if any(v[0] >= v[1] for v in view) or h1[0][2] < p["min_mapq"] or h2[0][2] < p["min_mapq"]:
            continue
        T = pm.concordant(view[0], view[1], dict(ins_min=1, ins_max=p["max_insert"]))
        if T is not None:
            out.append(T)
    return out


@pytest.mark.parametrize("chunk", range(5))
def test_the_model_against_independent_statements_on_500_random_batches(chunk):
    rng = np.random.default_rng(4170 + chunk)
    for _ in range(100):
        P = int(rng.integers(0, 120))
        hits, hidx, alns = batch(rng, P)
        kw = random_params(rng)
        p = im.params_of(**kw)
        got = im.estimate(hits, hidx, alns, **kw)
        rep, hist = got["report"], got["hist"]
        samples = samples_of(hits, hidx, alns, p)
        assert rep["samples"] == len(samples) == int(hist.sum())
        assert np.array_equal(hist, np.bincount(np.array(samples, dtype=np.int64), minlength=p["max_insert"] + 1))
        assert hist[0] == 0 and sum(rep[c] for c in im.CLASSES) == rep["P"] == P
        ok = len(samples) >= max(p["min_samples"], 1)
        assert rep["flags"] == (im.OK if ok else 0)
        if not ok:
            assert all(rep[k] == 0 for k in im.STATS)
            continue
        srt, N = np.sort(np.array(samples, dtype=np.int64)), len(samples)
        q25, q50, q75 = (int(srt[j * N // 4]) for j in (1, 2, 3))
        assert (rep["q25"], rep["q50"], rep["q75"]) == (q25, q50, q75)
        iqr = q75 - q25
        used = [T for T in samples if q25 - p["out_mult"] * iqr <= T <= q75 + p["out_mult"] * iqr]
        assert 1 <= rep["used"] == len(used) <= N
        mean = (sum(used) + len(used) // 2) // len(used)
        sd = math.isqrt(sum((T - mean) ** 2 for T in used) // len(used))
        assert (rep["mean"], rep["sd"], rep["ins_mean"]) == (mean, sd, mean)
        assert rep["ins_min"] == max(0, min(q25 - p["map_mult"] * iqr, mean - p["sd_mult"] * sd))
        assert rep["ins_max"] == max(q75 + p["map_mult"] * iqr, mean + p["sd_mult"] * sd)
        assert rep["ins_min"] <= q25 <= q50 <= q75 <= rep["ins_max"] and rep["ins_min"] <= mean <= rep["ins_max"]
        # the pairs in another order; the mates of every pair swapped
        order = rng.permutation(P)
        prs = [(hits[hidx[2 * k]:hidx[2 * k + 1]], hits[hidx[2 * k + 1]:hidx[2 * k + 2]]) for k in range(P)]
        for swap in (False, True):
            h2, i2 = [], [0]
            for k in order:
                for mate in (prs[k][::-1] if swap else prs[k]):
                    h2 += mate
                    i2.append(len(h2))
            other = im.estimate(h2, i2, alns, **kw)
            assert other["report"] == rep and np.array_equal(other["hist"], hist)


def test_hand_worked_cases():
    one = im.of_lengths([300], min_samples=1)["report"]
    assert one["flags"] == im.OK and [one[k] for k in im.STATS] == [1, 300, 300, 300, 300, 0, 300, 300, 300]
    assert im.of_lengths([300], min_samples=0)["report"]["flags"] == im.OK     # max(min_samples, 1)
    assert im.of_lengths([], min_samples=0)["report"]["flags"] == 0
    few = im.of_lengths([300] * 24)["report"]
    assert few["flags"] == 0 and few["samples"] == 24 and all(few[k] == 0 for k in im.STATS)
    same = im.of_lengths([412] * 25)["report"]
    assert [same[k] for k in im.STATS] == [25, 412, 412, 412, 412, 0, 412, 412, 412]
    # 30 at 200 and 10 at 5000: ranks 10, 20, 30 -> 200, 200, 5000; IQR 4800: with out_mult 2 every sample is used
    bi = im.of_lengths([200] * 30 + [5000] * 10)["report"]
    assert (bi["q25"], bi["q50"], bi["q75"], bi["used"]) == (200, 200, 5000, 40)
    assert bi["mean"] == (30 * 200 + 10 * 5000 + 20) // 40 == 1400
    assert bi["sd"] == math.isqrt((30 * 1200 ** 2 + 10 * 3600 ** 2) // 40) == 2078
    assert bi["ins_min"] == 0 and bi["ins_max"] == max(5000 + 3 * 4800, 1400 + 4 * 2078) == 19400
    # 31 at 200 and 9 at 5000: q75 is 200 too, IQR 0, only the 200s are used
    bi = im.of_lengths([200] * 31 + [5000] * 9)["report"]
    assert [bi[k] for k in im.STATS] == [31, 200, 200, 200, 200, 0, 200, 200, 200]
    # 99 samples 351 .. 449 and one outlier at max_insert: it is not used
    out = im.of_lengths(list(range(351, 450)) + [10000])["report"]
    assert (out["q25"], out["q50"], out["q75"], out["used"], out["mean"]) == (376, 401, 426, 99, 400)
    assert out["sd"] == math.isqrt(sum((T - 400) ** 2 for T in range(351, 450)) // 99) == 28
    assert (out["ins_min"], out["ins_max"]) == (min(376 - 150, 400 - 112), max(426 + 150, 400 + 112)) == (226, 576)


def test_classes_in_the_order_of_the_definition():
    p = im.params_of()
    alns = [(0,) * 4 + (100, 200) + (0,) * 6, (0,) * 4 + (400, 500) + (0,) * 6, (0,) * 4 + (9, 9) + (0,) * 6]
    f, r = (0, 0, 60, 50, 0, 0, 0, 0), (1, 1, 60, 50, 0, 0, 0, 0)
    assert im.classify([f], [r], alns, p) == ("samples", 400) == im.classify([r], [f], alns, p)
    assert im.classify([], [(99,) + r[1:]], alns, p) == ("unmapped", None)                  # unmapped before bad_input
    assert im.classify([(3, 0, 0) + f[3:]], [r], alns, p) == ("bad_input", None)          # bad_input before low_mapq
    assert im.classify([(0, 0, 19) + f[3:]], [(1, 0, 60) + r[3:]], alns, p) == ("low_mapq", None)  # low_mapq before discordant
    assert im.classify([f], [(1, 1, 20) + r[3:]], alns, p) == ("samples", 400)
    assert im.classify([f], [r[:7] + (1,)], alns, p) == ("discordant", None)
    assert im.classify([f], [(2,) + r[1:]], alns, p) == ("discordant", None)              # tbeg == tend
    assert im.classify([(1, 0) + f[2:]], [(0, 1) + r[2:]], alns, p) == ("discordant", None)  # forward behind reverse
    assert im.classify([f], [r], alns, im.params_of(max_insert=399)) == ("too_long", None)
    assert im.classify([f], [r], alns, im.params_of(max_insert=400)) == ("samples", 400)
