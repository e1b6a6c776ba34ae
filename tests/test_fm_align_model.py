"""tests/fm_align_model.py against (a) the enumeration of every M / I / D lattice path inside the band, (b) itself: the ops
re-scored give the score, the lengths add up, and the row form equals the cell form, (c) pins derived by hand.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import fm_align_model as am

PARAM_SETS = (dict(match=1, mismatch=4, gap_open=6, gap_extend=1), dict(match=2, mismatch=3, gap_open=0, gap_extend=1),
              dict(match=1, mismatch=1, gap_open=1, gap_extend=0), dict(match=3, mismatch=0, gap_open=0, gap_extend=0))
# (d0, d1, band)
GEOMETRIES = ((0, 0, 0), (0, 1, 1), (-1, -1, 2), (2, 0, 0))


def chain_of(d0, d1, at=10):
    """(rbeg, rend, tbeg, tend) with these two diagonals (nothing else of a chain is used)"""
    return at, at, at + d0, at + d1


def paths(L, n, dlo, dhi):
    """every lattice path of M / I / D steps with all points on diagonals dlo..dhi inside [0, L] x [0, n], the empty ones
    left out: (the cells its M steps compare, [gap lengths])"""
    out = []

    def inside(i, j):
        return 0 <= i <= L and 0 <= j <= n and dlo <= j - i <= dhi

    def grow(i, j, cells, gaps, last):
        if cells or gaps:
            out.append((tuple(cells), tuple(gaps)))
        if inside(i + 1, j + 1):
            grow(i + 1, j + 1, cells + [(i, j)], gaps, 0)
        for op, (di, dj) in ((1, (1, 0)), (2, (0, 1))):
            if inside(i + di, j + dj):
                grow(i + di, j + dj, cells, gaps[:-1] + [gaps[-1] + 1] if last == op else gaps + [1], op)

    for i in range(L + 1):
        for j in range(n + 1):
            if inside(i, j):
                grow(i, j, [], [], 0)
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_best_score_equals_the_best_lattice_path(geometry):
    d0, d1, band = geometry
    dlo, dhi, _ = am.band_of(*chain_of(d0, d1), band)
    for L in range(1, 5):
        for n in range(1, 6):
            reads = np.array(list(itertools.product((0, 1), repeat=L)), np.int64)
            texts = np.array(list(itertools.product((0, 1), repeat=n)), np.int64)
            eq = reads[:, None, :, None] == texts[None, :, None, :]  # [read, text, i, j]
            best = np.zeros((len(PARAM_SETS), reads.shape[0], texts.shape[0]), np.int64)  # (the empty path)
            for cells, gaps in paths(L, n, dlo, dhi):
                same = np.zeros(eq.shape[:2], np.int64)
                for i, j in cells:
                    same += eq[:, :, i, j]
                for k, p in enumerate(PARAM_SETS):
                    cost = sum(p["gap_open"] + g * p["gap_extend"] for g in gaps)
                    np.maximum(best[k], p["match"] * same - p["mismatch"] * (len(cells) - same) - cost, out=best[k])
            for k, p in enumerate(PARAM_SETS):
                for a, R in enumerate(reads):
                    for b, S in enumerate(texts):
                        rec, _ = am.align_plain(S, R, *chain_of(d0, d1), band=band, **p)
                        assert rec["score"] == best[k, a, b], (geometry, p, R, S, rec)


def random_case(rng):
    n, L = int(rng.integers(1, 40)), int(rng.integers(1, 30))
    S = rng.integers(0, 4 if rng.random() < 0.7 else 2, n)
    R = rng.integers(0, 4 if rng.random() < 0.7 else 2, L)
    if rng.random() < 0.6 and n > 3:  # a piece of the text with changes
        p = int(rng.integers(0, n - 2))
        R = S[p:p + L].copy()
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(0, R.size + 1))
            R = np.concatenate([R[:k], rng.integers(0, 4, int(rng.integers(0, 3))), R[k + int(rng.integers(0, 3)):]])
        if R.size == 0:
            R = S[:1].copy()
    R = np.where(rng.random(R.size) < 0.08, 78, R)  # no-bases
    d0, d1 = int(rng.integers(-8, 12)), int(rng.integers(-8, 12))
    return S, R, chain_of(d0, d1), int(rng.integers(0, 6))


def test_ops_rescore_to_the_score_and_the_lengths_add_up():
    rng = np.random.default_rng(5)
    aligned = gapped = 0
    for t in range(400):
        S, R, chain, band = random_case(rng)
        p = PARAM_SETS[t % len(PARAM_SETS)]
        rec, ops = am.align_plain(S, R, *chain, band=band, **p)
        again = am.align_rows(S, R, *chain, band=band, **p)
        assert again == (rec, ops), (S, R, chain, band, p)
        assert rec["band"] == abs((chain[2] - chain[0]) - (chain[3] - chain[1])) + 2 * band + 1
        if rec["score"] == 0:
            assert ops == [] and all(rec[k] == 0 for k in am.FIELDS if k != "band")
            continue
        aligned += 1
        gapped += rec["gaps"] > 0
        sc, i, j = am.rescore(ops, rec, S, R, **p)
        assert (sc, i, j) == (rec["score"], rec["rend"], rec["tend"])
        assert rec["rend"] - rec["rbeg"] == rec["matches"] + rec["mismatches"] + rec["ins"]
        assert rec["tend"] - rec["tbeg"] == rec["matches"] + rec["mismatches"] + rec["del"]
        assert rec["gaps"] == sum(1 for op, _ in ops if op) and all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
        assert rec["mismatches"] >= sum(1 for x in R[rec["rbeg"]:rec["rend"]] if x > 3) - rec["ins"]
    assert aligned > 200 and gapped > 20


@pytest.fixture(scope="module")
def text():
    return np.random.default_rng(11).integers(0, 4, 400)


def test_pin_exact_read_and_one_substitution(text):
    R = text[100:250].copy()
    rec, ops = am.align_rows(text, R, 0, 150, 100, 250)
    assert rec["score"] == 150 and am.cigar_string(ops) == "150M" and (rec["rbeg"], rec["tbeg"], rec["tend"]) == (0, 100, 250)
    assert rec["band"] == 65
    R[75] = (R[75] + 1) & 3
    rec, ops = am.align_rows(text, R, 0, 150, 100, 250)
    assert rec["score"] == 145 and am.cigar_string(ops) == "150M" and (rec["matches"], rec["mismatches"]) == (149, 1)


def test_pin_three_text_bases_missing_from_the_read(text):
    R = np.concatenate([text[100:175], text[178:253]])
    rec, ops = am.align_rows(text, R, 0, 150, 100, 250, band=3)
    assert rec["score"] == 141 and rec["tend"] - rec["tbeg"] == 153 and rec["band"] == 7 and (rec["del"], rec["gaps"]) == (3, 1)
    rec, ops = am.align_rows(text, R, 0, 150, 100, 250, band=2)  # the gap does not fit: one half, the one that ends first
    assert rec["score"] == 75 and rec["rend"] == 75 and rec["band"] == 5
    rec, ops = am.align_rows(text, R, 0, 150, 100, 253, band=0)  # the chain knows about the gap
    assert rec["score"] == 141 and rec["band"] == 4 and (rec["rbeg"], rec["rend"], rec["tbeg"], rec["tend"]) == (0, 150, 100, 253)


def test_pin_the_gap_sits_at_the_left_end_of_a_run():
    rng = np.random.default_rng(3)
    X, Y = rng.integers(1, 4, 20), rng.integers(1, 4, 20)  # (no A next to the run)
    S = np.concatenate([X, np.zeros(8, np.int64), Y])
    R = np.concatenate([X, np.zeros(6, np.int64), Y])
    rec, ops = am.align_rows(S, R, 0, 46, 0, 48)
    assert am.cigar_string(ops) == "20M2D26M" and rec["score"] == 46 - 8
    assert am.align_plain(S, R, 0, 46, 0, 48) == (rec, ops)


def test_pin_reads_that_hang_over_the_ends_of_the_text(text):
    n = text.size
    rng = np.random.default_rng(4)
    R = np.concatenate([(text[:5][::-1] + 1) & 3, text[:145]])  # five bases in front of the text
    rec, ops = am.align_rows(text, R, 5, 150, 0, 145)
    assert (rec["rbeg"], rec["tbeg"], rec["score"]) == (5, 0, 145) and am.cigar_string(ops) == "145M"
    R = np.concatenate([text[n - 143:], rng.integers(0, 4, 7)])  # seven bases behind it
    rec, ops = am.align_rows(text, R, 0, 143, n - 143, n)
    assert (rec["tend"], rec["rend"], rec["score"]) == (n, 143, 143)
