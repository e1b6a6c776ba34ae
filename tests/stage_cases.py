"""Texts and windows shared by tests/test_stage_model.py (CPU, model against the oracle) and tests/test_stage_*_gpu.py
(the stage calls against the model).  Every window has a name that says what it is for; claim() asserts that it is."""
import functools

import numpy as np

from tests import gen
from tests import stage_model as sm

TILE, WORD = sm.TILE, sm.WORD
K_EXACT = 0xFFFFFFFF
KS = (32, 256, K_EXACT)
RUN_LO, RUN_HI = 8000, 16500   # the long run of C of the "runs" texts: from inside tile 0, over tile 1, into tile 2
N_RUNS = 5 * TILE + 5
TAIL_RUN = 40                  # the "runs" texts end inside a run of C this long


def _runs(after):
    """iid with equal-base runs across word and tile boundaries; `after` follows the long run of C (G: the run is S-type,
    A: L-type).  An LMS position is planted on each far/near cut n - D (D = 125, 375) and none can sit right behind it."""
    S = gen.iid(N_RUNS, 21).copy()
    S[RUN_LO - 1] = 3
    S[RUN_LO:RUN_HI] = 1
    S[RUN_HI] = after
    S[3 * TILE - 600:3 * TILE] = 2      # a run that ends exactly at a tile boundary
    S[3 * TILE] = 0
    S[4 * TILE + 20:4 * TILE + 70] = 3  # a run across a word boundary, inside one tile
    S[4 * TILE + 70] = 1
    for D in (125, 375):                # T A C around the cut: the A is an LMS position
        S[N_RUNS - D - 1:N_RUNS - D + 2] = (3, 0, 1)
    S[N_RUNS - TAIL_RUN - 1] = 2
    S[N_RUNS - TAIL_RUN:] = 1           # the text ends inside a run
    S.setflags(write=False)
    return S


def _tandem():
    """(TTAGGG) arrays of 4000 and 3000 bases between iid stretches: many ties through D at k = 32 and 256"""
    unit = np.array([3, 3, 0, 2, 2, 2], dtype=np.uint8)
    parts = [gen.iid(9000, 31), np.tile(unit, 4000 // 6 + 1)[:4000], gen.iid(12_000, 32), np.tile(unit, 500), gen.iid(12_003, 33)]
    S = np.concatenate(parts)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def text(name):
    if name == "iid":
        S = gen.iid(3 * TILE + 37, 3)
    elif name == "genome":  # (at this size the 24 end arrays of 3000 bases, 2916 apart, overlap: one TTAGGG array from base 2832 on)
        S = gen.genome_like(70_001, 7)
    elif name == "genome120k":  # the end arrays stand apart; more than RADIX_TILE far LMS positions (only the sort tests use it)
        S = gen.genome_like(120_001, 7)
    elif name == "runs_G":
        return _runs(2)
    elif name == "runs_A":
        return _runs(0)
    elif name == "CA":  # 16 LMS positions in every word, every second base one
        S = np.tile(np.array([1, 0], dtype=np.uint8), TILE + 1)
    elif name == "tandem":
        return _tandem()
    elif name == "deep":  # one (TTAGGG) array: ties deeper than the exact-order rounds of the sort go
        S = np.tile(np.array([3, 3, 0, 2, 2, 2], dtype=np.uint8), 65_541 // 6 + 1)[:65_541]
    elif name == "no_lms":
        S = np.array([0, 0, 1, 1, 2, 2, 3, 3], dtype=np.uint8)
    else:
        assert name in ("n1", "n2", "n33"), name
        S = gen.iid(int(name[1:]), 5)
    S = np.ascontiguousarray(S, dtype=np.uint8).copy()
    S.setflags(write=False)
    return S


BIG_TEXTS = ("iid", "genome", "runs_G", "runs_A", "CA")
TINY_TEXTS = ("n1", "n2", "n33", "no_lms")
SORT_TEXTS = ("iid", "genome", "genome120k", "runs_G", "runs_A", "CA", "tandem")
RADIX_TILE = 16_384  # items of a radix tile (radix.hip: RX_TILE): the sort reuses the digit counts of the classification's emit
                     # pass only for a list of two tiles or more, 16 385 items (radix.hip: `one`, `counted`)


def ks_of(S):
    return KS + (len(S) - 1, len(S))


def in_run(S, i):
    """is i strictly inside a run of equal bases (the same base on both sides)?"""
    return 0 < i < len(S) - 1 and S[i - 1] == S[i] == S[i + 1]


def tilings(n):
    """an 8-way and a 5-way uneven tiling of [0, n), each with an empty and a one-base window"""
    e8 = [0, 1, 1, 33, min(TILE, n - 2), n // 2 + 7, (3 * n) // 4, n - 1, n]
    e5 = [0, n // 7, n // 7, n // 7 + 1, (2 * n) // 3 + 5, n]
    for e in (e8, e5):
        assert all(a <= b for a, b in zip(e, e[1:])) and any(a == b for a, b in zip(e, e[1:])) and any(b - a == 1 for a, b in zip(e, e[1:]))
    return {"tiling8": list(zip(e8, e8[1:])), "tiling5": list(zip(e5, e5[1:]))}


def windows(name, k):
    """-> {window name: (lo, hi)} of a text of BIG_TEXTS under k (k decides the far cut alone)"""
    S = text(name)
    n = len(S)
    L = sm.lms(S)
    D = sm.depth_of(n, k)
    p = int(L[len(L) // 2])
    j = n // 64 + 3  # a word well inside the text, not a tile boundary
    assert (WORD * j) % TILE and WORD * (j + 3) + 1 < n
    w = {"whole": (0, n), "empty_front": (0, 0), "empty_back": (n, n), "last_base": (n - 1, n),
         "one_lms": (p, p + 1), "base_before_lms": (p - 1, p),
         "inside_one_word": (WORD * j + 5, WORD * j + 20),
         "lms_as_lo": (p, min(n, p + 500)), "lms_as_hi": (max(0, p - 500), p)}
    for e in (-1, 0, 1):
        for f in (-1, 0, 1):
            w["word_edges%+d%+d" % (e, f)] = (WORD * j + e, WORD * (j + 3) + f)
            w["tile_edges%+d%+d" % (e, f)] = (TILE + e, 2 * TILE + f)
    if name.startswith("runs"):
        w["lo_inside_long_run"] = (12_000, RUN_HI + 3000)
        w["hi_inside_long_run"] = (RUN_LO - 1000, 12_001)
        w["both_inside_long_run"] = (RUN_LO + 100, RUN_HI - 100)
        w["hi_at_end_of_run_on_tile_boundary"] = (3 * TILE - 700, 3 * TILE)
        w["lo_at_end_of_run_on_tile_boundary"] = (3 * TILE, 3 * TILE + 700)
        w["tail_run"] = (n - TAIL_RUN + 3, n)
    elif name != "CA":
        i = next(i for i in range(TILE // 2, n - 2) if in_run(S, i))
        w["lo_inside_run"] = (i, i + 300)
        w["hi_inside_run"] = (i - 300, i + 1)
    if 0 < D < n:
        cut = n - D  # the last far position
        w["cut_inside"] = (cut - 1000, n)
        w["behind_cut"] = (cut + 1, n)
        w["hi_at_cut"] = (cut - 1000, cut)
        w["hi_behind_cut"] = (cut - 1000, cut + 1)
        w["lo_at_cut"] = (cut, n)
    return w


def claim(name, k, wname, lo, hi):
    """the window does what its name says (model only)"""
    S = text(name)
    n = len(S)
    L = set(int(x) for x in sm.lms(S))
    keys, pos, m_far = sm.local_list(S, k, lo, hi)
    D = sm.depth_of(n, k)
    if wname == "one_lms":
        assert pos.tolist() == [lo]
    elif wname == "base_before_lms":
        assert hi in L and pos.size == 0
    elif wname == "inside_one_word":
        assert lo // WORD == (hi - 1) // WORD and lo % WORD and hi % WORD
    elif wname == "lms_as_lo":
        assert lo in L and pos[0] == lo
    elif wname == "lms_as_hi":
        assert hi in L and pos.size and pos[-1] < hi
    elif wname in ("lo_inside_long_run", "lo_inside_run"):
        assert in_run(S, lo)
    elif wname in ("hi_inside_long_run", "hi_inside_run"):
        assert in_run(S, hi - 1)
    elif wname == "both_inside_long_run":
        assert in_run(S, lo) and in_run(S, hi - 1) and len(set(S[lo:hi].tolist())) == 1 and pos.size == 0
        assert sm.counts13(S, k, lo, hi)[4:8] == ([0, hi - lo, 0, 0] if name == "runs_G" else [0, 0, 0, 0])  # S-type or L-type
    elif wname == "hi_at_end_of_run_on_tile_boundary":
        assert hi % TILE == 0 and S[hi - 1] == S[hi - 2] != S[hi]
    elif wname == "lo_at_end_of_run_on_tile_boundary":
        assert lo % TILE == 0 and lo in L  # (G ... G A: the A behind the run is an LMS position, first of its tile)
    elif wname == "tail_run":
        assert len(set(S[lo - 2:].tolist())) == 1 and pos.size == 0
    elif wname == "cut_inside":
        assert 0 < m_far < pos.size
    elif wname == "behind_cut":
        assert m_far == 0 and pos.size > 0
    elif wname == "hi_at_cut":
        assert hi == n - D and m_far == pos.size > 0
    elif wname == "hi_behind_cut":
        assert hi == n - D + 1 and m_far == pos.size > 0
        assert name not in ("runs_G", "runs_A") or pos[-1] == n - D  # (planted: the cut itself is a far LMS position)
    elif wname == "lo_at_cut":
        assert name not in ("runs_G", "runs_A") or (pos[0] == n - D and m_far == 1 < pos.size)
    elif wname in ("empty_front", "empty_back"):
        assert lo == hi
    elif wname == "last_base":
        assert hi - lo == 1 and pos.size == 0
    elif wname.startswith("word_edges"):
        e, f = int(wname[-4:-2]), int(wname[-2:])
        assert (lo - e) % WORD == 0 and (hi - f) % WORD == 0 and (lo - e) % TILE and (hi - f) % TILE
    elif wname.startswith("tile_edges"):
        e, f = int(wname[-4:-2]), int(wname[-2:])
        assert (lo - e) % TILE == 0 and (hi - f) % TILE == 0 and hi - lo > TILE - 3
    else:
        assert wname == "whole" and (lo, hi) == (0, n)


def far_cut_texts():
    """tiny texts whose far/near cut n - D (k = 32, D = 125) falls on every field of a packed word in turn, with an LMS position
    planted on the cut (the last far one) or right behind it (the first near one) -> [(S, cut, planted position)]"""
    out = []
    for r in range(32):
        for behind in (0, 1):
            n = 1100 + r
            S = gen.iid(n, 100 + r).copy()
            cut = n - 125
            q = cut + behind
            S[q - 1:q + 2] = (3, 0, 1)
            S.setflags(write=False)
            out.append((S, cut, q))
    assert {c % 32 for _, c, _ in out} == set(range(32))
    return out


def tiny_windows(n):
    return sorted({(lo, hi) for lo in (0, 1, n // 2, n - 1, n) for hi in (0, 1, n // 2, n - 1, n, 32 if n > 32 else n) if 0 <= lo <= hi <= n})
