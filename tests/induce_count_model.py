"""The model's side of tests/test_induce_count_gpu.py (no GPU): where the count pass of the induction meets an item whose
context word has no bases left.  TEST ONLY.

  KEPT_TILES_PER_WAVE            tiles a wave of the count pass takes
  planted(case, placement)       full context words of the far list with zeros ("0 = gather") at chosen places of LMS(A)
  run_outs(case, bases, ...)     the induction walked pass by pass (as induce_model.schedule walks it) with the number of
                                 bases every item's word holds when its pass reads it -> per pass, the items that have none
"""
import numpy as np

from tests import induce_model as im

TILE = 2048


# tiles a wave of the count pass takes: 2, 4 and 8 were measured and lost to 1, so a wave has one
KEPT_TILES_PER_WAVE = 1


# ---- zeros planted in the far list ----------------------------------------------------------------------------------------
# A lane of the word path takes items 256 q + 4 lane + e of its tile, q = 0 .. 7, e = 0 .. 3 (induce.hip: count_word_tile)
PLACEMENTS = {
    "first_of_tile": [0],
    "last_of_tile": [TILE - 1],
    "item3_of_lane63": [4 * 63 + 3],
    "two_in_one_lane": [4 * 17 + 1, 256 * 5 + 4 * 17 + 2],
    "whole_lane": [256 * q + 4 * 40 + e for q in range(8) for e in range(4)],
    "one_per_tile": None,
    "every_word": None,
}


def lms_layout(case):
    """-> (isfar per merged index, far index per merged index, [(first merged index, items)] per LMS pass)"""
    isfar = np.zeros(case.n + 1, dtype=bool)
    isfar[case.far_asc] = True
    far_in_order = isfar[case.order]
    far_index = np.cumsum(far_in_order) - 1
    passes, a = [], 0
    for c in range(4):
        passes.append((a, case.sch.lms_pass[c]))
        a += case.sch.lms_pass[c]
    assert a == case.order.size
    return far_in_order, far_index, passes


def block_tile(case):
    """the last full tile of LMS(A) without a near-end suffix inside (the count pass reads it as a block of words)
    -> (tile, near-end suffixes in front of it = how far its words lie below their merged index)"""
    far_in_order, far_index, passes = lms_layout(case)
    a, N = passes[0]
    for t in range(N // TILE - 1, -1, -1):
        if far_in_order[a + t * TILE:a + (t + 1) * TILE].all():
            return t, int((~far_in_order[:a + t * TILE]).sum())
    raise AssertionError("%s: no full tile of LMS(A) without a near-end suffix" % case.name)


def planted(case, placement):
    """-> (context words of case.far, number of zeros planted)"""
    cw = im.ctx_words(case.S, case.far)
    assert ((cw & 0x7FFFFFFE) != 0).sum() >= cw.size - 1, "full words: at most position 0 has no base in front of it"
    far_in_order, far_index, passes = lms_layout(case)
    if placement == "every_word":
        return np.zeros_like(cw), cw.size
    if placement == "one_per_tile":
        where = []
        for a, N in passes:
            for t in range((N + TILE - 1) // TILE):
                size = min(TILE, N - t * TILE)
                j = a + t * TILE + (37 * t + 11) % size
                while j < a + t * TILE + size and not far_in_order[j]:  # (a near-end suffix has no word in the far list)
                    j += 1
                if j < a + t * TILE + size:
                    where.append(j)
    else:
        t, _ = block_tile(case)
        where = [passes[0][0] + t * TILE + off for off in PLACEMENTS[placement]]
        assert all(far_in_order[j] for j in where)
    cw[far_index[where]] = 0
    return cw, len(where)


# ---- words that run out beside SA -----------------------------------------------------------------------------------------
class Pass:
    def __init__(self, sweep, name, rnd, N, kind):
        self.sweep, self.name, self.round, self.N, self.kind = sweep, name, rnd, N, kind
        self.empties = []  # pass-order indices of the items (position > 0) read without a base in their word

    def full_tiles_with_run_out(self):
        return sorted({i // TILE for i in self.empties if (i // TILE + 1) * TILE <= self.N})


def run_outs(case, far_bases, small_max, collapse_n, max_n):
    """The passes of both sweeps with the items whose word has no bases when the pass reads it.

    far_bases: bases in the word of every entry of case.far (a near-end suffix comes with a full word).  A pass of the tile
    kernels or the one-workgroup kernel refreshes a word without bases from the text (min(15, v) bases) and keeps it; what
    it appends inherits the parent's word less one base.  The closed form of a chain writes freshly gathered words and is
    not known to keep what it refreshes: NB None = not known, and nothing is claimed about such an item.
    kind: 'tile', 'small' or 'closed' as induce_model.expected_paths routes the pass."""
    S, n = case.S, case.n
    stype, lms, cnt, cntS, cntL, cntLMS, start = im._layout(S)
    Sl = S.tolist()
    collapse_max = min(collapse_n, im.default_m_cap(max_n))
    nb_lms = {int(p): min(15, int(p)) for p in case.near}
    for p, b in zip(case.far.tolist(), np.asarray(far_bases).tolist()):
        nb_lms[int(p)] = min(int(b), int(p))
    groups = im._groups(S, case.order)
    SA = [-1] * (n + 1)
    NB = [None] * (n + 1)
    SA[0] = n
    passes = []

    def run(ps, slots, items, allowed, pos, step):
        for i, (slot, v) in enumerate(zip(slots, items)):
            b = NB[slot] if slot is not None else nb_lms[v] if v != n else 0
            if b == 0 and v > 0:
                ps.empties.append(i)
                b = min(15, v) if ps.kind != "closed" else None
                if slot is not None:
                    NB[slot] = b
            if v > 0 and allowed[Sl[v - 1]]:
                c = Sl[v - 1]
                SA[pos[c]] = v - 1
                NB[pos[c]] = min(15, v - 1) if ps.kind == "closed" else (None if b is None else b - 1)
                pos[c] += step
        passes.append(ps)

    def kind_of(N):
        return "tile" if N > small_max else "small"

    pos = start[:4]
    run(Pass("L", "sentinel", 1, 1, "small"), [None], [n], [True] * 4, pos, 1)
    for c in range(4):
        a, rnd, kind = start[c], 0, None
        while pos[c] > a:
            N = pos[c] - a
            rnd += 1
            if kind not in ("closed", "small"):
                kind = "closed" if N <= collapse_max else kind_of(N)
            run(Pass("L", "L-part(%s)" % im.BASES[c], rnd, N, kind), list(range(a, a + N)), SA[a:a + N], [x >= c for x in range(4)], pos, 1)
            a += N
        g = groups[c]
        if g:
            run(Pass("L", "LMS(%s)" % im.BASES[c], 1, len(g), kind_of(len(g))), [None] * len(g), g, [x > c for x in range(4)], pos, 1)
    pos = [start[c + 1] - 1 for c in range(4)]
    for c in range(3, -1, -1):
        hi, rnd, kind = start[c + 1], 0, None
        while pos[c] + 1 < hi:
            N = hi - (pos[c] + 1)
            rnd += 1
            if kind not in ("closed", "small"):
                kind = "closed" if N <= collapse_max else kind_of(N)
            run(Pass("S", "S-part(%s)" % im.BASES[c], rnd, N, kind), list(range(hi - 1, hi - N - 1, -1)), SA[hi - N:hi][::-1],
                [x <= c for x in range(4)], pos, -1)
            hi -= N
        if c > 0 and cntL[c]:
            lo = start[c]
            run(Pass("S", "L-part(%s)" % im.BASES[c], 1, cntL[c], kind_of(cntL[c])), list(range(lo + cntL[c] - 1, lo - 1, -1)),
                SA[lo:lo + cntL[c]][::-1], [x < c for x in range(4)], pos, -1)
    assert np.array_equal(np.asarray(SA, dtype=np.int64), case.want.astype(np.int64)), case.name + ": the walk does not give the model's SA"
    return passes


def tile_passes_with_run_out(passes, sweep):
    """[(pass name, round, full tiles that hold an item without bases)] over the tile passes beside SA (not the LMS passes)"""
    return [(p.name, p.round, p.full_tiles_with_run_out()) for p in passes
            if p.sweep == sweep and p.kind == "tile" and not p.name.startswith("LMS") and p.full_tiles_with_run_out()]
