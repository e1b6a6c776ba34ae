"""Model of the FM-index search with mismatches (kiss_hip_fmi_query_mm_*).  It knows nothing of the GPU code.

A hit of pattern P (length L) in a text S of n bases under the bound e is a position p in [0, n - L] with Hamming distance
d = #{j : S[p + j] != P[j]} <= e.  Ground truth is `brute`: the text itself.  `mm_ranges` / `locate` / `fm_search` are the
FM-index route on top of tests/fm_model.py (backward search with backtracking, then a per-row LF walk to a sampled row,
bounded by SA_INTV - 1 steps): they give the leaf count and the walk-failure behaviour on suffix arrays that are not exact.
"""
import numpy as np


def brute(S, P, e):
    """-> counts (e + 1,), positions (ascending), mismatches.  One column at a time: n * L work per pattern."""
    S = np.asarray(S, dtype=np.uint8) & 3
    P = np.asarray(P, dtype=np.uint8) & 3
    n, L = S.size, P.size
    if L == 0 or L > n:
        return np.zeros(e + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    d = np.zeros(n - L + 1, np.int32)
    for j in range(L):
        d += S[j:n - L + 1 + j] != P[j]
    pos = np.flatnonzero(d <= e)
    mm = d[pos].astype(np.int64)
    return np.bincount(mm, minlength=e + 1)[:e + 1].astype(np.int64), pos.astype(np.int64), mm


def brute_batch(S, pats, e):
    """-> counts (Q, e + 1), positions, mismatches, index (Q + 1): the CSR layout of the library"""
    cs, ps, ms, idx = [], [], [], [0]
    for P in pats:
        c, p, m = brute(S, P, e)
        cs.append(c)
        ps.append(p)
        ms.append(m)
        idx.append(idx[-1] + p.size)
    Q = len(cs)
    return (np.array(cs, np.int64).reshape(Q, e + 1), np.concatenate(ps) if ps else np.zeros(0, np.int64),
            np.concatenate(ms) if ms else np.zeros(0, np.int64), np.array(idx, np.int64))


def exact_sa(S):
    """the exact suffix array by sorting the suffixes themselves (n + 1 entries, SA[0] = n); small texts only"""
    b = (np.asarray(S, dtype=np.uint8) & 3).tobytes()
    return np.array(sorted(range(len(b) + 1), key=lambda i: b[i:]), np.int64)


def k_ordered_sa(S, k, seed):
    """a k-ordered suffix array with the ties broken AT RANDOM: the worst case of what a sort of order k may return"""
    b = (np.asarray(S, dtype=np.uint8) & 3).tobytes()
    tie = np.random.default_rng(seed).random(len(b) + 1)
    return np.array(sorted(range(len(b) + 1), key=lambda i: (b[i:i + k], tie[i])), np.int64)


def mm_ranges(fm, P, e):
    """leaves (beg, end, mismatches) of the branching backward search on an FmModel; disjoint, none empty"""
    P = [int(x) & 3 for x in P]
    R, cnt = fm.R, [int(x) for x in fm.cnt]
    out = []
    stack = [(0, fm.N, len(P) - 1, 0)]
    while stack:
        beg, end, pos, d = stack.pop()
        if pos < 0:
            out.append((beg, end, d))
            continue
        for c in range(4):
            dd = d + (c != P[pos])
            if dd > e:
                continue
            nb, ne = cnt[c] + int(R[c, beg]), cnt[c] + int(R[c, end])
            if nb < ne:
                stack.append((nb, ne, pos - 1, dd))
    return out


def locate(fm, row):
    """text position of SA row `row` by the bounded LF walk, or None when no sampled row is reached within
    SA_INTV - 1 steps or before the primary row"""
    for step in range(fm.sa_intv):
        if fm.b is None or fm.b[row]:
            return int(fm.sa[row if fm.b is None else fm.brank[row]]) + step
        if row == fm.pri or step + 1 == fm.sa_intv:
            return None
        row = int(fm.lf(int(fm.bwt[row]), row))
    return None


def fm_search(fm, P, e, want_positions=True):
    """-> dict(counts, leaves, walk_failures[, positions, mismatches]) of one pattern by the FM route"""
    leaves = mm_ranges(fm, P, e)
    counts = np.zeros(e + 1, np.int64)
    hits, fails = [], 0
    for beg, end, d in leaves:
        counts[d] += end - beg
        if want_positions:
            for row in range(beg, end):
                p = locate(fm, row)
                if p is None:
                    fails += 1
                else:
                    hits.append((p, d))
    res = {"counts": counts, "leaves": len(leaves), "walk_failures": fails}
    if want_positions:
        hits.sort()
        res["positions"] = np.array([h[0] for h in hits], np.int64)
        res["mismatches"] = np.array([h[1] for h in hits], np.int64)
    return res


def patterns_for(S, Q, L, e, seed):
    """Q patterns of length L: two thirds cut from the text with 0 .. e + 1 random substitutions, the rest random; every
    third row gets bytes >= 4 with the same low two bits (the library uses pattern bytes & 3)"""
    rng = np.random.default_rng(seed)
    S = np.asarray(S, dtype=np.uint8)
    pats = rng.integers(0, 4, (Q, L), dtype=np.uint8)
    if S.size >= L:
        for q in range(Q):
            if q % 3 == 2:
                continue
            p = int(rng.integers(0, S.size - L + 1))
            row = S[p:p + L].copy()
            for _ in range(int(rng.integers(0, e + 2))):
                j = int(rng.integers(0, L))
                row[j] = (row[j] + 1 + rng.integers(0, 3)) & 3
            pats[q] = row
    pats[::3] |= (rng.integers(0, 64, (pats[::3].shape[0], L), dtype=np.uint8) << 2).astype(np.uint8)
    return np.ascontiguousarray(pats)
