"""A plain restatement of the banded affine-gap local alignment of chains (include/kiss_hip.h, kiss_hip_fmi_align_dev).

align_plain() fills the whole matrix cell by cell into dicts, exactly as the definition reads, and walks back over the
final H / E / F values.  align_rows() computes the same values a row at a time with numpy (E as a running maximum along the
row: exact because gap_open >= 0) so that the GPU tests can afford reads of thousands of bases; tests/test_fm_align_model.py
holds the two against each other.  align() runs a whole batch the way the C call sees it.
"""
import numpy as np

DEFAULTS = dict(match=1, mismatch=4, gap_open=6, gap_extend=1, band=32)
MAX_BAND = 1024
CELLS_PER_N = 16
BAND_TOO_WIDE = 1
FIELDS = ("score", "flags", "rbeg", "rend", "tbeg", "tend", "matches", "mismatches", "ins", "del", "gaps", "band")
NEG = -(1 << 60)  # -inf


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    return p


def band_of(rbeg, rend, tbeg, tend, band):
    """(dlo, dhi, B)"""
    d0, d1 = int(tbeg) - int(rbeg), int(tend) - int(rend)
    dlo, dhi = min(d0, d1) - band, max(d0, d1) + band
    return dlo, dhi, dhi - dlo + 1


def virtual_read(read, odd):
    """the read, or its reverse complement (a no-base is its own complement)"""
    read = np.asarray(read, dtype=np.uint8)
    if not odd:
        return read
    rev = read[::-1]
    return np.where(rev <= 3, 3 - np.minimum(rev, 3), rev).astype(np.uint8)


def sub_score(x, y, p):
    if x > 3:
        return -1
    return p["match"] if x == y else -p["mismatch"]


def _walk(get, bi, bj, p):
    """the traceback from the best cell; get(i, j) -> (H, E, F, Hd + s, s > 0) of an existing cell -> the ops from the first
    to the last as [op, len] with op 0 M, 1 I, 2 D, the counts, and the point (i, j) the path starts at"""
    oe = p["gap_open"] + p["gap_extend"]
    i, j, state = bi, bj, "H"
    steps = []  # backwards: (op, matched)
    while True:
        if state == "H":
            if i == 0 or j == 0:
                break
            H, E, F, dg, eq = get(i, j)
            if H == 0:
                break
            if H == dg:
                steps.append((0, eq))
                i, j = i - 1, j - 1
            elif H == E:
                state = "E"
            else:
                assert H == F
                state = "F"
        elif state == "E":
            E = get(i, j)[1]
            steps.append((2, False))
            if E == get(i, j - 1)[0] - oe:
                state = "H"
            j -= 1
        else:
            F = get(i, j)[2]
            steps.append((1, False))
            if F == get(i - 1, j)[0] - oe:
                state = "H"
            i -= 1
    steps.reverse()
    ops = []
    for op, _ in steps:
        if ops and ops[-1][0] == op:
            ops[-1][1] += 1
        else:
            ops.append([op, 1])
    counts = dict(matches=sum(1 for op, eq in steps if op == 0 and eq), mismatches=sum(1 for op, eq in steps if op == 0 and not eq),
                  ins=sum(1 for op, _ in steps if op == 1), gaps=sum(1 for op, _ in ops if op != 0))
    counts["del"] = sum(1 for op, _ in steps if op == 2)
    return ops, counts, i, j


def _record(best, bi, bj, B, get, p):
    rec = dict.fromkeys(FIELDS, 0)
    rec["band"] = min(B, 0xFFFFFFFF)
    if best == 0:
        return rec, []
    ops, counts, i0, j0 = _walk(get, bi, bj, p)
    rec.update(counts)
    rec.update(score=best, rbeg=i0, rend=bi, tbeg=j0, tend=bj)
    return rec, ops


def align_plain(S, R, rbeg, rend, tbeg, tend, **kw):
    """one chain, the definition cell by cell -> (record dict, ops)"""
    p = params_of(**kw)
    S, R = [int(c) for c in S], [int(c) for c in R]
    n, L = len(S), len(R)
    o, e = p["gap_open"], p["gap_extend"]
    dlo, dhi, B = band_of(rbeg, rend, tbeg, tend, p["band"])
    if B > MAX_BAND:
        rec = dict.fromkeys(FIELDS, 0)
        rec.update(flags=BAND_TOO_WIDE, band=min(B, 0xFFFFFFFF))
        return rec, []
    H, E, F, D, Q = {}, {}, {}, {}, {}
    best, bi, bj = 0, 0, 0
    for i in range(1, L + 1):
        for j in range(max(1, i + dlo), min(n, i + dhi) + 1):
            s = sub_score(R[i - 1], S[j - 1], p)
            E[i, j] = max(H[i, j - 1] - o - e, E[i, j - 1] - e) if (i, j - 1) in H else NEG
            F[i, j] = max(H[i - 1, j] - o - e, F[i - 1, j] - e) if (i - 1, j) in H else NEG
            D[i, j] = H.get((i - 1, j - 1), 0) + s
            Q[i, j] = s > 0
            H[i, j] = max(0, D[i, j], E[i, j], F[i, j])
            if H[i, j] > best:  # (ascending i, then ascending j: the first of equals stays)
                best, bi, bj = H[i, j], i, j
    return _record(best, bi, bj, B, lambda i, j: (H[i, j], E[i, j], F[i, j], D[i, j], Q[i, j]), p)


def align_rows(S, R, rbeg, rend, tbeg, tend, **kw):
    """the same values a row at a time; band coordinates: diagonal k = j - i - dlo"""
    p = params_of(**kw)
    S, R = np.asarray(S, dtype=np.int64), np.asarray(R, dtype=np.int64)
    n, L = S.size, R.size
    o, e = p["gap_open"], p["gap_extend"]
    dlo, dhi, B = band_of(rbeg, rend, tbeg, tend, p["band"])
    if B > MAX_BAND:
        rec = dict.fromkeys(FIELDS, 0)
        rec.update(flags=BAND_TOO_WIDE, band=min(B, 0xFFFFFFFF))
        return rec, []
    ks = np.arange(B, dtype=np.int64)
    Hm = np.full((L + 1, B + 1), NEG, np.int64)  # NEG: no such cell (row 0 and column B never exist)
    Em, Fm, Dm = Hm.copy(), Hm.copy(), Hm.copy()
    Qm = np.zeros((L + 1, B + 1), bool)
    for i in range(1, L + 1):
        js = i + dlo + ks
        ok = (js >= 1) & (js <= n)
        if not ok.any():
            continue
        y = np.where(ok, S[np.clip(js - 1, 0, max(n - 1, 0))] if n else 0, -1)
        x = int(R[i - 1])
        s = np.full(B, -1 if x > 3 else -p["mismatch"], np.int64)
        if x <= 3:
            s[y == x] = p["match"]
        up_h, up_f = Hm[i - 1, 1:], Fm[i - 1, 1:]  # cell (i - 1, j) is diagonal k + 1 of the row above
        F = np.where(up_h > NEG, np.maximum(up_h - o - e, up_f - e), NEG)
        dg = np.maximum(Hm[i - 1, :B], 0) + s  # (an existing H is >= 0)
        T = np.maximum(np.maximum(dg, F), 0)
        U = np.where(ok, T + ks * e, NEG)
        run = np.maximum.accumulate(U)
        pre = np.concatenate([[NEG], run[:-1]])
        E = np.where(pre > NEG // 2, pre - o - ks * e, NEG)
        Hm[i, :B] = np.where(ok, np.maximum(T, E), NEG)
        Em[i, :B] = np.where(ok, E, NEG)
        Fm[i, :B] = np.where(ok, np.maximum(F, NEG), NEG)
        Dm[i, :B] = dg
        Qm[i, :B] = s > 0
    flat = int(np.argmax(Hm[:, :B]))  # the first of the largest: the smallest i, then the smallest diagonal
    bi, bk = divmod(flat, B)
    best = max(int(Hm[bi, bk]), 0)

    def get(i, j):
        k = j - i - dlo
        return int(Hm[i, k]), int(Em[i, k]), int(Fm[i, k]), int(Dm[i, k]), bool(Qm[i, k])

    return _record(best, bi, bi + dlo + bk, B, get, p)


def rescore(ops, rec, S, R, **kw):
    """the score of the ops laid over read and text from (rbeg, tbeg), and the point they end at"""
    p = params_of(**kw)
    i, j, sc = rec["rbeg"], rec["tbeg"], 0
    for op, ln in ops:
        if op == 0:
            for _ in range(ln):
                sc += sub_score(int(R[i]), int(S[j]), p)
                i, j = i + 1, j + 1
        else:
            sc -= p["gap_open"] + ln * p["gap_extend"]
            if op == 1:
                i += ln
            else:
                j += ln
    return sc, i, j


def cigar_string(ops):
    return "".join("%d%s" % (ln, "MID"[op]) for op, ln in ops)


def quads_of(chains):
    """(rbeg, rend, tbeg, tend) rows from a structured chain array or an (n, 4) array"""
    chains = np.asarray(chains)
    if chains.dtype.names:
        return np.stack([chains[k].astype(np.int64) for k in ("rbeg", "rend", "tbeg", "tend")], axis=1).reshape(-1, 4)
    return np.asarray(chains, np.int64).reshape(-1, 4)


def align(text, reads, chains, chain_index, both_strands=False, one=align_rows, **kw):
    """a batch as the C call sees it -> dict(alignments (C x 12 int64, FIELDS), cigar (u32 ops), cigar_index, cells, aligned,
    too_wide, best_score, max_band)"""
    p = params_of(**kw)
    quads = quads_of(chains)
    cidx = [int(c) for c in chain_index]
    V = len(cidx) - 1
    assert V == (2 * len(reads) if both_strands else len(reads))
    recs, cigar, oidx = [], [], [0]
    cells = too_wide = max_band = 0
    for v in range(V):
        R = virtual_read(reads[v // 2] if both_strands else reads[v], both_strands and v % 2 == 1)
        for c in range(cidx[v], cidx[v + 1]):
            rec, ops = one(text, R, *quads[c], **p)
            if rec["flags"] & BAND_TOO_WIDE:
                too_wide += 1
            else:
                cells += len(R) * rec["band"]
                max_band = max(max_band, rec["band"])
            recs.append([rec[k] for k in FIELDS])
            cigar += [(ln << 4) | op for op, ln in ops]
            oidx.append(len(cigar))
    C = len(recs)
    return {"alignments": np.array(recs, np.int64).reshape(C, 12), "cigar": np.array(cigar, np.uint32),
            "cigar_index": np.array(oidx, np.uint64), "cells": cells, "too_wide": too_wide, "aligned": C - too_wide,
            "best_score": max([r[0] for r in recs], default=0), "max_band": max_band}
