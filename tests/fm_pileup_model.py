"""A plain restatement of the pileup counts of the mappings (include/kiss_hip_pileup.h, kiss_hip_fmi_pileup_dev).

walk() goes through one counted item exactly as the definition reads, column by column; pileup() runs a batch the way the C call
sees it: items from alignments, hits or pairs, the filter, the bad items, the window, accumulate.  tests/test_fm_pileup_model.py
holds it against a statement that shares no loop with it.
"""
import bisect

import numpy as np

from .fm_align_model import virtual_read
from .fm_md_model import is_bad, unpack_ops

PLANES = ("cov", "alt_a", "alt_c", "alt_g", "alt_t", "alt_n", "del", "ins")
COV, ALT_A, ALT_C, ALT_G, ALT_T, ALT_N, DEL, INS = range(8)
HIT_REVERSE, HIT_SECONDARY, HIT_SUPPLEMENTARY = 1, 2, 4
PAIR_NONE, PAIR_PROPER, PAIR_BAD_INPUT = 0xFFFFFFFF, 1, 64
DEFAULTS = dict(min_mapq=0, skip_flags=HIT_SECONDARY, proper_only=0)
COUNTS = ("items", "bad", "filtered", "unmapped", "counted", "columns", "alt_columns", "deleted_bases", "insertions", "clipped")
MASK = 0xFFFFFFFF


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    assert p["min_mapq"] <= 255 and not p["skip_flags"] & ~7
    return p


def walk(S, Rv, rbeg, tbeg, ops, lo, hi, counts, rep):
    """the walk of one counted item: adds into counts ((8, hi - lo), u32, modulo 2^32) and into the dict rep"""

    def add(plane, j):
        if lo <= j < hi:
            counts[plane, j - lo] = (int(counts[plane, j - lo]) + 1) & MASK
        else:
            rep["clipped"] += 1

    i, j = int(rbeg), int(tbeg)
    for op, ln in ops:
        if op == 0:
            for _ in range(ln):
                add(COV, j)
                rep["columns"] += 1
                if int(Rv[i]) > 3:
                    add(ALT_N, j)
                    rep["alt_columns"] += 1
                elif int(Rv[i]) != int(S[j]):
                    add(ALT_A + int(Rv[i]), j)
                    rep["alt_columns"] += 1
                i, j = i + 1, j + 1
        elif op == 2:
            for _ in range(ln):
                add(DEL, j)
                j += 1
            rep["deleted_bases"] += ln
        else:
            if j > 0:
                add(INS, j - 1)
            rep["insertions"] += 1
            i += ln


def field(recs, name, column):
    recs = np.asarray(recs)
    if recs.dtype.names:
        return recs[name].astype(np.int64).ravel()
    return recs.astype(np.int64)[:, column]


def items_of(C, hits, pairs, p):
    """-> per item: ("walk", aln) | ("bad",) | ("filtered",) | ("unmapped",)"""
    if hits is None:
        assert pairs is None
        return [("walk", a) for a in range(C)]
    h_aln, h_flags, h_mapq = field(hits, "aln", 0), field(hits, "flags", 1), field(hits, "mapq", 2)
    H = len(h_aln)
    out = []

    def filtered(mapq, flags):
        return mapq < p["min_mapq"] or (flags & p["skip_flags"]) != 0

    if pairs is None:
        for h in range(H):
            out.append(("filtered",) if filtered(int(h_mapq[h]), int(h_flags[h])) else ("walk", int(h_aln[h])))
        return out
    cols = {k: field(pairs, k, c) for c, k in enumerate(("hit1", "hit2", "flags", "tlen", "score", "sub1", "sub2", "mapq1", "mapq2", "n_conc"))}
    for pr in range(len(cols["flags"])):
        for m in range(2):
            h = int(cols["hit%d" % (m + 1)][pr])
            flags = int(cols["flags"][pr])
            if flags & PAIR_BAD_INPUT:
                out.append(("bad",))
            elif h == PAIR_NONE:
                out.append(("unmapped",))
            elif h >= H:
                out.append(("bad",))
            elif p["proper_only"] and not flags & PAIR_PROPER:
                out.append(("filtered",))
            elif filtered(int(cols["mapq%d" % (m + 1)][pr]), int(h_flags[h]) & ~HIT_SECONDARY):
                out.append(("filtered",))
            else:
                out.append(("walk", int(h_aln[h])))
    return out


def pileup(text, reads, alns, chain_index, cigar, cigar_index, both_strands=False, hits=None, pairs=None, lo=0, hi=None, counts=None,
           order=None, **params):
    """a batch as the C call sees it.  alns: rows whose columns 2..5 are rbeg, rend, tbeg, tend, or a structured array; hits / pairs:
    structured arrays or integer rows in the order of the record's fields; counts: (8, W) to add to (not changed), None: from
    zero; order: a permutation of the items to go through them in (the result does not depend on it) -> dict(counts, and the
    report's counts)"""
    p = params_of(**params)
    alns = np.asarray(alns)
    if alns.dtype.names:
        quads = np.stack([alns[k].astype(np.int64) for k in ("rbeg", "rend", "tbeg", "tend")], axis=1).reshape(-1, 4)
    else:
        quads = np.asarray(alns, np.int64).reshape(-1, 12)[:, 2:6]
    cidx = [int(c) for c in chain_index]
    V = len(cidx) - 1
    assert V == (2 * len(reads) if both_strands else len(reads))
    C = cidx[V] - cidx[0]
    n = len(text)
    hi = n if hi is None else int(hi)
    lo = int(lo)
    assert 0 <= lo <= hi <= n
    out = np.zeros((8, hi - lo), np.uint32) if counts is None else np.array(counts, np.uint32).reshape(8, hi - lo).copy()
    items = items_of(C, hits, pairs, p)
    rep = dict.fromkeys(COUNTS, 0)
    rep["items"] = len(items)
    vreads = {}
    for g in (range(len(items)) if order is None else order):
        it = items[g]
        if it[0] != "walk":
            rep[it[0]] += 1
            continue
        a = it[1]
        if a >= C:
            rep["bad"] += 1
            continue
        ops = unpack_ops(cigar[int(cigar_index[a]):int(cigar_index[a + 1])])
        if not ops:
            rep["counted"] += 1
            continue
        v = bisect.bisect_right(cidx, cidx[0] + a, 0, V) - 1
        if v not in vreads:
            vreads[v] = virtual_read(reads[v // 2] if both_strands else reads[v], both_strands and v % 2 == 1)
        Rv = vreads[v]
        if is_bad(quads[a], ops, len(Rv), n):
            rep["bad"] += 1
            continue
        rep["counted"] += 1
        walk(text, Rv, quads[a][0], quads[a][2], ops, lo, hi, out, rep)
    rep["counts"] = out
    return rep


def base_counts(counts, text_window):
    """(5, W): the A, C, G, T and no-base read bases per position, position by position"""
    c = np.asarray(counts, np.int64).reshape(8, -1)
    out = np.zeros((5, c.shape[1]), np.int64)
    for j in range(c.shape[1]):
        for b in range(5):
            out[b, j] = c[ALT_A + b, j]
        if int(text_window[j]) <= 3:
            out[int(text_window[j]), j] += c[COV, j] - sum(int(c[ALT_A + b, j]) for b in range(5))
    return out.astype(np.uint32)
