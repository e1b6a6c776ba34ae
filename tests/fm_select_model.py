"""A plain restatement of the selection of a read's mappings (include/kiss_hip.h, kiss_hip_fmi_select_dev).

select() runs a whole batch the way the C call sees it: alignment records (12 integers each), chain_index, the read lengths
and optionally the record starts of the text.  Everything is plain Python loops over integers, in the order the definition
reads; numpy only carries the arrays in and out.
"""
import numpy as np

DEFAULTS = dict(min_score=30, overlap=128, mapq_coef=120, mapq_max=60, max_hits=0)
LIMITS = dict(overlap=256, mapq_coef=65535, mapq_max=255)
HIT_REVERSE, HIT_SECONDARY, HIT_SUPPLEMENTARY = 1, 2, 4
HIT_FIELDS = ("aln", "flags", "mapq", "score", "sub", "n_sec", "head", "ref")
ALN_FIELDS = ("score", "flags", "rbeg", "rend", "tbeg", "tend", "matches", "mismatches", "ins", "del", "gaps", "band")
REPORT_COUNTS = ("Q", "V", "alignments", "candidates", "spanning", "redundant", "hits", "heads", "mapped", "max_candidates")


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    return p


def overlaps(x0, x1, y0, y1, share):
    """X and Y overlap by more than the share (in 256ths); a length below 0 counts as 0"""
    ov = max(0, min(x1, y1) - max(x0, y0))
    return ov * 256 > share * min(max(0, x1 - x0), max(0, y1 - y0))


def mapq_of(s, s2, coef, cap):
    return min(cap, (coef * (s - s2)) // s)


def record_of(bounds, tbeg, tend):
    """(rho, spanning) of a text interval; bounds has R + 1 entries"""
    R = len(bounds) - 1
    rho = 0
    for i in range(R + 1):  # the largest rho with bounds[rho] <= tbeg
        if bounds[i] <= tbeg:
            rho = i
    if rho >= R or tend > bounds[rho + 1]:
        return 0, True
    return rho, False


def walk(cands, L, p):
    """cands: the candidates of ONE read in order, each (a, score, rev, rbeg, rend, tbeg, tend, ref) with rbeg / rend in the
    virtual read -> (hits before the cap as dicts, number of redundant candidates)"""
    share = p["overlap"]
    kept = []
    redundant = 0
    for (a, score, rev, rbeg, rend, tbeg, tend, ref) in cands:
        r0, r1 = (L - rend, L - rbeg) if rev else (rbeg, rend)
        is_red = False
        for k in kept:
            if k["rev"] == rev and overlaps(tbeg, tend, k["t0"], k["t1"], share):
                is_red = True
                break
        if is_red:
            redundant += 1
            continue
        h = len(kept)
        g = None
        for k in kept:
            if k["is_head"] and overlaps(r0, r1, k["r0"], k["r1"], share):
                g = k
                break
        hit = dict(aln=a, score=score, rev=rev, r0=r0, r1=r1, t0=tbeg, t1=tend, ref=ref, sub=0, n_sec=0, number=h)
        if g is not None:
            hit["is_head"] = False
            hit["head"] = g["number"]
            hit["flags"] = (HIT_REVERSE if rev else 0) | HIT_SECONDARY
            g["n_sec"] += 1
            g["sub"] = max(g["sub"], score)
        else:
            first = True
            for k in kept:
                if k["is_head"]:
                    first = False
            hit["is_head"] = True
            hit["head"] = h
            hit["flags"] = (HIT_REVERSE if rev else 0) | (0 if first else HIT_SUPPLEMENTARY)
        kept.append(hit)
    for k in kept:
        k["mapq"] = mapq_of(k["score"], k["sub"] if k["n_sec"] else 0, p["mapq_coef"], p["mapq_max"]) if k["is_head"] else 0
    return kept, redundant


def as_rows(alns):
    """the structured array of the align call, or a (C, 12) integer array -> list of 12-tuples of Python ints"""
    if isinstance(alns, list):  # (rows of plain integers: the small inputs of the model's own tests)
        return [tuple(int(x) for x in r) for r in alns]
    alns = np.asarray(alns)
    if alns.dtype.names:
        return [tuple(int(r[k]) for k in ALN_FIELDS) for r in alns]
    return [tuple(int(x) for x in r) for r in alns.reshape(-1, 12)]


def select(alns, chain_index, read_lengths, both_strands=False, bounds=None, **params):
    """-> dict(hits: (n, 8) int64 array in the order of HIT_FIELDS, hit_index: Q + 1 int64, report: the counts)"""
    p = params_of(**params)
    rows = as_rows(alns)
    cidx = [int(x) for x in chain_index]
    lens = [int(x) for x in read_lengths]
    Q = len(lens)
    V = 2 * Q if both_strands else Q
    assert len(cidx) == V + 1
    c0 = cidx[0]
    C = cidx[V] - c0
    bnd = None if bounds is None else [int(x) for x in bounds]
    rep = dict(Q=Q, V=V, alignments=C, candidates=0, spanning=0, redundant=0, hits=0, heads=0, mapped=0, max_candidates=0)
    out = []
    hidx = [0]
    for q in range(Q):
        vs = (2 * q, 2 * q + 1) if both_strands else (q,)
        cands = []
        for v in vs:
            rev = bool(both_strands and v % 2 == 1)
            for c in range(cidx[v], cidx[v + 1]):
                a = c - c0
                score, flags, rbeg, rend, tbeg, tend = rows[a][:6]
                if flags != 0 or score < max(p["min_score"], 1):
                    continue
                ref = 0
                if bnd is not None:
                    ref, spanning = record_of(bnd, tbeg, tend)
                    if spanning:
                        rep["spanning"] += 1
                        continue
                cands.append((a, score, rev, rbeg, rend, tbeg, tend, ref))
        cands.sort(key=lambda c: (-c[1], c[0]))
        rep["candidates"] += len(cands)
        rep["max_candidates"] = max(rep["max_candidates"], len(cands))
        kept, red = walk(cands, lens[q], p)
        rep["redundant"] += red
        if p["max_hits"]:
            kept = kept[:p["max_hits"]]
        for k in kept:
            out.append([k["aln"], k["flags"], k["mapq"], k["score"], k["sub"] if k["is_head"] else 0,
                        k["n_sec"] if k["is_head"] else 0, k["head"], k["ref"]])
            rep["heads"] += 1 if k["is_head"] else 0
        rep["hits"] += len(kept)
        rep["mapped"] += 1 if kept else 0
        hidx.append(len(out))
    return dict(hits=np.array(out, dtype=np.int64).reshape(-1, 8), hit_index=np.array(hidx, dtype=np.int64), report=rep)
