"""A plain restatement of the pairing of the mappings of two mates (include/kiss_hip.h, kiss_hip_fmi_pair_dev).

pair() runs a whole batch the way the C call sees it: hits (8 integers each) with hit_index over the reads, and the alignment
records (12 integers each) a hit's aln field indexes.  Reads 2 p and 2 p + 1 are the mates of pair p.  Everything is plain
Python loops over every (x, y), in the order the definition reads; numpy only carries the arrays in and out.
"""
import numpy as np

DEFAULTS = dict(ins_min=0, ins_max=1000, ins_mean=400, pen_coef=8, pen_max=20, mapq_coef=120, mapq_max=60)
LIMITS = dict(pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255)
NONE = 0xFFFFFFFF
PROPER, MATE1_MAPPED, MATE2_MAPPED, SAME_REF, PROMOTED1, PROMOTED2, BAD_INPUT = 1, 2, 4, 8, 16, 32, 64
HIT_REVERSE = 1
HIT_FIELDS = ("aln", "flags", "mapq", "score", "sub", "n_sec", "head", "ref")
ALN_FIELDS = ("score", "flags", "rbeg", "rend", "tbeg", "tend", "matches", "mismatches", "ins", "del", "gaps", "band")
PAIR_FIELDS = ("hit1", "hit2", "flags", "tlen", "score", "sub1", "sub2", "mapq1", "mapq2", "n_conc")
REPORT_COUNTS = ("P", "eligible", "combinations", "concordant", "proper", "promoted", "lifted", "bad_input", "max_combinations")
SCORE_TOP = 1 << 30


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    return p


def rows_of(arr, fields):
    """a structured array, an (n, len(fields)) integer array or a list of rows -> list of tuples of Python ints"""
    if isinstance(arr, list):
        return [tuple(int(x) for x in r) for r in arr]
    arr = np.asarray(arr)
    if arr.dtype.names:
        return [tuple(int(r[k]) for k in fields) for r in arr]
    return [tuple(int(x) for x in r) for r in arr.reshape(-1, len(fields))]


def concordant(x, y, p):
    """x, y: (tbeg, tend, ref, reverse) of two eligible hits -> T, or None when the combination is not concordant"""
    if x[2] != y[2] or bool(x[3]) == bool(y[3]):
        return None
    f, r = (y, x) if x[3] else (x, y)
    if not (f[0] <= r[0] and f[1] <= r[1]):
        return None
    T = r[1] - f[0]
    if not p["ins_min"] <= T <= p["ins_max"]:
        return None
    return T


def pair_score(sx, sy, T, p):
    return max(1, sx + sy - min(p["pen_max"], (abs(T - p["ins_mean"]) * p["pen_coef"]) // 256))


def pair_mapq(own, S, sub, p):
    return max(own, min(p["mapq_max"], (p["mapq_coef"] * (S - sub)) // S))


def pair_one(h1, h2, first1, first2, alns, p):
    """h1, h2: the hits of mate 1 and mate 2 (rows of HIT_FIELDS); first1, first2: where their segments start in hits
    -> (the record as a list in the order of PAIR_FIELDS, dict of what the pair adds to the report)"""
    for h in h1 + h2:
        if not 0 <= h[0] < len(alns) or h[3] >= SCORE_TOP:
            return [0, 0, BAD_INPUT, 0, 0, 0, 0, 0, 0, 0], dict(bad_input=1)

    def view(h):  # (tbeg, tend, ref, reverse)
        return (alns[h[0]][4], alns[h[0]][5], h[7], h[1] & HIT_REVERSE)

    E1 = [x for x, h in enumerate(h1) if h[6] == 0 and view(h)[0] < view(h)[1]]
    E2 = [y for y, h in enumerate(h2) if h[6] == 0 and view(h)[0] < view(h)[1]]
    add = dict(eligible=len(E1) + len(E2), combinations=len(E1) * len(E2), concordant=0, proper=0, promoted=0, lifted=0)
    conc = []  # (S, x, y, T)
    for x in E1:
        for y in E2:
            T = concordant(view(h1[x]), view(h2[y]), p)
            if T is not None:
                conc.append((pair_score(h1[x][3], h2[y][3], T, p), x, y, T))
    add["concordant"] = len(conc)
    flags = (MATE1_MAPPED if h1 else 0) | (MATE2_MAPPED if h2 else 0)
    if conc:
        best = None
        for c in conc:  # the largest S, then the smallest x, then the smallest y
            if best is None or c[0] > best[0] or (c[0] == best[0] and (c[1], c[2]) < (best[1], best[2])):
                best = c
        S, x, y, T = best
        sub1 = max([c[0] for c in conc if c[1] != x], default=0)
        sub2 = max([c[0] for c in conc if c[2] != y], default=0)
        mapq1, mapq2 = pair_mapq(h1[x][2], S, sub1, p), pair_mapq(h2[y][2], S, sub2, p)
        flags |= PROPER | SAME_REF | (PROMOTED1 if x else 0) | (PROMOTED2 if y else 0)
        add["proper"] = 1
        add["promoted"] = (1 if x else 0) + (1 if y else 0)
        add["lifted"] = (1 if mapq1 > h1[x][2] else 0) + (1 if mapq2 > h2[y][2] else 0)
        return [first1 + x, first2 + y, flags, T, S, sub1, sub2, mapq1, mapq2, min(len(conc), 0xFFFFFFFF)], add
    score = (h1[0][3] if h1 else 0) + (h2[0][3] if h2 else 0)
    tlen = 0
    if h1 and h2 and h1[0][7] == h2[0][7]:
        flags |= SAME_REF
        a, b = view(h1[0]), view(h2[0])
        tlen = max(0, max(a[1], b[1]) - min(a[0], b[0]))
    return [first1 if h1 else NONE, first2 if h2 else NONE, flags, tlen, score, 0, 0, h1[0][2] if h1 else 0, h2[0][2] if h2 else 0,
            0], add


def pair(hits, hit_index, alns, **params):
    """-> dict(pairs: (P, 10) int64 array in the order of PAIR_FIELDS, report: the counts)"""
    p = params_of(**params)
    H = rows_of(hits, HIT_FIELDS)
    A = rows_of(alns, ALN_FIELDS)
    hidx = [int(x) for x in hit_index]
    Q = len(hidx) - 1
    assert Q % 2 == 0
    rep = dict((k, 0) for k in REPORT_COUNTS)
    rep["P"] = Q // 2
    out = []
    for q in range(0, Q, 2):
        rec, add = pair_one(H[hidx[q]:hidx[q + 1]], H[hidx[q + 1]:hidx[q + 2]], hidx[q], hidx[q + 1], A, p)
        out.append(rec)
        for k, v in add.items():
            rep[k] += v
        rep["max_combinations"] = max(rep["max_combinations"], add.get("combinations", 0))
    return dict(pairs=np.array(out, dtype=np.int64).reshape(-1, 10), report=rep)


def pair_windowed(hits, hit_index, alns, **params):
    """The same records by another route: per record of the text and per orientation, the reverse hits sorted by tend and the
    window ins_min <= r.tend - f.tbeg <= ins_max found by bisection; then the rules on the concordant list in another order
    (sort by (-S, x, y)).  An independent statement for tests/test_fm_pair_model.py to hold pair() against."""
    import bisect
    p = params_of(**params)
    H = rows_of(hits, HIT_FIELDS)
    A = rows_of(alns, ALN_FIELDS)
    hidx = [int(x) for x in hit_index]
    out = []
    for q in range(0, len(hidx) - 1, 2):
        seg = [H[hidx[q]:hidx[q + 1]], H[hidx[q + 1]:hidx[q + 2]]]
        if any(not 0 <= h[0] < len(A) or h[3] >= SCORE_TOP for h in seg[0] + seg[1]):
            out.append([0, 0, BAD_INPUT, 0, 0, 0, 0, 0, 0, 0])
            continue
        el = [[(n, A[h[0]][4], A[h[0]][5], h[7], h[1] & 1, h[3]) for n, h in enumerate(s) if h[6] == 0 and A[h[0]][4] < A[h[0]][5]]
              for s in seg]
        conc = []
        for fm in (0, 1):  # the mate that is forward
            fw = [e for e in el[fm] if not e[4]]
            for ref in set(e[3] for e in fw):
                rv = sorted((e for e in el[1 - fm] if e[4] and e[3] == ref), key=lambda e: e[2])
                ends = [e[2] for e in rv]
                for f in (e for e in fw if e[3] == ref):
                    lo = bisect.bisect_left(ends, max(f[1] + p["ins_min"], f[2]))
                    hi = bisect.bisect_right(ends, f[1] + p["ins_max"])
                    for r in rv[lo:hi]:
                        if r[1] >= f[1]:
                            T = r[2] - f[1]
                            S = max(1, f[5] + r[5] - min(p["pen_max"], abs(T - p["ins_mean"]) * p["pen_coef"] // 256))
                            conc.append((-S, f[0], r[0], T) if fm == 0 else (-S, r[0], f[0], T))
        conc.sort()
        flags = (MATE1_MAPPED if seg[0] else 0) | (MATE2_MAPPED if seg[1] else 0)
        if conc:
            nS, x, y, T = conc[0]
            sub1 = next((-c[0] for c in conc if c[1] != x), 0)
            sub2 = next((-c[0] for c in conc if c[2] != y), 0)
            m1 = max(seg[0][x][2], min(p["mapq_max"], p["mapq_coef"] * (-nS - sub1) // -nS))
            m2 = max(seg[1][y][2], min(p["mapq_max"], p["mapq_coef"] * (-nS - sub2) // -nS))
            out.append([hidx[q] + x, hidx[q + 1] + y, flags | PROPER | SAME_REF | (PROMOTED1 if x else 0) | (PROMOTED2 if y else 0), T, -nS,
                        sub1, sub2, m1, m2, len(conc)])
            continue
        a, b = (seg[0][0] if seg[0] else None), (seg[1][0] if seg[1] else None)
        tlen = 0
        if a and b and a[7] == b[7]:
            flags |= SAME_REF
            tlen = max(0, max(A[a[0]][5], A[b[0]][5]) - min(A[a[0]][4], A[b[0]][4]))
        out.append([hidx[q] if a else NONE, hidx[q + 1] if b else NONE, flags, tlen, (a[3] if a else 0) + (b[3] if b else 0), 0, 0,
                    a[2] if a else 0, b[2] if b else 0, 0])
    return np.array(out, dtype=np.int64).reshape(-1, 10)


def batch_of(pairs, first_aln=0):
    """test inputs: pairs = [(hits of mate 1, hits of mate 2), ...], a hit = (tbeg, tend, reverse, score[, ref[, head[, mapq]]])
    -> (hits rows, hit_index, alignment rows): one alignment record per hit, in an order that is not the hits' (reversed), behind
    first_aln records that no hit uses"""
    flat = [h for pr in pairs for mate in pr for h in mate]
    n = len(flat)
    alns = [(0, 0, 0, 0, 7, 3, 0, 0, 0, 0, 0, 65)] * first_aln + [None] * n
    hits, hidx = [], [0]
    for pr in pairs:
        assert len(pr) == 2
        for mate in pr:
            for h in mate:
                tbeg, tend, rev, score = h[:4]
                ref = h[4] if len(h) > 4 else 0
                head = h[5] if len(h) > 5 else 0
                mapq = h[6] if len(h) > 6 else 0
                a = first_aln + n - 1 - len(hits)
                alns[a] = (score, 0, 0, max(0, tend - tbeg), tbeg, tend, 0, 0, 0, 0, 0, 65)
                hits.append((a, (HIT_REVERSE if rev else 0) | (0 if len(hits) == hidx[-1] else 2 if head == 0 else 0), mapq, score, 0, 0,
                             head, ref))
            hidx.append(len(hits))
    return hits, hidx, alns
