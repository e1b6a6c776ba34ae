"""A plain restatement of the insert-size estimate (include/kiss_hip_insert.h, kiss_hip_fmi_insert_dev).

estimate() runs a whole batch the way the C call sees it: hits (8 integers each) with hit_index over the reads, and the
alignment records (12 integers each) a hit's aln field indexes.  Reads 2 p and 2 p + 1 are the mates of pair p; only hit
number 0 of either mate is looked at.  Everything is plain Python loops in the order the definition reads, on Python
integers; numpy only carries the histogram out.
"""
import numpy as np

from tests.fm_pair_model import ALN_FIELDS, HIT_FIELDS, HIT_REVERSE, rows_of

DEFAULTS = dict(min_mapq=20, max_insert=10000, min_samples=25, out_mult=2, map_mult=3, sd_mult=4)
LIMITS = dict(max_insert=65535, out_mult=255, map_mult=255, sd_mult=255)
OK = 1
CLASSES = ("unmapped", "bad_input", "low_mapq", "discordant", "too_long", "samples")
STATS = ("used", "q25", "q50", "q75", "mean", "sd", "ins_min", "ins_max", "ins_mean")
REPORT_COUNTS = ("P",) + CLASSES + ("flags",) + STATS


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    return p


def classify(h1, h2, alns, p):
    """h1, h2: the hits of mate 1 and mate 2 (rows of HIT_FIELDS) -> (class name, T or None)"""
    if not h1 or not h2:
        return "unmapped", None
    a, b = h1[0], h2[0]
    if not 0 <= a[0] < len(alns) or not 0 <= b[0] < len(alns):
        return "bad_input", None
    if a[2] < p["min_mapq"] or b[2] < p["min_mapq"]:
        return "low_mapq", None
    ta, tb = (alns[a[0]][4], alns[a[0]][5]), (alns[b[0]][4], alns[b[0]][5])
    ra, rb = a[1] & HIT_REVERSE, b[1] & HIT_REVERSE
    if a[7] != b[7] or ra == rb or ta[0] >= ta[1] or tb[0] >= tb[1]:
        return "discordant", None
    f, r = (tb, ta) if ra else (ta, tb)
    if not (f[0] <= r[0] and f[1] <= r[1]):
        return "discordant", None
    T = r[1] - f[0]
    if T > p["max_insert"]:
        return "too_long", None
    return "samples", T


def isqrt_loop(v):
    s = 0
    while (s + 1) * (s + 1) <= v:
        s += 1
    return s


def stats_of(hist, p):
    """hist: the counts by T (a list of max_insert + 1 integers) -> dict of flags and STATS"""
    out = dict((k, 0) for k in ("flags",) + STATS)
    N = 0
    for c in hist:
        N += c
    if N < max(p["min_samples"], 1):
        return out
    q = []
    for j in (1, 2, 3):
        rank = (j * N) // 4
        cum = 0
        for T, c in enumerate(hist):
            cum += c
            if cum > rank:
                q.append(T)
                break
    q25, q50, q75 = q
    iqr = q75 - q25
    M = total = 0
    for T, c in enumerate(hist):
        if q25 - p["out_mult"] * iqr <= T <= q75 + p["out_mult"] * iqr:
            M += c
            total += c * T
    mean = (total + M // 2) // M
    dev2 = 0
    for T, c in enumerate(hist):
        if q25 - p["out_mult"] * iqr <= T <= q75 + p["out_mult"] * iqr:
            dev2 += c * (T - mean) * (T - mean)
    sd = isqrt_loop(dev2 // M)
    out.update(flags=OK, used=M, q25=q25, q50=q50, q75=q75, mean=mean, sd=sd,
               ins_min=max(0, min(q25 - p["map_mult"] * iqr, mean - p["sd_mult"] * sd)),
               ins_max=max(q75 + p["map_mult"] * iqr, mean + p["sd_mult"] * sd), ins_mean=mean)
    return out


def estimate(hits, hit_index, alns, **params):
    """-> dict(report: the counts of REPORT_COUNTS, hist: uint32 array of max_insert + 1, classes: the class of every pair)"""
    p = params_of(**params)
    H = rows_of(hits, HIT_FIELDS)
    A = rows_of(alns, ALN_FIELDS)
    hidx = [int(x) for x in hit_index]
    Q = len(hidx) - 1
    assert Q % 2 == 0
    rep = dict((k, 0) for k in REPORT_COUNTS)
    rep["P"] = Q // 2
    hist = [0] * (p["max_insert"] + 1)
    classes = []
    for q in range(0, Q, 2):
        cls, T = classify(H[hidx[q]:hidx[q + 1]], H[hidx[q + 1]:hidx[q + 2]], A, p)
        classes.append(cls)
        rep[cls] += 1
        if T is not None:
            hist[T] += 1
    rep.update(stats_of(hist, p))
    return dict(report=rep, hist=np.array(hist, dtype=np.uint32), classes=classes)


def of_lengths(lengths, **params):
    """the report of a batch whose samples are exactly `lengths` (and no other pair)"""
    p = params_of(**params)
    hist = [0] * (p["max_insert"] + 1)
    for T in lengths:
        assert 1 <= T <= p["max_insert"]
        hist[int(T)] += 1
    rep = dict((k, 0) for k in REPORT_COUNTS)
    rep["P"] = rep["samples"] = len(lengths)
    rep.update(stats_of(hist, p))
    return dict(report=rep, hist=np.array(hist, dtype=np.uint32))
