"""A plain restatement of mate rescue (include/kiss_hip.h: kiss_hip_fmi_rescue_dev, kiss_hip_fmi_aln_merge_dev).

plan() turns the pairs that are not proper into rescue chains, the way the C call sees a batch: pair records (10 integers
each), hits (8 each) with hit_index over the reads, the alignment records a hit's aln field indexes (12 each), the read
lengths, the text length and optionally the record bounds.  merge() puts two alignment sets of one batch behind each other,
virtual read by virtual read.  pipeline() composes both with the five models of the stages before.  Everything is plain
Python loops in the order the definition reads; numpy only carries the arrays in and out.
"""
import numpy as np

from tests import fm_align_model as am, fm_chain_model as cm, fm_pair_model as pm, fm_seed_model as sd, fm_select_model as sm

DEFAULTS = dict(ins_min=0, ins_max=1000, max_anchors=4, min_anchor_score=0, max_width=960)
MAX_WIDTH_TOP = am.MAX_BAND
CHAIN_FIELDS = ("score", "anchors", "rbeg", "rend", "tbeg", "tend")
REPORT_COUNTS = ("P", "pairs_planned", "anchors", "chains", "split", "empty", "bad_input", "max_chains")


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = int(v)
    assert p["ins_min"] <= p["ins_max"] and p["max_anchors"] >= 1 and 1 <= p["max_width"] <= MAX_WIDTH_TOP
    return p


def window(tbeg, tend, reverse, L, ins_min, ins_max):
    """the diagonals [dmin, dmax] next to an anchor, before the record clip (dmin > dmax: none)"""
    if not reverse:
        return max(tbeg + ins_min, tend, tbeg + L) - L, tbeg + ins_max - L
    return tend - ins_max, min(tend - ins_min, tbeg, tend - L)


def clip(dmin, dmax, lo, hi, L):
    return max(dmin, lo), min(dmax, hi - L)


def pieces(dmin, dmax, max_width):
    """[dmin, dmax] cut into ceil(W / max_width) pieces [a, b]"""
    W = dmax - dmin + 1
    k = -(-W // max_width)
    return [(dmin + j * W // k, dmin + (j + 1) * W // k - 1) for j in range(k)]


def plan(pairs, hits, hit_index, alns, read_lengths, n, bounds=None, **params):
    """-> dict(chains: (C, 6) int64 in the order of CHAIN_FIELDS, chain_index: 2 Q + 1 int64 over the virtual reads, origin: C
    int64, report: the counts)"""
    p = params_of(**params)
    PR = pm.rows_of(pairs, pm.PAIR_FIELDS)
    H = pm.rows_of(hits, pm.HIT_FIELDS)
    A = pm.rows_of(alns, pm.ALN_FIELDS)
    hidx = [int(x) for x in hit_index]
    lens = [int(x) for x in read_lengths]
    bnd = None if bounds is None else [int(x) for x in bounds]
    Q = len(lens)
    assert Q % 2 == 0 and len(hidx) == Q + 1 and len(PR) >= Q // 2
    rep = dict((k, 0) for k in REPORT_COUNTS)
    rep["P"] = Q // 2
    per_v = [[] for _ in range(2 * Q)]  # (chain row, origin)
    for pi in range(Q // 2):
        if PR[pi][2] & (pm.PROPER | pm.BAD_INPUT):
            continue
        of_pair = 0
        for m in (0, 1):
            q, o = 2 * pi + m, 2 * pi + 1 - m
            L = lens[q]
            taken = 0
            for h in range(hidx[o], hidx[o + 1]):
                aln, flags, _, score, _, _, head, ref = H[h]
                if head != 0 or score < p["min_anchor_score"]:
                    continue
                bad = not 0 <= aln < len(A)
                if not bad and not A[aln][4] < A[aln][5]:
                    continue
                if taken == p["max_anchors"]:
                    break
                taken += 1
                rep["anchors"] += 1
                if bad or (bnd is not None and ref >= len(bnd) - 1):
                    rep["bad_input"] += 1
                    continue
                rev = flags & pm.HIT_REVERSE
                lo, hi = (0, n) if bnd is None else (bnd[ref], bnd[ref + 1])
                dmin, dmax = clip(*window(A[aln][4], A[aln][5], rev, L, p["ins_min"], p["ins_max"]), lo, hi, L)
                if dmin > dmax:
                    rep["empty"] += 1
                    continue
                cut = pieces(dmin, dmax, p["max_width"])
                rep["split"] += 1 if len(cut) > 1 else 0
                v = 2 * q if rev else 2 * q + 1
                for a, b in cut:
                    per_v[v].append(([score, 0, 0, L, a, b + L], h))
                of_pair += len(cut)
        rep["pairs_planned"] += 1 if of_pair else 0
        rep["max_chains"] = max(rep["max_chains"], of_pair)
    chains, origin, cidx = [], [], [0]
    for v in range(2 * Q):
        for row, h in per_v[v]:
            chains.append(row)
            origin.append(h)
        cidx.append(len(chains))
    rep["chains"] = len(chains)
    return dict(chains=np.array(chains, np.int64).reshape(-1, 6), chain_index=np.array(cidx, np.int64),
                origin=np.array(origin, np.int64), report=rep)


def merge(alns_a, cidx_a, alns_b, cidx_b, cigar_a=None, oidx_a=None, cigar_b=None, oidx_b=None):
    """-> dict(alignments (C x 12 int64), chain_index (V + 1, from 0), source (C) and, with the ops of both sets, cigar /
    cigar_index)"""
    A, B = sm.as_rows(alns_a), sm.as_rows(alns_b)
    ia, ib = [int(x) for x in cidx_a], [int(x) for x in cidx_b]
    assert len(ia) == len(ib)
    V = len(ia) - 1
    CA = ia[V] - ia[0]
    want = cigar_a is not None
    out, src, cidx, cig, oidx = [], [], [0], [], [0]
    for v in range(V):
        for rows, idx, base, ops, oi in ((A, ia, 0, cigar_a, oidx_a), (B, ib, CA, cigar_b, oidx_b)):
            for c in range(idx[v], idx[v + 1]):
                i = c - idx[0]
                out.append(list(rows[i]))
                src.append(base + i)
                if want:
                    cig += [int(x) for x in ops[int(oi[i]):int(oi[i + 1])]]
                    oidx.append(len(cig))
        cidx.append(len(out))
    res = dict(alignments=np.array(out, np.int64).reshape(-1, 12), chain_index=np.array(cidx, np.int64), source=np.array(src, np.int64))
    if want:
        res.update(cigar=np.array(cig, np.uint32), cigar_index=np.array(oidx, np.uint64))
    return res


def pipeline(text, reads, bounds=None, min_len=19, max_occ=500, chain_params=None, align_params=None, select_params=None,
             pair_params=None, rescue_params=None):
    """pass 1, rescue and pass 2 on the models: reads 2 p and 2 p + 1 are the mates of pair p -> dict of every stage's output"""
    sp, pp = select_params or {}, pair_params or {}
    rp = dict(rescue_params or {})
    for k in ("ins_min", "ins_max"):
        rp.setdefault(k, pm.params_of(**pp)[k])
    lens = [len(r) for r in reads]
    seeds = sd.Batch(text, reads, True, 0).seeds(min_len, max_occ)
    ch = cm.chain(seeds["start"], seeds["len"], seeds["seed_index"], seeds["positions"], seeds["pos_index"], **(chain_params or {}))
    al = am.align(text, reads, ch["chains"][:, 2:6], ch["chain_index"], True, **(align_params or {}))
    sel = sm.select(al["alignments"], ch["chain_index"], lens, both_strands=True, bounds=bounds, **sp)
    pr = pm.pair(sel["hits"], sel["hit_index"], al["alignments"], **pp)
    pl = plan(pr["pairs"], sel["hits"], sel["hit_index"], al["alignments"], lens, len(text), bounds, **rp)
    al2 = am.align(text, reads, pl["chains"][:, 2:6], pl["chain_index"], True, **(align_params or {}))
    mg = merge(al["alignments"], ch["chain_index"], al2["alignments"], pl["chain_index"], al["cigar"], al["cigar_index"], al2["cigar"],
               al2["cigar_index"])
    sel2 = sm.select(mg["alignments"], mg["chain_index"], lens, both_strands=True, bounds=bounds, **sp)
    pr2 = pm.pair(sel2["hits"], sel2["hit_index"], mg["alignments"], **pp)
    rescued = sum(1 for x, y in zip(pr["pairs"], pr2["pairs"]) if int(y[2]) & pm.PROPER and not int(x[2]) & pm.PROPER)
    return dict(chains=ch, align=al, select=sel, pair=pr, plan=pl, rescue_align=al2, merge=mg, select2=sel2, pair2=pr2, rescued=rescued)


def random_mate(rng, count, span, nrefs=1, extra=0, top_score=150):
    """test inputs: `count` hits (tbeg, tend, reverse, score, ref, head, mapq) for fm_pair_model.batch_of, and `extra` that are
    no anchors (supplementary heads, empty intervals) mixed in behind hit 0"""
    out = []
    for _ in range(count):
        tb = int(rng.integers(0, span))
        out.append((tb, tb + int(rng.integers(1, 160)), int(rng.integers(0, 2)), int(rng.integers(1, top_score)), int(rng.integers(0, nrefs)), 0, 0))
    for _ in range(extra if count else 0):
        at = int(rng.integers(1, len(out) + 1))
        tb = int(rng.integers(0, span))
        out.insert(at, (tb, tb + 100, int(rng.integers(0, 2)), 150, 0, 1, 0) if rng.integers(0, 2) else (tb + 50, tb, int(rng.integers(0, 2)), 150, 0, 0, 0))
    return out


def random_case(rng, counts, span, nrefs=1, lens=(30, 151), first_aln=0, extra=0, **pair_params):
    """test inputs: one pair per entry (c1, c2) of counts -> dict(pairs: the records fm_pair_model.pair() gives them, hits,
    hit_index, alns, lens)"""
    mates = [(random_mate(rng, c1, span, nrefs, extra), random_mate(rng, c2, span, nrefs, extra)) for c1, c2 in counts]
    hits, hidx, alns = pm.batch_of(mates, first_aln)
    pairs = pm.pair(hits, hidx, alns, **pair_params)["pairs"]
    return dict(pairs=pairs, hits=hits, hit_index=hidx, alns=alns, lens=[int(rng.integers(*lens)) for _ in range(2 * len(counts))])
