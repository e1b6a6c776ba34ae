"""tests/fm_rescue_model.py held against statements that do not use its bookkeeping: the window against the pair model's own
concordance rule, diagonal by diagonal; the pieces as a partition; the clip; merge against select; and plan() against a second
statement of the whole batch in array form.  No GPU needed."""
import numpy as np

from tests import fm_pair_model as pm, fm_rescue_model as rm, fm_select_model as sm


def test_a_diagonal_lies_in_the_window_iff_the_pair_rule_accepts_the_mate_laid_there():
    seen = 0
    for ins_min, ins_max in ((0, 60), (25, 25), (10, 40), (0, 0), (35, 90)):
        p = pm.params_of(ins_min=ins_min, ins_max=ins_max)
        for tbeg in (100,):
            for alen in (1, 2, 7, 20, 33):
                for L in (1, 5, 20, 33, 50):
                    for rev in (0, 1):
                        A = (tbeg, tbeg + alen, 0, rev)
                        dmin, dmax = rm.window(A[0], A[1], rev, L, ins_min, ins_max)
                        ok = [d for d in range(tbeg - ins_max - L - 3, tbeg + alen + ins_max + L + 3)
                              if pm.concordant(A, (d, d + L, 0, 1 - rev), p) is not None]
                        assert ok == list(range(dmin, dmax + 1)), (A, L, ins_min, ins_max, dmin, dmax, ok[:1], ok[-1:])
                        for d in (dmin - 1, dmax + 1):
                            assert pm.concordant(A, (d, d + L, 0, 1 - rev), p) is None
                        # as mate 1 or as mate 2: the rule is symmetric in the mates
                        assert all(pm.concordant((d, d + L, 0, 1 - rev), A, p) is not None for d in ok)
                        seen += bool(ok)
    assert seen > 100


def test_the_pieces_partition_the_window_and_none_is_wider_than_max_width():
    for W in list(range(1, 80)) + [959, 960, 961, 1920, 1921, 2880, 5000]:
        for mw in (1, 2, 7, 64, 960, 1024):
            if W // mw > 3000:
                continue
            cut = rm.pieces(-17, -17 + W - 1, mw)
            assert len(cut) == -(-W // mw)
            assert cut[0][0] == -17 and cut[-1][1] == -17 + W - 1
            assert all(a <= b and b - a + 1 <= mw for a, b in cut), (W, mw)
            assert all(cut[j + 1][0] == cut[j][1] + 1 for j in range(len(cut) - 1))
            sizes = [b - a + 1 for a, b in cut]
            assert max(sizes) - min(sizes) <= 1  # (as even as integers allow)


def plan_arrays(pairs, hits, hit_index, alns, lens, n, bounds=None, **params):
    """the second statement: every hit of the batch at once, in numpy -> (chains, chain_index, origin, counts)"""
    p = rm.params_of(**params)
    PR = np.asarray(pairs, np.int64).reshape(-1, 10)
    H = np.asarray(hits, np.int64).reshape(-1, 8)
    A = np.asarray(alns, np.int64).reshape(-1, 12)
    hidx = np.asarray(hit_index, np.int64)
    lens = np.asarray(lens, np.int64)
    Q = lens.size
    nh = int(hidx[Q] - hidx[0])
    h = np.arange(hidx[0], hidx[Q])
    o = np.searchsorted(hidx, h, side="right") - 1          # the read that owns hit h (the last one that starts at or before it) ...
    q = o ^ 1                                                # ... and the mate it is an anchor for
    ok_pair = (PR[q // 2, 2] & (pm.PROPER | pm.BAD_INPUT)) == 0
    aln = H[h, 0]
    bad_aln = (aln < 0) | (aln >= A.shape[0])
    safe = np.where(bad_aln, 0, aln) if A.shape[0] else np.zeros(nh, np.int64)
    tb = A[safe, 4] if A.shape[0] else np.zeros(nh, np.int64)
    te = A[safe, 5] if A.shape[0] else np.zeros(nh, np.int64)
    qual = ok_pair & (H[h, 6] == 0) & (H[h, 3] >= p["min_anchor_score"]) & (bad_aln | (tb < te))
    rank = np.cumsum(qual) - qual                            # qualifying hits before h in the batch ...
    first = np.concatenate([[0], np.cumsum(qual)])[hidx[o] - hidx[0]]
    sel = qual & (rank - first < p["max_anchors"])           # ... and before h in its read
    ref = H[h, 7]
    if bounds is None:
        bad = sel & bad_aln
        lo, hi = np.zeros(nh, np.int64), np.full(nh, n, np.int64)
    else:
        b = np.asarray(bounds, np.int64)
        bad = sel & (bad_aln | (ref >= b.size - 1))
        r = np.where(ref >= b.size - 1, 0, ref)
        lo, hi = b[r], b[r + 1]
    L = lens[q] if nh else np.zeros(0, np.int64)
    rev = (H[h, 1] & 1) == 1
    dmin = np.where(rev, te - p["ins_max"], np.maximum(np.maximum(tb + p["ins_min"], te), tb + L) - L)
    dmax = np.where(rev, np.minimum(np.minimum(te - p["ins_min"], tb), te - L), tb + p["ins_max"] - L)
    dmin, dmax = np.maximum(dmin, lo), np.minimum(dmax, hi - L)
    good = sel & ~bad
    empty = good & (dmin > dmax)
    live = good & ~empty
    W = np.where(live, dmax - dmin + 1, 0)
    k = -(-W // p["max_width"])
    v = np.where(rev, 2 * q, 2 * q + 1)
    rows = []
    for i in np.flatnonzero(live):
        for j in range(int(k[i])):
            a = int(dmin[i]) + j * int(W[i]) // int(k[i])
            e = int(dmin[i]) + (j + 1) * int(W[i]) // int(k[i]) - 1
            rows.append((int(v[i]), int(h[i]), j, int(H[h[i], 3]), 0, 0, int(L[i]), a, e + int(L[i])))
    rows.sort()
    per_v = np.bincount([r[0] for r in rows], minlength=2 * Q) if rows else np.zeros(2 * Q, np.int64)
    per_pair = per_v.reshape(-1, 4).sum(axis=1) if Q else np.zeros(0, np.int64)
    counts = dict(P=Q // 2, pairs_planned=int((per_pair > 0).sum()), anchors=int(sel.sum()), chains=len(rows), split=int((k > 1).sum()),
                  empty=int(empty.sum()), bad_input=int(bad.sum()), max_chains=int(per_pair.max()) if Q else 0)
    return (np.array([r[3:] for r in rows], np.int64).reshape(-1, 6), np.concatenate([[0], np.cumsum(per_v)]).astype(np.int64),
            np.array([r[1] for r in rows], np.int64), counts)


def random_batch(rng):
    npairs = int(rng.integers(0, 7))
    counts = [(int(rng.choice((0, 1, 2, 3, 6))), int(rng.choice((0, 1, 2, 5)))) for _ in range(npairs)]
    nrefs = int(rng.integers(1, 4))
    case = rm.random_case(rng, counts, 600, nrefs, lens=(1, 200), first_aln=int(rng.integers(0, 3)), extra=int(rng.integers(0, 3)),
                          ins_max=int(rng.choice((100, 300, 1000))))
    bounds = None
    n = int(rng.integers(300, 900))
    if rng.integers(0, 2):
        cuts = sorted(set(int(x) for x in rng.integers(1, n, nrefs - 1))) if nrefs > 1 else []
        bounds = [0] + cuts + [n]
    params = dict(ins_min=int(rng.choice((0, 50, 120))), ins_max=int(rng.choice((120, 300, 700))), max_anchors=int(rng.choice((1, 2, 4, 9))),
                  min_anchor_score=int(rng.choice((0, 40, 149))), max_width=int(rng.choice((1, 37, 100, 960))) if rng.integers(0, 4) else 960)
    if params["max_width"] == 1:
        params["ins_max"] = params["ins_min"] + 30
    hits = [list(h) for h in case["hits"]]
    for h in hits:  # a few anchors that cannot be used, pair records that are no candidates
        if rng.random() < 0.03:
            h[0] = len(case["alns"]) + int(rng.integers(0, 3))
    pairs = case["pairs"].copy()
    for r in pairs:
        if rng.random() < 0.1:
            r[2] |= pm.BAD_INPUT
    return pairs, hits, case["hit_index"], case["alns"], case["lens"], n, bounds, params


def test_500_random_batches_against_the_statement_in_arrays():
    rng = np.random.default_rng(41)
    totals = dict((k, 0) for k in rm.REPORT_COUNTS)
    for _ in range(500):
        pairs, hits, hidx, alns, lens, n, bounds, params = random_batch(rng)
        got = rm.plan(pairs, hits, hidx, alns, lens, n, bounds, **params)
        chains, cidx, origin, counts = plan_arrays(pairs, hits, hidx, alns, lens, n, bounds, **params)
        assert np.array_equal(got["chains"], chains) and np.array_equal(got["chain_index"], cidx) and np.array_equal(got["origin"], origin)
        assert got["report"] == counts
        for k in totals:
            totals[k] += counts[k]
        # the clip: no chain leaves its record
        for c, h in zip(got["chains"], got["origin"]):
            lo, hi = (0, n) if bounds is None else (bounds[hits[h][7]], bounds[hits[h][7] + 1])
            assert lo <= c[4] and c[5] <= hi and c[5] - c[3] - c[4] + 1 <= params["max_width"] and c[3] >= 1, (c, lo, hi)
    print(totals)
    assert min(totals[k] for k in ("pairs_planned", "anchors", "chains", "split", "empty", "bad_input")) > 50


def aln_rows(rng, count, score=None):
    rows = []
    for _ in range(count):
        tb = int(rng.integers(0, 500))
        ln = int(rng.integers(20, 60))
        rb = int(rng.integers(0, 10))
        rows.append((int(rng.integers(30, 60)) if score is None else score, 0, rb, rb + ln, tb, tb + ln, ln, 0, 0, 0, 0, 65))
    return rows


def test_merge_with_an_empty_set_and_select_on_a_merge_with_records_of_score_0():
    rng = np.random.default_rng(42)
    for _ in range(40):
        Q = int(rng.integers(1, 5))
        V = 2 * Q
        na, nb = rng.integers(0, 5, V), rng.integers(0, 4, V)
        first_a, first_b = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        ia = np.concatenate([[first_a], first_a + np.cumsum(na)])
        ib = np.concatenate([[first_b], first_b + np.cumsum(nb)])
        A, B0 = aln_rows(rng, int(na.sum())), aln_rows(rng, int(nb.sum()), score=0)
        # B empty: A, from 0
        e = rm.merge(A, ia, [], np.full(V + 1, first_b))
        assert [tuple(r) for r in e["alignments"]] == A and list(e["chain_index"]) == list(ia - first_a) and list(e["source"]) == list(range(len(A)))
        e = rm.merge([], np.full(V + 1, first_a), A, ia)
        assert [tuple(r) for r in e["alignments"]] == A and list(e["source"]) == list(range(len(A)))
        # B with score 0 only: select sees A's alignments alone, under their new numbers
        m = rm.merge(A, ia, B0, ib)
        assert list(m["chain_index"]) == list((ia - first_a) + (ib - first_b)) and sorted(m["source"]) == list(range(len(A) + len(B0)))
        lens = [80] * Q
        on_a, on_m = sm.select(A, ia, lens, both_strands=True), sm.select(m["alignments"], m["chain_index"], lens, both_strands=True)
        back = on_m["hits"].copy()
        back[:, 0] = m["source"][back[:, 0]] if back.size else back[:, 0]
        assert np.array_equal(back, on_a["hits"]) and np.array_equal(on_m["hit_index"], on_a["hit_index"])
        # with ops: every alignment keeps its own
        oa = np.concatenate([[0], np.cumsum(rng.integers(0, 4, len(A)))])
        ob = np.concatenate([[0], np.cumsum(rng.integers(0, 4, len(B0)))])
        ca, cb = rng.integers(0, 1 << 20, int(oa[-1])), rng.integers(0, 1 << 20, int(ob[-1]))
        w = rm.merge(A, ia, B0, ib, ca, oa, cb, ob)
        for k, s in enumerate(w["source"]):
            want = ca[oa[s]:oa[s + 1]] if s < len(A) else cb[ob[s - len(A)]:ob[s - len(A) + 1]]
            assert list(w["cigar"][int(w["cigar_index"][k]):int(w["cigar_index"][k + 1])]) == list(want)
        assert int(w["cigar_index"][-1]) == len(ca) + len(cb)
