"""tests/fm_pileup_model.py held against a second statement of include/kiss_hip_pileup.h that shares no loop with it: every item
is expanded from its CIGAR alone into (kind, i, j) triples -- numpy ranges, no walk -- the items are classified by array
expressions, and the planes come from np.add.at.  500 random batches in the three modes, cases worked by hand, and the
properties the definition promises.  No GPU needed.  random_batch() also feeds tests/test_fm_pileup_gpu.py."""
import numpy as np
import pytest

from tests import fm_pileup_model as pm
from tests.fm_align_model import virtual_read

M, I, D = 0, 1, 2


# ---- the second statement ----------------------------------------------------------------------------------------------------------
def triples(rbeg, tbeg, ops):
    """-> kinds ('M' columns, 'D' bases, 'I' ops), each an (k, 2) array of (i, j): where the read and the text stand"""
    op = np.array([o for o, _ in ops], np.int64)
    ln = np.array([l for _, l in ops], np.int64)
    i0 = int(rbeg) + np.concatenate([[0], np.cumsum(np.where(op != D, ln, 0))[:-1]])
    j0 = int(tbeg) + np.concatenate([[0], np.cumsum(np.where(op != I, ln, 0))[:-1]])
    out = {}
    for kind, code in (("M", M), ("D", D)):
        sel = np.flatnonzero(op == code)
        within = np.concatenate([np.arange(ln[k]) for k in sel]) if sel.size else np.zeros(0, np.int64)
        rep = np.repeat(sel, ln[sel])
        out[kind] = np.stack([i0[rep] + (within if kind == "M" else 0), j0[rep] + within], axis=1).reshape(-1, 2)
    sel = np.flatnonzero(op == I)
    out["I"] = np.stack([i0[sel], j0[sel] - 1], axis=1).reshape(-1, 2)
    return out


def second(text, reads, alns, cidx, cigar, oidx, both, hits, pairs, lo, hi, counts, p):
    text = np.asarray(text, np.int64)
    alns = np.asarray(alns, np.int64).reshape(-1, 12)
    cidx = np.asarray(cidx, np.int64)
    V = cidx.size - 1
    C = int(cidx[V] - cidx[0])
    n = text.size
    # which alignment every item is (-1: none), and why not
    if hits is None:
        aln, state = np.arange(C), np.zeros(C, np.int64)
    else:
        hits = np.asarray(hits, np.int64).reshape(-1, 8)
        H = hits.shape[0]
        if pairs is None:
            idx, mapq, flags, state = np.arange(H), hits[:, 2], hits[:, 1], np.zeros(H, np.int64)
        else:
            pairs = np.asarray(pairs, np.int64).reshape(-1, 10)
            idx = pairs[:, 0:2].reshape(-1)
            mapq = pairs[:, 7:9].reshape(-1)
            pflags = np.repeat(pairs[:, 2], 2)
            state = np.select([(pflags & 64) != 0, idx == 0xFFFFFFFF, idx >= H, (p["proper_only"] != 0) & ((pflags & 1) == 0)], [1, 3, 1, 2], 0)
            idx = np.where(state == 0, idx, 0)
            flags = (hits[idx, 1] if H else np.zeros(idx.size, np.int64)) & ~2
        if hits.shape[0]:
            drop = (mapq < p["min_mapq"]) | ((flags & p["skip_flags"]) != 0)
            state = np.where((state == 0) & drop, 2, state)
            aln = hits[idx, 0]
        else:
            aln = np.zeros(idx.size, np.int64)
    rep = dict.fromkeys(pm.COUNTS, 0)
    rep["items"] = int(state.size)
    rep["bad"], rep["filtered"], rep["unmapped"] = [int((state == s).sum()) for s in (1, 2, 3)]
    adds = []  # (plane, j)
    for g in np.flatnonzero(state == 0):
        a = int(aln[g])
        if a >= C:
            rep["bad"] += 1
            continue
        ops = [(int(w) & 15, int(w) >> 4) for w in cigar[int(oidx[a]):int(oidx[a + 1])]]
        if not ops:
            rep["counted"] += 1
            continue
        v = int(np.searchsorted(cidx[:V], cidx[0] + a, side="right")) - 1
        Rv = virtual_read(reads[v // 2] if both else reads[v], both and v % 2 == 1).astype(np.int64)
        rbeg, rend, tbeg, tend = [int(x) for x in alns[a, 2:6]]
        op = np.array([o for o, _ in ops])
        ln = np.array([l for _, l in ops])
        good = (op <= 2).all() and (ln > 0).all() and ln[op != D].sum() == rend - rbeg and ln[op != I].sum() == tend - tbeg
        if op.max() > 2 or not good or rend > Rv.size or tend > n or rbeg > rend or tbeg > tend:
            rep["bad"] += 1
            continue
        rep["counted"] += 1
        t = triples(rbeg, tbeg, ops)
        m = t["M"]
        r, s = Rv[m[:, 0]], text[m[:, 1]]
        alt = np.where(r > 3, pm.ALT_N, np.where(r != s, pm.ALT_A + np.minimum(r, 3), 0))
        adds += [np.stack([np.zeros(len(m), np.int64), m[:, 1]], 1), np.stack([alt[alt > 0], m[alt > 0, 1]], 1),
                 np.stack([np.full(len(t["D"]), pm.DEL), t["D"][:, 1]], 1)]
        ins = t["I"][t["I"][:, 1] >= 0]
        adds.append(np.stack([np.full(len(ins), pm.INS), ins[:, 1]], 1))
        rep["columns"] += len(m)
        rep["alt_columns"] += int((alt > 0).sum())
        rep["deleted_bases"] += len(t["D"])
        rep["insertions"] += len(t["I"])
    adds = np.concatenate(adds) if adds else np.zeros((0, 2), np.int64)
    inside = (adds[:, 1] >= lo) & (adds[:, 1] < hi)
    rep["clipped"] = int((~inside).sum())
    out = np.zeros((8, hi - lo), np.uint64) if counts is None else np.array(counts, np.uint64).reshape(8, hi - lo)
    np.add.at(out, (adds[inside, 0], adds[inside, 1] - lo), 1)
    rep["counts"] = (out & 0xFFFFFFFF).astype(np.uint32)
    return rep


def same(a, b, what=""):
    for k in pm.COUNTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["counts"].dtype == b["counts"].dtype == np.uint32 and a["counts"].shape == b["counts"].shape, what
    assert np.array_equal(a["counts"], b["counts"]), (what, np.argwhere(a["counts"] != b["counts"])[:5])


# ---- random batches ----------------------------------------------------------------------------------------------------------------
def random_ops(rng, L, room):
    """ops over at most L read bases and at most `room` text bases, at least one of each -> ops, read bases, text bases"""
    ops, r, t = [], 0, 0
    for _ in range(int(rng.integers(1, 7))):
        kind = int(rng.choice([M, M, M, I, D]))
        if ops and ops[-1][0] == kind:
            continue
        ln = int(rng.integers(1, 12))
        if kind != D and r + ln > L or kind != I and t + ln > room:
            continue
        ops.append((kind, ln))
        r += ln if kind != D else 0
        t += ln if kind != I else 0
    return ops, r, t


def random_batch(seed, n_max=160):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, n_max))
    text = rng.integers(0, 4, n).astype(np.uint8)
    text[rng.random(n) < 0.05] = 4
    both = bool(rng.integers(0, 2))
    Q = int(rng.integers(1, 6)) * 2
    reads = [rng.integers(0, 5 if rng.random() < 0.3 else 4, int(rng.integers(1, 50))).astype(np.uint8) for _ in range(Q)]
    V = 2 * Q if both else Q
    alns, words, per_v = [], [], []
    for v in range(V):
        L = reads[v // 2 if both else v].size
        k = int(rng.integers(0, 3))
        per_v.append(k)
        for _ in range(k):
            rec = [0] * 12
            ops, r, t = random_ops(rng, L, n)
            roll = rng.random()
            if roll < 0.1 or not ops:
                ops = []
            else:
                rbeg, tbeg = int(rng.integers(0, L - r + 1)), int(rng.integers(0, n - t + 1))
                rec[2:6] = [rbeg, rbeg + r, tbeg, tbeg + t]
                if roll < 0.3:  # a bad item of some kind
                    kind = int(rng.integers(0, 6))
                    if kind == 0:
                        ops[int(rng.integers(0, len(ops)))] = (int(rng.integers(3, 16)), 3)
                    elif kind == 1:
                        ops[int(rng.integers(0, len(ops)))] = (int(rng.integers(0, 3)), 0)
                    elif kind == 2:
                        rec[3] += 1
                    elif kind == 3:
                        rec[5] += 1
                    elif kind == 4:
                        rec[2], rec[3] = L + 5, L + 5 + r
                    else:
                        rec[4], rec[5] = n + 1, n + 1 + t
            alns.append(rec)
            words.append([(ln << 4) | op for op, ln in ops])
    first = int(rng.choice([0, 7, 1 << 33]))
    cidx = (np.concatenate([[0], np.cumsum(per_v)]) + first).astype(np.uint64)
    C = len(alns)
    b = dict(text=text, reads=reads, both=both, alns=np.array(alns, np.uint32).reshape(C, 12), cidx=cidx,
             cigar=np.array([w for ws in words for w in ws], np.uint32),
             oidx=np.concatenate([[0], np.cumsum([len(ws) for ws in words])]).astype(np.uint64))
    H = int(rng.integers(0, 2 * C + 3))
    hits = np.zeros((H, 8), np.uint32)
    hits[:, 0] = rng.integers(0, C + 2, H)
    hits[:, 1] = rng.choice([0, 0, 0, 1, 2, 4, 3, 5], H)
    hits[:, 2] = rng.integers(0, 61, H)
    hits[:, 3:] = rng.integers(0, 1 << 32, (H, 5))  # (no other field of a hit is read)
    P = int(rng.integers(0, 6))
    pairs = np.zeros((P, 10), np.uint32)
    pairs[:, 3:] = rng.integers(0, 1 << 32, (P, 7))
    pairs[:, 0:2] = np.where(rng.random((P, 2)) < 0.2, 0xFFFFFFFF, rng.integers(0, H + 2, (P, 2)))
    pairs[:, 2] = rng.choice([0, 1, 1, 1 | 16, 32, 64, 65], P)
    pairs[:, 7:9] = rng.integers(0, 61, (P, 2))
    b["hits"], b["pairs"] = hits, pairs
    lo = int(rng.integers(0, n + 1))
    hi = int(rng.integers(lo, n + 1))
    b["lo"], b["hi"] = (0, n) if rng.random() < 0.4 else (lo, hi)
    b["params"] = dict(min_mapq=int(rng.choice([0, 0, 20, 61])), skip_flags=int(rng.choice([0, 2, 2, 6, 1])), proper_only=int(rng.integers(0, 2)))
    b["mode"] = ("alignments", "hits", "pairs")[seed % 3]
    return b


def mode_args(b):
    return dict(hits=None if b["mode"] == "alignments" else b["hits"], pairs=b["pairs"] if b["mode"] == "pairs" else None)


def run_model(b, counts=None, order=None, **over):
    kw = dict(mode_args(b), lo=b["lo"], hi=b["hi"], **b["params"])
    kw.update(over)
    return pm.pileup(b["text"], b["reads"], b["alns"], b["cidx"], b["cigar"], b["oidx"], b["both"], counts=counts, order=order, **kw)


def run_second(b, counts=None):
    m = mode_args(b)
    return second(b["text"], b["reads"], b["alns"], b["cidx"], b["cigar"], b["oidx"], b["both"], m["hits"], m["pairs"], b["lo"], b["hi"], counts,
                  pm.params_of(**b["params"]))


def test_500_random_batches_against_the_second_statement():
    seen = dict.fromkeys(pm.COUNTS, 0)
    for seed in range(500):
        b = random_batch(seed)
        want = run_model(b)
        same(want, run_second(b), "seed %d (%s)" % (seed, b["mode"]))
        assert want["items"] == want["bad"] + want["filtered"] + want["unmapped"] + want["counted"]
        for k in pm.COUNTS:
            seen[k] += want[k]
    assert all(seen.values()), seen  # (every kind of item and of add occurred)


def test_properties_on_random_batches():
    for seed in range(0, 120):
        b = random_batch(seed)
        want = run_model(b)
        # COV and the clipped M columns are the M lengths of the counted items
        whole = run_model(b, lo=0, hi=b["text"].size)
        assert whole["clipped"] == 0 and int(whole["counts"][pm.COV].sum()) == whole["columns"] == want["columns"]
        assert np.array_equal(whole["counts"][:, b["lo"]:b["hi"]], want["counts"])
        assert want["clipped"] == int(whole["counts"].sum()) - int(want["counts"].sum())
        alts = whole["counts"][pm.ALT_A:pm.ALT_N + 1].sum(axis=0)
        assert (alts <= whole["counts"][pm.COV]).all() and int(alts.sum()) == want["alt_columns"]
        assert int(whole["counts"][pm.DEL].sum()) == want["deleted_bases"]
        # the order of the items changes nothing
        order = np.random.default_rng(seed).permutation(want["items"])
        same(want, run_model(b, order=[int(x) for x in order]), "permuted %d" % seed)
        # two calls with accumulate give the sum (modulo 2^32)
        start = np.random.default_rng(seed + 1).integers(0, 1 << 32, want["counts"].shape).astype(np.uint32)
        twice = run_model(b, counts=run_model(b, counts=start)["counts"])
        assert np.array_equal(twice["counts"], start + want["counts"] + want["counts"])
        same(run_model(b, counts=start), run_second(b, counts=start), "accumulate %d" % seed)
        # base counts: every column is one base
        bc = pm.base_counts(whole["counts"], b["text"])
        known = b["text"] <= 3
        assert np.array_equal(bc[:, known].sum(axis=0), whole["counts"][pm.COV][known])


def test_pair_mode_on_hit_number_0_with_the_hits_mapq_is_hits_mode():
    for seed in range(60):
        b = random_batch(seed)
        hits = b["hits"].copy()
        H = hits.shape[0] // 2 * 2
        hits = hits[:H]
        hits[:, 1] &= ~np.uint32(2)  # (pair mode clears SECONDARY on the chosen hit)
        pairs = np.zeros((H // 2, 10), np.uint32)
        pairs[:, 0], pairs[:, 1] = np.arange(0, H, 2), np.arange(1, H, 2)
        pairs[:, 7], pairs[:, 8] = hits[0::2, 2], hits[1::2, 2]
        kw = dict(lo=b["lo"], hi=b["hi"], min_mapq=b["params"]["min_mapq"], skip_flags=b["params"]["skip_flags"])
        args = (b["text"], b["reads"], b["alns"], b["cidx"], b["cigar"], b["oidx"], b["both"])
        same(pm.pileup(*args, hits=hits, pairs=pairs, **kw), pm.pileup(*args, hits=hits, **kw), "seed %d" % seed)


# ---- by hand -----------------------------------------------------------------------------------------------------------------------
def one(text, read, rec, ops, both=False, v=0, **kw):
    reads = [np.array(read, np.uint8)]
    V = 2 if both else 1
    cidx = [0] * (v + 1) + [1] * (V - v)
    words = np.array([(ln << 4) | op for op, ln in ops], np.uint32)
    alns = np.zeros((1, 12), np.uint32)
    alns[0, 2:6] = rec
    return pm.pileup(np.array(text, np.uint8), reads, alns, cidx, words, [0, len(ops)], both, **kw)


def test_2d1i3d_by_hand():
    #        j: 0  1  2  3  4  5  6  7  8
    text = [0, 1, 2, 3, 0, 1, 2, 3, 0]
    # M2 over 0..1, D2 over 2..3, I1 behind 3, D3 over 4..6, M2 over 7..8 (the second column differs: read 1, text 0)
    r = one(text, [0, 1, 3, 3, 1], (0, 5, 0, 9), [(M, 2), (D, 2), (I, 1), (D, 3), (M, 2)])
    c = r["counts"]
    assert c[pm.COV].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 1]
    assert c[pm.DEL].tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0]
    assert c[pm.INS].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert c[pm.ALT_C].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1] and c[[1, 3, 4, 5]].sum() == 0
    assert [r[k] for k in pm.COUNTS] == [1, 0, 0, 0, 1, 4, 1, 5, 1, 0]


def test_an_insertion_first_at_0_and_at_lo():
    text = [0, 1, 2, 3, 0, 1]
    r = one(text, [3, 3, 0, 1], (0, 4, 0, 2), [(I, 2), (M, 2)])
    assert r["counts"].sum() == 2 and r["insertions"] == 1 and r["clipped"] == 0  # j = 0: no position in front
    r = one(text, [3, 3, 2, 3], (0, 4, 2, 4), [(I, 2), (M, 2)], lo=2, hi=6)
    assert r["counts"][pm.INS].sum() == 0 and r["insertions"] == 1 and r["clipped"] == 1  # j - 1 = 1 lies in front of lo
    r = one(text, [3, 3, 2, 3], (0, 4, 2, 4), [(I, 2), (M, 2)], lo=1, hi=6)
    assert r["counts"][pm.INS].tolist() == [1, 0, 0, 0, 0] and r["clipped"] == 0


def test_ops_cut_by_the_window_and_an_empty_window():
    text = [0, 1, 2, 3] * 5
    ops, rec, read = [(M, 4), (D, 4), (M, 4)], (0, 8, 4, 16), [0, 1, 2, 3, 0, 1, 2, 3]
    r = one(text, read, rec, ops, lo=6, hi=14)
    assert r["counts"][pm.COV].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and r["counts"][pm.DEL].tolist() == [0, 0, 1, 1, 1, 1, 0, 0]
    assert r["clipped"] == 4 and r["columns"] == 8 and r["deleted_bases"] == 4
    r = one(text, read, rec, ops, lo=9, hi=11)
    assert r["counts"][pm.DEL].tolist() == [1, 1] and r["counts"].sum() == 2 and r["clipped"] == 10
    for at in (0, 9, 20):
        r = one(text, read, rec, ops, lo=at, hi=at)
        assert r["counts"].shape == (8, 0) and r["clipped"] == 12 and r["counted"] == 1


def test_a_reverse_read_with_a_no_base_and_a_text_byte_of_4():
    text = [0, 1, 4, 3, 2, 2]
    # the read as sequenced; its reverse complement is [0, 1, 2, 4, 2, 1]: equal, equal, 2 over a text byte of 4 (never
    # equal: ALT_G), a no-base (ALT_N), equal, 1 over 2 (ALT_C)
    r = one(text, [2, 1, 4, 1, 2, 3], (0, 6, 0, 6), [(M, 6)], both=True, v=1)
    c = r["counts"]
    assert c[pm.COV].tolist() == [1] * 6 and c[pm.ALT_G].tolist() == [0, 0, 1, 0, 0, 0] and c[pm.ALT_N].tolist() == [0, 0, 0, 1, 0, 0]
    assert c[pm.ALT_C].tolist() == [0, 0, 0, 0, 0, 1] and r["alt_columns"] == 3
    bc = pm.base_counts(c, text)
    assert bc.T.tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 1], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0]]


def test_wrap_and_the_python_base_counts_agree_with_the_models():
    r = one([0, 1], [0, 1], (0, 2, 0, 2), [(M, 2)], counts=np.full((8, 2), 0xFFFFFFFF, np.uint32))
    assert r["counts"][pm.COV].tolist() == [0, 0] and r["counts"][pm.DEL].tolist() == [0xFFFFFFFF] * 2
    from kiss_amd import fm_pileup
    assert fm_pileup.PLANES == pm.PLANES
    for seed in range(40):
        b = random_batch(seed)
        whole = run_model(b, lo=0, hi=b["text"].size)
        assert np.array_equal(fm_pileup.base_counts(whole["counts"], b["text"]), pm.base_counts(whole["counts"], b["text"]))
    with pytest.raises(TypeError):
        fm_pileup.pileup_params(min_mapqq=1)
    with pytest.raises(ValueError):
        fm_pileup.pileup_params(min_mapq=256)
    with pytest.raises(ValueError):
        fm_pileup.pileup_params(skip_flags=8)
    p = fm_pileup.pileup_params()
    assert (p.min_mapq, p.skip_flags, p.proper_only, p.reserved_) == (0, 2, 0, 0)
