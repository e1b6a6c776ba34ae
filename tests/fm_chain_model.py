"""Plain restatement of the chaining definition of include/kiss_hip.h (kiss_hip_fmi_chain_dev), for the tests.

Python integers and numpy over the lookback window; no cleverness.  Test infrastructure: nothing under kiss_amd/ imports it.
"""
import numpy as np

DEFAULTS = dict(max_gap=5000, band=500, gap_cost=2, max_lookback=64, min_score=40)
M32 = 0xFFFFFFFF


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown chain parameter %r" % k)
        p[k] = int(v)
    return p


def allowed(ri, ti, rj, tj, p):
    """anchor j = (rj, tj) may precede anchor i = (ri, ti), the order and the lookback aside"""
    dt, dr = ti - tj, ri - rj
    return dt > 0 and dr > 0 and dt <= p["max_gap"] and dr <= p["max_gap"] and abs(dt - dr) <= p["band"]


def step(li, ri, ti, rj, tj, p):
    """what an allowed pair adds to f(j)"""
    dt, dr = ti - tj, ri - rj
    return min(li, dr, dt) - (abs(dt - dr) * p["gap_cost"]) // 8


def dp(r, t, l, p):
    """anchors of one virtual read, already in (t, slot) order -> f, pred (-1: none), root, depth as lists of int"""
    A = len(r)
    r64, t64 = np.asarray(r, np.int64), np.asarray(t, np.int64)
    f, pred, root, depth = [0] * A, [-1] * A, [0] * A, [0] * A
    fa = np.zeros(A, np.int64)  # f once more, for the window
    look = p["max_lookback"]
    for i in range(A):
        lo = max(0, i - look) if look else 0
        best = (int(l[i]), 0)
        if i > lo:
            dt, dr = t64[i] - t64[lo:i], r64[i] - r64[lo:i]
            g = np.abs(dt - dr)
            ok = (dt > 0) & (dr > 0) & (dt <= p["max_gap"]) & (dr <= p["max_gap"]) & (g <= p["band"])
            gain = np.minimum(np.minimum(dt, dr), int(l[i]))
            score = fa[lo:i] + gain - (g * p["gap_cost"]) // 8
            idx = np.flatnonzero(ok)
            if idx.size:  # the largest score, and of those that have it the largest j
                top = int(score[idx].max())
                best = max(best, (top, lo + int(idx[score[idx] == top][-1]) + 1))
        f[i], pred[i] = best[0], best[1] - 1
        fa[i] = best[0]
        root[i] = i if pred[i] < 0 else root[pred[i]]
        depth[i] = 0 if pred[i] < 0 else depth[pred[i]] + 1
    return f, pred, root, depth


def chains_of(r, t, l, p):
    """-> [(record of six ints, [anchor numbers root .. end])] in ascending root"""
    f, pred, root, depth = dp(r, t, l, p)
    end = {}
    for i in range(len(r)):
        if root[i] not in end or f[i] > f[end[root[i]]]:  # (ascending i: the smallest i stays on ties)
            end[root[i]] = i
    out = []
    for ro in sorted(end):
        e = end[ro]
        if f[e] < p["min_score"]:
            continue
        path = [e]
        while pred[path[-1]] >= 0:
            path.append(pred[path[-1]])
        path.reverse()
        assert path[0] == ro and len(path) == depth[e] + 1
        rec = (f[e] & M32, len(path), int(r[ro]), (int(r[e]) + int(l[e])) & M32, int(t[ro]), (int(t[e]) + int(l[e])) & M32)
        out.append((rec, path))
    return out


def chain(start, length, seed_index, positions, pos_index, **kw):
    """The chain call on the arrays of the seeds call (start / length per seed).  -> dict(chains (n x 6 int64: score, anchors,
    rbeg, rend, tbeg, tend), chain_index, anchors (m x 3: rstart, tpos, len), anchor_index, and the report's totals)"""
    p = params_of(**kw)
    start, length = np.asarray(start, np.int64), np.asarray(length, np.int64)
    seed_index, pos_index = np.asarray(seed_index, np.int64), np.asarray(pos_index, np.int64)
    positions = np.asarray(positions, np.int64)
    V = seed_index.size - 1
    recs, cidx, ancs, aidx = [], [0], [], [0]
    total = dp_pairs = max_anchors = best = 0
    for v in range(V):
        r, t, l = [], [], []
        for s in range(int(seed_index[v]), int(seed_index[v + 1])):
            for h in range(int(pos_index[s]), int(pos_index[s + 1])):
                r.append(int(start[s]))
                t.append(int(positions[h]))
                l.append(int(length[s]))
        order = sorted(range(len(t)), key=lambda a: t[a])  # stable: ties stay in slot order
        r, t, l = [r[a] for a in order], [t[a] for a in order], [l[a] for a in order]
        A = len(r)
        total += A
        max_anchors = max(max_anchors, A)
        look = p["max_lookback"]
        dp_pairs += sum(min(i, look) if look else i for i in range(A))
        for rec, path in chains_of(r, t, l, p):
            recs.append(rec)
            best = max(best, rec[0])
            for a in path:
                ancs.append((r[a], t[a], l[a]))
            aidx.append(len(ancs))
        cidx.append(len(recs))
    return {"chains": np.array(recs, np.int64).reshape(len(recs), 6), "chain_index": np.array(cidx, np.int64),
            "anchors": np.array(ancs, np.int64).reshape(len(ancs), 3), "anchor_index": np.array(aidx, np.int64),
            "V": V, "n_anchors": total, "dp_pairs": dp_pairs, "max_anchors": max_anchors, "best_score": best}
