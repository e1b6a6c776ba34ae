"""tests/fm_chain_model.py against an independent statement of the definition: f(i) is the best score over EVERY sequence of
anchors that ends in i and whose consecutive pairs are allowed, found by enumeration; every reported chain is such a
sequence and its score recomputes; the tie rules on hand-made cases."""
import numpy as np

from tests import fm_chain_model as cm


def random_anchors(rng, A, spread):
    """anchors in (t, slot) order with many equal coordinates and a few diagonals"""
    t = np.sort(rng.integers(0, spread, A))
    r = np.clip(t - rng.integers(0, 4, A) * 3 + rng.integers(-2, 3, A), 0, None)
    l = rng.integers(1, 12, A)
    return r.tolist(), t.tolist(), l.tolist()


def best_by_enumeration(r, t, l, p):
    """best[i] = max over all allowed sequences ending in i of l_first + sum of steps, every sequence walked"""
    A = len(r)
    best = [None] * A

    def walk(i, score):  # score = the value of the sequence up to and including i
        if best[i] is None or score > best[i]:
            best[i] = score
        for k in range(i + 1, A):
            if cm.allowed(r[k], t[k], r[i], t[i], p):
                walk(k, score + cm.step(l[k], r[k], t[k], r[i], t[i], p))

    for i in range(A):
        walk(i, l[i])
    return best


def test_f_is_the_best_over_all_sequences():
    rng = np.random.default_rng(5)
    seen_pred = 0
    for case in range(300):
        A = int(rng.integers(1, 10))
        p = cm.params_of(max_gap=int(rng.integers(3, 40)), band=int(rng.integers(0, 12)), gap_cost=int(rng.integers(0, 30)),
                         max_lookback=0, min_score=int(rng.integers(0, 20)))
        r, t, l = random_anchors(rng, A, int(rng.integers(4, 60)))
        f, pred, root, depth = cm.dp(r, t, l, p)
        assert f == best_by_enumeration(r, t, l, p)
        seen_pred += sum(1 for x in pred if x >= 0)
        # every reported chain is an allowed sequence and its score recomputes
        for rec, path in cm.chains_of(r, t, l, p):
            score = l[path[0]]
            for a, b in zip(path, path[1:]):
                assert a < b and cm.allowed(r[b], t[b], r[a], t[a], p)
                score += cm.step(l[b], r[b], t[b], r[a], t[a], p)
            assert rec == (score, len(path), r[path[0]], r[path[-1]] + l[path[-1]], t[path[0]], t[path[-1]] + l[path[-1]])
            assert score == f[path[-1]] >= p["min_score"]
            assert all(root[a] == path[0] for a in path) and [depth[a] for a in path] == list(range(len(path)))
        ends = [path[-1] for _, path in cm.chains_of(r, t, l, p)]
        for e in ends:  # the end has the largest f of its tree, and is the first anchor that has it
            tree = [i for i in range(A) if root[i] == root[e]]
            assert f[e] == max(f[i] for i in tree) and e == min(i for i in tree if f[i] == f[e])
    assert seen_pred > 200


def test_the_nearest_predecessor_wins_a_tie():
    p = cm.params_of(max_gap=100, band=100, gap_cost=0, max_lookback=0, min_score=0)
    # anchors 0 and 1 both give anchor 2 the score 10 + 5: f(0) = f(1) = 10, and l_2 = 5 is the smallest of (l, dr, dt);
    # 1 cannot follow 0 (dr = 0): two roots with f = 10
    r, t, l = [0, 0, 20], [0, 1, 21], [10, 10, 5]
    f, pred, root, depth = cm.dp(r, t, l, p)
    assert f == [10, 10, 15] and pred == [-1, -1, 1] and root == [0, 1, 1]


def test_a_predecessor_that_ties_with_a_fresh_start_wins():
    p = cm.params_of(max_gap=100, band=100, gap_cost=8, max_lookback=0, min_score=0)
    # through 0: 4 + min(6, 3, 5) - floor(2 * 8 / 8) = 4 + 3 - 2 = 5; afresh: 5... made equal with l_1 = 5
    r, t, l = [0, 3], [0, 5], [4, 5]
    f, pred, root, depth = cm.dp(r, t, l, p)
    assert f == [4, 5] and pred == [-1, 0] and depth == [0, 1]
    # one point less through 0: the fresh start wins
    r, t, l = [0, 3], [0, 5], [3, 5]
    assert cm.dp(r, t, l, p)[1] == [-1, -1]


def test_the_smallest_anchor_is_the_end_on_a_tie():
    p = cm.params_of(max_gap=100, band=0, gap_cost=0, max_lookback=0, min_score=0)
    # 1 and 2 both follow 0 with the same score, 2 cannot follow 1 (dr = 0)
    r, t, l = [0, 10, 10], [0, 10, 10], [5, 3, 3]
    f, pred, root, depth = cm.dp(r, t, l, p)
    assert f == [5, 8, 8] and pred == [-1, 0, 0]
    (rec, path), = cm.chains_of(r, t, l, p)
    assert path == [0, 1] and rec == (8, 2, 0, 13, 0, 13)


def test_lookback_and_the_batch_form():
    p = dict(max_gap=100, band=0, gap_cost=0, max_lookback=1, min_score=0)
    # three anchors on a diagonal with one off it in between: with a lookback of 1 anchor 3 cannot reach anchor 1
    start, length = [0, 50, 10, 20], [5, 5, 5, 5]
    res = cm.chain(start, length, [0, 0, 4, 4], [100, 105, 110, 120], [0, 1, 2, 3, 4], **p)
    assert res["chain_index"].tolist() == [0, 0, 3, 3] and res["dp_pairs"] == 3 and res["max_anchors"] == 4
    assert res["chains"].tolist() == [[5, 1, 0, 5, 100, 105], [5, 1, 50, 55, 105, 110], [10, 2, 10, 25, 110, 125]]
    assert res["anchor_index"].tolist() == [0, 1, 2, 4] and res["anchors"].tolist()[2:] == [[10, 110, 5], [20, 120, 5]]
    p["max_lookback"] = 0
    res = cm.chain(start, length, [0, 0, 4, 4], [100, 105, 110, 120], [0, 1, 2, 3, 4], **p)
    assert res["chains"].tolist() == [[15, 3, 0, 25, 100, 125], [5, 1, 50, 55, 105, 110]] and res["dp_pairs"] == 6
    # equal t: slot order; the positions of a seed are one anchor each
    res = cm.chain([7, 3], [4, 4], [0, 2], [9, 9, 9], [0, 1, 3], **p)
    assert res["anchors"].tolist() == [[7, 9, 4], [3, 9, 4], [3, 9, 4]] and res["n_anchors"] == 3
