"""The whole chain of stage calls of the sharded suffix sort for R ranks simulated in ONE process on one ctx, through the shipped
wrapper multi_gpu.GpuBackend and its views: classify a window, histogram, partition, "exchange" on the host, sort the received
key range in the ctx's buffers, induce.  No torch.distributed, no second process: what tests/test_multi_gpu.py runs with an even
split of one text and up to three ranks is run here with chosen windows (an empty one, a last one shorter than D) and up to
eight ranks, and every step on the way is held against tests/stage_model.py."""
import numpy as np
import pytest

from tests import stage_cases as sc
from tests import stage_model as sm

pytestmark = pytest.mark.gpu

BITS = sm.HIST_BITS
SHORT = 100  # bases of the last window of an uneven split: shorter than D = 125 and 375


def even(n, R):
    return [((n * r) // R, (n * (r + 1)) // R) for r in range(R)]


def uneven(n, R):
    """an empty window in the middle, a last window of SHORT bases"""
    edges = {2: [0, n - SHORT, n], 3: [0, n - SHORT, n - SHORT, n], 5: [0, n // 3, n // 3, n // 2 + 11, n - SHORT, n],
             8: [0, 1, 33, n // 4, n // 4, n // 2 + 11, (3 * n) // 4 + sc.TILE // 2, n - SHORT, n]}[R]
    assert len(edges) == R + 1 and all(a <= b for a, b in zip(edges, edges[1:]))
    return list(zip(edges, edges[1:]))


@pytest.fixture(scope="module")
def env():
    import torch
    import kiss_amd
    ctx = kiss_amd.Context(max_n=50_000, device=0)
    yield ctx, torch, torch.device("cuda", 0)
    ctx.close()


def host(t, dtype):
    return t.cpu().numpy().view(dtype).copy()


def k_id(k):
    return "exact" if k == sc.K_EXACT else "k%d" % k


CASES = [(R, split) for R in (1, 2, 3, 5, 8) for split in ("even", "uneven") if not (R == 1 and split == "uneven")]


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
@pytest.mark.parametrize("R,split", CASES, ids=["%d-%s" % c for c in CASES])
@pytest.mark.parametrize("name", ["runs_G", "tandem"])
def test_simulated_ranks(env, oracle, name, R, split, k):
    from kiss_amd import multi_gpu
    ctx, torch, dev = env
    S = sc.text(name)
    n = S.size
    D = sm.depth_of(n, k)
    windows = even(n, R) if split == "even" else uneven(n, R)
    if split == "uneven":
        assert windows[-1][1] - windows[-1][0] == SHORT and (R < 3 or any(lo == hi for lo, hi in windows))
        assert D == 0 or SHORT < D
    be = multi_gpu.GpuBackend(ctx, torch.from_numpy(np.array(S)).to(dev), k)
    # 1, 2: every rank classifies its window; the list is cloned at once (the next classification overwrites the views)
    lists, hists, near, total = [], [], [], [0] * 13
    for r, (lo, hi) in enumerate(windows):
        what = "%s k=%d rank %d of %d [%d, %d)" % (name, k, r, R, lo, hi)
        counts = be.classify(lo, hi)
        assert counts == sm.counts13(S, k, lo, hi), what
        keys, pos, m_far = be.local_lms()
        mkeys, mpos, mfar = sm.local_list(S, k, lo, hi)
        assert m_far == mfar and np.array_equal(host(pos, np.uint32), mpos) and np.array_equal(host(keys, np.uint64), mkeys), what
        hist = host(be.key_hist(keys[:m_far], BITS), np.uint64)
        assert np.array_equal(hist, sm.key_hist(mkeys[:mfar]).astype(np.uint64)), what + ": histogram"
        lists.append((keys[:m_far].clone(), pos[:m_far].clone()))
        near.append(mpos[mfar:])
        hists.append(hist.astype(np.int64))
        total = [a + b for a, b in zip(total, counts)]
    assert total == sm.counts13(S, k, 0, n)
    if split == "uneven" and D:
        assert near[-1].size == sm.local_list(S, k, *windows[-1])[1].size and lists[-1][1].numel() == 0  # (nothing far in the last window)
    splitters = multi_gpu.choose_splitters(np.sum(hists, axis=0), R)
    # 3: every rank partitions its list by destination; the host puts each destination's list together in source-rank order
    received = [([], []) for _ in range(R)]
    for r, (keys, pos) in enumerate(lists):
        sizes = multi_gpu.group_counts(hists[r], splitters, R)
        assert sum(sizes) == pos.numel()
        pk, pp = be.partition(keys, pos, BITS, splitters, R) if R > 1 else (keys, pos)
        pk, pp = host(pk, np.uint64), host(pp, np.uint32)
        edges = np.concatenate([[0], np.cumsum(sizes)])
        for g in range(R):
            received[g][0].append(pk[edges[g]:edges[g + 1]])
            received[g][1].append(pp[edges[g]:edges[g + 1]])
    # 4: the state of a rank behind its own classification, then the sort of each destination's list in the ctx's buffers
    be.classify(0, n)
    pieces, words = [], []
    for g in range(R):
        keys, pos = np.concatenate(received[g][0]), np.concatenate(received[g][1])
        what = "%s k=%d key range %d of %d" % (name, k, g, R)
        assert np.all(np.diff(pos.astype(np.int64)) > 0), what + ": the received list does not ascend by position"
        top = (keys >> np.uint64(64 - BITS)).astype(np.int64)
        assert np.all((top[:, None] >= np.asarray(splitters, dtype=np.int64)[None, :]).sum(1) == g), what + ": a key of another range"
        rkeys, rpos = be.recv_buffers(pos.size)
        rkeys.copy_(torch.from_numpy(keys.view(np.int64)).to(dev))
        rpos.copy_(torch.from_numpy(pos.view(np.int32)).to(dev))
        res = be.sort(rkeys, rpos)
        assert res is not None, what + ": KISS_HIP_E_DEEP"
        got, cw = host(res[0], np.uint32), host(res[1], np.uint32)
        assert np.array_equal(got, sm.sort_list(S, k, pos)), what
        assert all(sm.valid_ctx_word(S, p, w) for p, w in zip(got, cw)), what + ": context words"
        if D:
            tied = sm.tied(S, k, pos)
            assert all(int(w) >> 31 for p, w in zip(got, cw) if int(p) in tied), what + ": a tied suffix without the taint bit"
        pieces.append(got)
        words.append(cw)
    far_all = np.concatenate(pieces)
    far = [p for p in sm.lms(S).tolist() if sm.is_far(n, k, p)]
    assert np.array_equal(far_all, sm.sort_list(S, k, far)), "%s k=%d: the pieces in key-range order" % (name, k)
    # 5: the induction on "rank 0": summed counters, the near-end positions in rank order
    near_all = np.concatenate(near).astype(np.uint32)
    assert np.all(np.diff(near_all.astype(np.int64)) > 0) and near_all.size + far_all.size == sm.lms(S).size
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    SA = be.induce(to_dev(far_all), to_dev(near_all), total[:12], far_ctx=to_dev(np.concatenate(words)))
    assert np.array_equal(host(SA, np.uint32), oracle.suffix_sort(S, k)), "%s k=%d R=%d %s: the suffix array" % (name, k, R, split)
