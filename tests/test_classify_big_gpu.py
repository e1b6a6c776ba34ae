"""kiss_hip_stage_classify at the text sizes where the carry fold of the classification changes form (classify.hip,
kiss_classify: several tiles per thread and empty threads in k_tile_cin, the chunk level above 4096 tiles, several chunks per
thread above 16 384, the tile loops of the count pass above 2048 and of the emit pass above 8192 tiles), on texts whose planted
runs make the fold propagate across every boundary of that split (tests/classify_big_cases.py), against the run-length model
(tests/classify_big_model.py).  Every comparison is bit for bit.

The cases of one text stand together and a text, its model and its context are built once and released before the next one
(the largest holds about 3.5 GB of device memory)."""
import gc
import time

import numpy as np
import pytest

from tests import classify_big_cases as bc
from tests import classify_big_model as bm
from tests.stage_dev import VIEW_LOCAL_KEYS, VIEW_LOCAL_POS, Stage

pytestmark = pytest.mark.gpu

COUNTERS = ["count[%s]" % c for c in "ACGT"] + ["s_count[%s]" % c for c in "ACGT"] + ["lms_count[%s]" % c for c in "ACGT"] + ["far"]
SORT_TEXT = "emit_loop"
CASES = []
for _name in bc.TEXTS:
    CASES += [(_name, "whole", k) for k in bc.KS] + [(_name, "windows", None)]
    if _name == SORT_TEXT:
        CASES += [(_name, "sort", k) for k in (32, 256)]


class Big:
    def __init__(self, name):
        import kiss_amd
        t0 = time.perf_counter()
        self.name, self.plan = name, bc.plan(name)
        self.S = bc.text(name)
        self.M = bm.Model(self.S)
        self.ctx = kiss_amd.Context(max_n=self.plan.n, device=0)
        self.st = Stage(self.ctx)
        self.twelve = {}
        self.sample = None
        print("%s: text, model and context in %.1f s, %d LMS positions (%.3f per base)" % (
            name, time.perf_counter() - t0, self.M.lms.size, self.M.lms.size / self.plan.n))

    def counts13(self, k, lo, hi):
        if (lo, hi) not in self.twelve:  # (k enters the far count alone)
            self.twelve[lo, hi] = self.M.counts13(k, lo, hi)[:12]
        return self.twelve[lo, hi] + [self.M.far_count(k, self.M.window(lo, hi))]

    def close(self):
        self.ctx.close()
        self.st.texts.clear()
        self.st = self.M = self.S = None


_current = []


def release():
    import torch
    while _current:
        _current.pop().close()
    gc.collect()
    torch.cuda.empty_cache()


def current(name):
    if not _current or _current[0].name != name:
        release()
        _current.append(Big(name))
    return _current[0]


@pytest.fixture(scope="module", autouse=True)
def released_at_the_end():
    yield
    release()


def first_difference(b, what, got, want):
    """positions: the first index at which the lists differ, with where that position lies"""
    m = min(got.size, want.size)
    bad = np.flatnonzero(got[:m] != want[:m])
    if bad.size == 0 and got.size == want.size:
        return
    i = int(bad[0]) if bad.size else m
    g = "%d" % got[i] if i < got.size else "nothing"
    w = int(want[i]) if i < want.size else int(got[i])
    raise AssertionError("%s: %d entries, model %d; %d differ, first at index %d: %s, model has %s" % (
        what, got.size, want.size, bad.size, i, g, bc.where(b.plan, w) if i < want.size else "nothing, that is " + bc.where(b.plan, w)))


def check_window(b, k, lo, hi, wname, all_keys):
    """one stage_classify call: the emitted list through the ctx's views, its far prefix, its keys, the 13 counters"""
    st, M, n = b.st, b.M, b.plan.n
    what = "%s k=%d %s [%d, %d)" % (b.name, k, wname, lo, hi)
    rc, got = st.classify(b.S, k, lo, hi)
    assert rc == 0, (what, rc)
    pos = M.window(lo, hi)
    m_far = M.far_count(k, pos)
    m_got, far_got = st.sizes()
    got_pos = st.view(VIEW_LOCAL_POS, min(m_got, st.capacity())).astype(np.int64)
    first_difference(b, what + ": emitted positions", got_pos, pos)
    assert far_got == m_far, "%s: %d far, model %d; the first near one: %s" % (
        what, far_got, m_far, bc.where(b.plan, int(pos[m_far])) if m_far < pos.size else "none")
    D = bm.depth(n, k)
    assert D == 0 or (np.all(got_pos[:far_got] + D <= n) and np.all(got_pos[far_got:] + D > n)), what + ": the far ones are a prefix"
    want = b.counts13(k, lo, hi)
    assert got == want, "%s: counters differ: %s" % (what, ", ".join(
        "%s %d, model %d" % (COUNTERS[i], got[i], want[i]) for i in range(13) if got[i] != want[i]))
    # keys
    if all_keys:
        idx = np.arange(pos.size)
    else:
        if (lo, hi) == (0, n):
            if b.sample is None:
                b.sample = bc.key_sample(b.plan, pos)
            idx = b.sample
        else:
            idx = bc.key_sample(b.plan, pos)
    if idx.size:
        keys_t = st.view_tensor(VIEW_LOCAL_KEYS, pos.size)
        got_keys = keys_t[st.torch.from_numpy(idx).to(st.dev)].cpu().numpy().view(np.uint64)
        want_keys = M.keys(pos[idx])
        bad = np.flatnonzero(got_keys != want_keys)
        assert bad.size == 0, "%s: %d of %d compared keys differ, first at index %d: %016x, model %016x, %s" % (
            what, bad.size, idx.size, idx[bad[0]], got_keys[bad[0]], want_keys[bad[0]], bc.where(b.plan, int(pos[idx[bad[0]]])))
    return pos


def check_whole(b, k):
    pos = check_window(b, k, 0, b.plan.n, "whole", b.name == "fold2")
    if b.name != "fold2":  # the sample holds what it is there for
        s = set(pos[b.sample].tolist())
        for r in b.plan.runs:
            assert (r.lo in s) == (r.s_type and r.lo > 0) and (r.hi in s) == (not r.s_type and r.hi < b.plan.n), r
        assert all(q in s for _, q in b.plan.points)


def check_windows(b, k):
    for k in (bc.KS if b.name == "fold2" else (256,)):  # (k enters through the far count alone)
        for wname, (lo, hi) in bc.windows(b.plan).items():
            check_window(b, k, lo, hi, wname, b.name == "fold2")


def check_sort(b, k):
    """the whole sort on the device: the emit pass counts the digits of round 0 over several tiles per workgroup here, the
    radix sort consumes the counts, and the device verifier judges the suffix array"""
    torch, n = b.st.torch, b.plan.n
    assert b.plan.tiles > bm.EMIT_GRID
    d_S = b.st.upload(b.S)
    d_SA = torch.empty(n + 1, dtype=torch.int32, device=b.st.dev)
    b.st.sync()
    b.ctx.suffix_sort_dev(d_S.data_ptr(), n, d_SA.data_ptr(), k=k)
    rep = b.ctx.verify_sa_dev(d_S.data_ptr(), n, d_SA.data_ptr(), k)
    assert rep["ok"] == 1, rep  # permutation, SA[0] = n, k-order of every adjacent pair
    asc, srt, counts = b.ctx.stage_outputs()
    first_difference(b, "%s k=%d: ascending LMS list of the sort" % (b.name, k), asc.astype(np.int64), b.M.lms)
    assert [int(x) for x in counts] == b.counts13(k, 0, n)[:12]
    assert srt.size == asc.size


@pytest.mark.parametrize("name,what,k", CASES, ids=["%s-%s%s" % (n, w, "" if k is None else "-k%d" % k if k != bc.K_EXACT else "-exact")
                                                    for n, w, k in CASES])
def test_classification(name, what, k):
    t0 = time.perf_counter()
    {"whole": check_whole, "windows": check_windows, "sort": check_sort}[what](current(name), k)
    print("%s %s %s: %.2f s" % (name, what, k, time.perf_counter() - t0))
