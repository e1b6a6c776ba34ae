"""kiss_hip_fmi_insert_dev / _host on the GPU against tests/fm_insert_model.py: every field of the report and every bin of the
histogram.  (a) synthetic hits and alignment records -- the call takes arrays from anywhere --, placed with tests/dev_place.py:
records at 4-byte leads, hit_index at 8, the histogram between guard words; (b) the error contract; (c) the caller's stream
(the method of tests/test_dev_stream_gpu.py); (d) FMIndex.map_pairs(insert=...) on the texts of the FM tests, and against the
truth: a library of 1400 .. 1600 bases, of which the default parameters make no proper pair and the estimate makes every one."""
import ctypes
import functools

import numpy as np
import pytest

from tests import dev_place
from tests import fm_insert_model as im
from tests import fm_pair_model as pm
from tests.test_fm_insert_model import batch
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu
GUARD = 512
INIT = 0xEE
TOP = (1 << 32) - 4097
WINDOW = 16384  # the bins a workgroup keeps in LDS (kiss_amd/csrc/fm_insert.hip)
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=1 << 20, device=0)
    yield c
    c.close()


def device():
    import torch
    return torch.device("cuda", 0)


class Call:
    """one kiss_hip_fmi_insert_dev call on placed arrays; hits / alns: rows of integers, as the model takes them"""

    def __init__(self, ctx, hits, hidx, alns, want_hist=True, fill=0x5A, run=True, want=None, **params):
        from kiss_amd import _lib, fm_insert
        self.lib, self.ctx, dev = ctx._lib, ctx, device()
        self.p = fm_insert.insert_params(**params)
        self.want = want if want is not None else im.estimate(hits, hidx, alns, **params)
        ht = np.asarray(hits, np.int64).reshape(-1, 8).astype(np.uint32)
        al = np.asarray(alns, np.int64).reshape(-1, 12).astype(np.uint32)
        hx = np.asarray(hidx, np.uint64)
        self.Q = hx.size - 1
        self.aln_count = al.shape[0]
        put = lambda arr, lead: dev_place.place(arr, lead, GUARD, fill, device=dev)  # noqa: E731
        self.ins = {"hits": put(ht, 4), "hidx": put(hx, 8), "alns": put(al, 4)}
        self.outs = {"hist": dev_place.place_out(4 * (self.p.max_insert + 1), 4, GUARD, fill, device=dev)} if want_hist else {}
        self.rep = _lib.InsertReport()
        if run:
            self.run()

    def address(self, name):
        v = self.ins.get(name, self.outs.get(name))
        return vp(v.placement.address) if v is not None else None

    def run(self, stream=None, null=(), params=True):
        p = {k: (None if k in null else self.address(k)) for k in ("hits", "hidx", "alns", "hist")}
        self.rc = self.lib.kiss_hip_fmi_insert_dev(self.ctx._ctx, p["hits"], p["hidx"], self.Q, p["alns"], self.aln_count,
                                                   ctypes.byref(self.p) if params else None, p["hist"],
                                                   None if "report" in null else ctypes.byref(self.rep), stream)
        return self

    def fetch(self, name="hist", dtype=np.uint32):
        """through kiss_hip_copy_to_host: a blocking copy on the null stream, no torch call"""
        out = np.empty(self.outs[name].numel(), np.uint8)
        assert self.lib.kiss_hip_copy_to_host(vp(out.ctypes.data), self.address(name), out.size) == 0
        return out.view(dtype)

    def untouched(self):
        for name in self.outs:
            assert (self.fetch(name, np.uint8) == INIT).all(), name + " was written"
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())

    def check(self, what=""):
        w = self.want["report"]
        assert self.rc == 0, (what, self.rc)
        got = {k: getattr(self.rep, k) for k in im.REPORT_COUNTS}
        print("INSERT %-44s %s" % (what, got))
        assert got == w, (what, {k: (got[k], w[k]) for k in got if got[k] != w[k]})
        if self.outs:
            hist = self.fetch()
            bad = np.flatnonzero(hist != self.want["hist"])
            assert not bad.size, (what, "bin %d holds %d, the model says %d" % (bad[0], hist[bad[0]], self.want["hist"][bad[0]]))
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())
        return self


def pairs_of_lengths(lengths, rng, L=100):
    """for pm.batch_of(): one pair of MAPQ 60 per length, somewhere in the first 2^20 bases, the forward mate first in even pairs"""
    out = []
    for k, T in enumerate(lengths):
        s = int(rng.integers(0, 1 << 20))
        fwd, rev = (s, s + min(L, T), 0, 50, 0, 0, 60), (s + T - min(L, T), s + T, 1, 50, 0, 0, 60)
        out.append(([fwd], [rev]) if k % 2 == 0 else ([rev], [fwd]))
    return out


def both_ways(ctx, hits, hidx, alns, what, **params):
    """the histogram in the caller's array, then in the context's scratch: the same report"""
    c = Call(ctx, hits, hidx, alns, **params).check(what)
    Call(ctx, hits, hidx, alns, want_hist=False, want=c.want, **params).check(what + ", hist NULL")
    return c.want


# ---- (a) synthetic hits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (0, 1, 63, 64, 65, 255, 256, 257))
def test_pair_counts_around_the_wave_and_the_workgroup(ctx, P):
    rng = np.random.default_rng(100 + P)
    hits, hidx, alns = batch(rng, P, centre=400)
    want = both_ways(ctx, hits, hidx, alns, "P = %d" % P, min_samples=1)
    assert want["report"]["P"] == P and (P < 63 or want["report"]["samples"] > P // 10)
    both_ways(ctx, hits, hidx, alns, "P = %d, defaults" % P)


def test_one_hundred_thousand_pairs_in_one_bin(ctx):
    """the worst contention: every sample in one bin, inside the window of LDS and, with fewer pairs, past it"""
    for P, T, max_insert in ((100000, 400, 10000), (20000, 40000, 65535)):
        a = np.arange(2 * P, dtype=np.int64)
        hits = np.zeros((2 * P, 8), np.int64)
        hits[:, 0], hits[:, 1], hits[:, 2], hits[:, 3] = a[::-1], a & 1, 60, 50  # (mate 2 reverse; the records in another order)
        alns = np.zeros((2 * P, 12), np.int64)
        start = 1000 + 3 * (a // 2)
        alns[hits[:, 0], 4] = np.where(a & 1, start + T - 100, start)
        alns[hits[:, 0], 5] = np.where(a & 1, start + T, start + 100)
        want = Call(ctx, hits, np.arange(2 * P + 1), alns, max_insert=max_insert).check("%d pairs of T = %d" % (P, T)).want
        assert want["report"]["samples"] == want["report"]["used"] == P == int(want["hist"][T])
        assert (want["report"]["q25"], want["report"]["mean"], want["report"]["sd"], want["report"]["ins_max"]) == (T, T, 0, T)


def test_the_edges_of_T_of_max_insert_and_of_the_window(ctx):
    rng = np.random.default_rng(5)
    edges = [1, 2, WINDOW - 1, WINDOW, WINDOW + 1, 65534, 65535, 65536, 70000, TOP - (1 << 20)]
    for max_insert in (65535, WINDOW + 1, WINDOW, WINDOW - 1, WINDOW - 2, 10000, 2, 1):
        lengths = [T for T in edges + [max_insert - 1, max_insert, max_insert + 1] if T >= 1] * 3 + [WINDOW] * 5
        hits, hidx, alns = pm.batch_of(pairs_of_lengths(lengths, rng, L=150), first_aln=2)
        want = both_ways(ctx, hits, hidx, alns, "max_insert = %d" % max_insert, max_insert=max_insert, min_samples=1)
        n_long = sum(1 for T in lengths if T > max_insert)
        assert want["report"]["too_long"] == n_long > 0 and want["report"]["samples"] == len(lengths) - n_long
        assert want["hist"][1] == lengths.count(1) >= 3 and want["hist"][max_insert] >= 3 and want["report"]["flags"] == im.OK
    # positions up to the end of the largest text
    far = [([(TOP - T, TOP - T + 100, 0, 50, 0, 0, 60)], [(TOP - 100, TOP, 1, 50, 0, 0, 60)]) for T in (100, 101, 5000, WINDOW, 65535, 65536)]
    far += [([(0, 100, 0, 50, 0, 0, 60)], [(TOP - 100, TOP, 1, 50, 0, 0, 60)])]
    hits, hidx, alns = pm.batch_of(far)
    want = both_ways(ctx, hits, hidx, alns, "positions up to 2^32 - 4097", max_insert=65535, min_samples=1)
    assert want["report"]["samples"] == 5 and want["report"]["too_long"] == 2


def test_min_samples_and_min_mapq_at_their_boundaries(ctx):
    rng = np.random.default_rng(6)
    for N in (24, 25):
        lengths = [int(x) for x in rng.integers(300, 500, N)]
        hits, hidx, alns = pm.batch_of(pairs_of_lengths(lengths, rng) + [([], [(5, 9, 0, 50)])] * 3)
        for min_samples in (0, 1, 24, 25, 26):
            want = both_ways(ctx, hits, hidx, alns, "N = %d, min_samples = %d" % (N, min_samples), min_samples=min_samples)
            assert want["report"]["flags"] == (im.OK if N >= min_samples else 0) and want["report"]["samples"] == N
            assert (want["report"]["used"] > 0) == (N >= min_samples) and want["report"]["unmapped"] == 3
    pairs = []
    for q1, q2 in ((19, 60), (60, 19), (20, 20), (20, 60), (60, 20), (19, 19), (0, 0), (255, 255)):
        pairs.append(([(1000, 1100, 0, 50, 0, 0, q1)], [(1300, 1400, 1, 50, 0, 0, q2)]))
    hits, hidx, alns = pm.batch_of(pairs)
    for min_mapq, samples in ((20, 4), (21, 1), (0, 8), (19, 7), (255, 1), (256, 0)):
        want = both_ways(ctx, hits, hidx, alns, "min_mapq = %d" % min_mapq, min_mapq=min_mapq, min_samples=1)
        assert want["report"]["samples"] == samples and want["report"]["low_mapq"] == 8 - samples


def test_one_pair_of_every_class_beside_good_ones(ctx):
    rng = np.random.default_rng(7)
    good = pairs_of_lengths([int(x) for x in rng.integers(350, 450, 40)], rng)
    f, r = (1000, 1100, 0, 50, 0, 0, 60), (1300, 1400, 1, 50, 0, 0, 60)
    odd = [
        ([], [r]), ([f], []), ([], []),                                      # unmapped
        ([f], [r]), ([f], [r]),                                              # bad_input (made so below)
        ([f[:6] + (19,)], [r]),                                              # low_mapq
        ([f], [r[:4] + (1,) + r[5:]]),                                       # another record
        ([f], [(1300, 1400, 0) + r[3:]]), ([(1000, 1100, 1) + f[3:]], [r]),  # equal strands
        ([(1300, 1400, 0) + f[3:]], [(1000, 1100, 1) + r[3:]]),              # the forward hit behind the reverse one
        ([(1000, 1500, 0) + f[3:]], [(1100, 1400, 1) + r[3:]]),              # f.tend > r.tend
        ([f], [(1400, 1400, 1) + r[3:]]), ([(1100, 1000, 0) + f[3:]], [r]),  # tbeg = tend, tbeg > tend
        ([f], [(20000, 20100, 1) + r[3:]]),                                  # too_long
        ([f, (7, 9, 0, 30, 0, 0, 0)], [r, (1, 2, 0, 30, 0, 0, 0)]),          # later hits say nothing
    ]
    pairs = good[:20] + odd + good[20:]
    hits, hidx, alns = pm.batch_of(pairs, first_aln=1)
    hits = [list(h) for h in hits]
    hits[hidx[2 * 23]][0] = len(alns)          # one past the end, mate 1
    hits[hidx[2 * 24 + 1]][0] = 0xFFFFFFFF     # far out, mate 2
    hits[hidx[2 * 34] + 1][0] = 0xFFFFFFFF     # (a later hit: not looked at)
    want = both_ways(ctx, hits, hidx, alns, "every class")
    assert want["classes"][20:35] == ["unmapped"] * 3 + ["bad_input"] * 2 + ["low_mapq"] + ["discordant"] * 7 + ["too_long", "samples"]
    assert {k: want["report"][k] for k in im.CLASSES} == dict(unmapped=3, bad_input=2, low_mapq=1, discordant=7, too_long=1, samples=41)
    # aln_count is what bounds the reads of alns
    c = Call(ctx, hits, hidx, alns, want=im.estimate(hits, hidx, alns[:-9]), run=False)
    c.aln_count -= 9
    c.run().check("fewer records than the hits name")
    assert c.want["report"]["bad_input"] > 2


def test_the_mults_at_0_and_255_and_a_bimodal_set(ctx):
    rng = np.random.default_rng(8)
    lengths = [int(x) for x in rng.normal(400, 40, 300).clip(1, 10000)] + [int(x) for x in rng.integers(3000, 9000, 30)]
    hits, hidx, alns = pm.batch_of(pairs_of_lengths(lengths, rng))
    seen = set()
    for kw in (dict(), dict(out_mult=0), dict(out_mult=255), dict(map_mult=0, sd_mult=0), dict(map_mult=255, sd_mult=255),
               dict(out_mult=0, map_mult=255, sd_mult=0), dict(out_mult=1, map_mult=0, sd_mult=255)):
        rep = both_ways(ctx, hits, hidx, alns, str(kw), **kw)["report"]
        assert rep["samples"] == 330 and rep["ins_min"] <= rep["q25"] <= rep["mean"] <= rep["ins_max"]
        seen.add((rep["used"], rep["ins_min"], rep["ins_max"]))
        if kw.get("out_mult", 2) < 255:
            assert rep["used"] < rep["samples"]          # the outliers are left out
        else:
            assert rep["used"] == rep["samples"]
    assert len(seen) == 7
    # 30 at 200 and 10 at 5000 (tests/test_fm_insert_model.py works it by hand), then 31 and 9
    for n_low, n_high, q75 in ((30, 10, 5000), (31, 9, 200)):
        hits, hidx, alns = pm.batch_of(pairs_of_lengths([200] * n_low + [5000] * n_high, rng))
        rep = both_ways(ctx, hits, hidx, alns, "%d + %d" % (n_low, n_high))["report"]
        assert rep["q75"] == q75 and rep["used"] == (40 if q75 == 5000 else 31)


def test_the_host_entry_equals_the_device_entry_and_the_model(ctx):
    import kiss_amd
    rng = np.random.default_rng(9)
    hits, hidx, alns = batch(rng, 700, centre=450)
    c = Call(ctx, hits, hidx, alns).check("700 pairs")
    res = kiss_amd.estimate_insert(np.array(hits, np.int64).reshape(-1, 8), hidx, np.array(alns, np.int64).reshape(-1, 12))
    assert {k: res["report"][k] for k in im.REPORT_COUNTS} == c.want["report"] and np.array_equal(res["hist"], c.want["hist"])
    assert res["stats"] == {k: c.want["report"][k] for k in kiss_amd.fm_insert.INSERT_STATS}
    assert res["report"]["ms_total"] > 0 and c.rep.ms_hist > 0 and c.rep.ms_stats > 0 and c.rep.ms_total >= c.rep.ms_hist
    assert c.want["report"]["flags"] == im.OK and c.want["report"]["samples"] > 50
    empty = kiss_amd.estimate_insert(np.zeros((0, 8), np.int64), [0], np.zeros((0, 12), np.int64), max_insert=50)
    assert empty["hist"].shape == (51,) and not empty["hist"].any() and not any(empty["stats"].values())
    no_hits = kiss_amd.estimate_insert(np.zeros((0, 8), np.int64), [0] * 7, np.zeros((0, 12), np.int64))
    assert no_hits["report"]["unmapped"] == no_hits["report"]["P"] == 3 and no_hits["report"]["flags"] == 0


# ---- (b) the error contract ----------------------------------------------------------------------------------------------------------
def test_error_contract_of_the_device_call(ctx):
    from kiss_amd import _lib
    rng = np.random.default_rng(10)
    hits, hidx, alns = pm.batch_of(pairs_of_lengths([int(x) for x in rng.integers(300, 500, 6)], rng))
    ok = im.estimate(hits, hidx, alns, min_samples=1)
    Call(ctx, hits, hidx, alns, want=ok, min_samples=1).check("in order")
    for k in ("hits", "hidx", "alns", "report"):
        c = Call(ctx, hits, hidx, alns, want=ok, run=False).run(null=(k,))
        assert c.rc == _lib.KISS_HIP_E_INVALID, k
        c.untouched()
    c = Call(ctx, hits, hidx, alns, want=ok, run=False).run(params=False)
    assert c.rc == _lib.KISS_HIP_E_INVALID
    c.untouched()
    c = Call(ctx, hits, hidx[:-1], alns, want=ok, run=False).run()          # Q odd
    assert c.rc == _lib.KISS_HIP_E_INVALID
    c.untouched()
    for kw in (dict(max_insert=0), dict(max_insert=65536), dict(out_mult=256), dict(map_mult=256), dict(sd_mult=256)):
        c = Call(ctx, hits, hidx, alns, want=ok, run=False)
        for k, v in kw.items():
            setattr(c.p, k, v)
        assert c.run().rc == _lib.KISS_HIP_E_INVALID, kw
        c.untouched()
    # a hit_index that decreases -- inside a pair, between two pairs, and past the hits there are: no hit outside the array is read
    for bad in (hidx[:5] + [hidx[5] - 2] + hidx[6:], [hidx[0] + 5] + hidx[1:], hidx[:6] + [hidx[6] + 50, hidx[7] + 50] + hidx[8:],
                hidx[:-1] + [hidx[-1] - 3]):
        assert any(y < x for x, y in zip(bad, bad[1:]))
        c = Call(ctx, hits, bad, alns, want=ok, run=False).run()
        assert c.rc == _lib.KISS_HIP_E_INVALID, bad
        dev_place.check_canaries(*c.ins.values(), *c.outs.values())
    # hit_index[Q] of 2^32 - 1 or more
    c = Call(ctx, [], [0, 0, 0xFFFFFFFF], [], want=ok, run=False).run()
    assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED
    # no pairs: the histogram is all zero
    c = Call(ctx, [], [0], [], max_insert=77).check("Q = 0")
    assert not c.fetch().any() and c.rep.flags == 0
    # the ctx is as good as before
    Call(ctx, hits, hidx, alns, want=ok, min_samples=1).check("after the refusals")


# ---- (c) the caller's stream ---------------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(ctx):
    """tests/test_dev_stream_gpu.py's method: after a warm-up on the NULL stream the alignment records are overwritten with a
    decoy (every interval 37 bases longer: other bins, other statistics); a delay and then the copy that puts the real records
    back are queued on s; the call is made with s while s is busy; on return the histogram is read by a blocking copy on the
    null stream."""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    rng = np.random.default_rng(11)
    hits, hidx, alns = batch(rng, 3000, centre=500)
    c = Call(ctx, hits, hidx, alns)
    decoy = np.asarray(alns, np.int64).reshape(-1, 12).copy()
    decoy[:, 5] += 37
    other = im.estimate(hits, hidx, decoy)
    assert other["report"]["mean"] != c.want["report"]["mean"] and not np.array_equal(other["hist"], c.want["hist"])
    s = caller_stream()
    for _ in range(2):  # 1. warm up on the NULL stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(None)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    c.check("warm-up on the NULL stream")
    staging = c.ins["alns"].clone()
    c.ins["alns"].copy_(torch.from_numpy(decoy.astype(np.uint32).reshape(-1).view(np.uint8)))  # 2. the decoy
    c.outs["hist"].fill_(INIT)
    torch.cuda.synchronize()
    before = ctx.workspace_bytes()
    with Delayed(s, idle_ms) as delay:  # 3. a delay on s, and behind it the real input
        c.ins["alns"].copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.run(vp(s.cuda_stream))  # 4. the call, while s is busy
    got = c.fetch()  # 5. no torch synchronisation
    after = ctx.workspace_bytes()
    delay.check("kiss_hip_fmi_insert_dev")
    assert after == before, "the timed call allocated work arrays (%d -> %d bytes)" % (before, after)
    assert np.array_equal(got, c.want["hist"])
    c.check("on the caller's stream")


# ---- (d) FMIndex.map_pairs(insert=...) -----------------------------------------------------------------------------------------------
def same_results(a, b, path=""):
    """key for key; the times of the reports aside"""
    assert a.keys() == b.keys(), (path, sorted(a.keys() ^ b.keys()))
    for k in a:
        if isinstance(a[k], dict):
            same_results(a[k], b[k], path + k + ".")
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), path + k
        elif not k.startswith("ms_"):
            assert a[k] == b[k], path + k


def check_insert(res, hits, hidx, alns, caller, **insert):
    """res["insert"] against the model on the given hits -> the pair parameters that were used"""
    ins = res["insert"]
    want = im.estimate(hits, hidx, alns, **insert)
    assert {k: ins["report"][k] for k in im.REPORT_COUNTS} == want["report"]
    assert np.array_equal(ins["hist"], want["hist"]) and ins["hist"].dtype == np.uint32
    assert ins["applied"] == bool(want["report"]["flags"] & im.OK)
    used = dict(caller)
    if ins["applied"]:
        used.update({k: want["report"][k] for k in ("ins_min", "ins_max", "ins_mean")})
    assert {k: ins[k] for k in ("ins_min", "ins_max", "ins_mean")} == {k: used.get(k, pm.DEFAULTS[k]) for k in ("ins_min", "ins_max", "ins_mean")}
    return used


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_insert_equals_the_models_on_the_hits_of_the_device(name):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import PAIR_SETS, check as check_pairs, mates_of
    f = index_of(name, 4)
    S = text(name)
    m1, m2 = mates_of(name)
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20))
    applied = 0
    for params in PAIR_SETS:
        plain = f.map_pairs(m1, m2, S, 15, 0, 200, **common, **params)
        assert "insert" not in plain
        same_results(plain, f.map_pairs(m1, m2, S, 15, 0, 200, insert=None, **common, **params))
        for insert in ("auto", True, dict(min_samples=1, min_mapq=0, max_insert=3000)):
            res = f.map_pairs(m1, m2, S, 15, 0, 200, insert=insert, **common, **params)
            assert res.keys() == plain.keys() | {"insert"}
            used = check_insert(res, res["hits"], res["hit_index"], res["alignments"], params, **(insert if isinstance(insert, dict) else {}))
            check_pairs(res, pm.pair(res["hits"], res["hit_index"], res["alignments"], **used), key="pair_report")
            if res["insert"]["applied"]:
                applied += 1
                same_results({k: v for k, v in res.items() if k not in ("pairs", "pair_report", "insert")},
                             {k: v for k, v in plain.items() if k not in ("pairs", "pair_report")})
            else:
                res.pop("insert")
                same_results(res, plain)
    if name in ("genome", "iid"):
        assert applied >= 2
    with pytest.raises(TypeError):
        f.map_pairs(m1, m2, S, insert=dict(ins_max=3))
    with pytest.raises(ValueError):
        f.map_pairs(m1, m2, S, insert=dict(max_insert=0))


TRUTH_SEED = 417


def revcomp(R):
    return (3 - np.asarray(R, np.uint8)[::-1]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def insert_truth_case(pairs=200, damaged=0):
    """a random text of 60 000 bases; `pairs` pairs of unmutated 100-base mates, fragments drawn from rng.integers(1400, 1601),
    orientation alternating; behind them `damaged` pairs of the same library one mate of which carries a substitution every
    12th base (no seed: tests/test_fm_rescue_gpu.py), the reverse mate in even pairs -> text, mates 1, mates 2, [(start,
    fragment length)]"""
    rng = np.random.default_rng(TRUTH_SEED)
    S = rng.integers(0, 4, 60000, dtype=np.uint8)
    m1, m2, truth = [], [], []
    for p in range(pairs + damaged):
        frag = int(rng.integers(1400, 1601))
        a = int(rng.integers(0, S.size - frag))
        fwd, rev = S[a:a + 100].copy(), S[a + frag - 100:a + frag].copy()
        if p >= pairs:
            hurt = rev if p % 2 == 0 else fwd
            for j in range(5, 100, 12):
                hurt[j] = (hurt[j] + 1 + rng.integers(0, 3)) & 3
        x, y = (fwd, revcomp(rev)) if p % 2 == 0 else (revcomp(rev), fwd)
        m1.append(x), m2.append(y), truth.append((a, frag))
    return S, m1, m2, truth


def assert_insert_truth(plain_pairs, pairs, insert, truth):
    """the conditions of the issue.  plain_pairs / pairs: rows of PAIR_FIELDS with the defaults and with the estimate; insert:
    dict(report, hist)"""
    frags = [t[1] for t in truth]
    assert not (np.asarray(plain_pairs)[:, 2] & pm.PROPER).any()                     # with the defaults no pair is proper
    for p, (a, frag) in enumerate(truth):
        r = dict(zip(pm.PAIR_FIELDS, (int(v) for v in pairs[p])))
        assert r["flags"] & pm.PROPER and r["tlen"] == frag, (p, r, frag)             # with the estimate every pair is
    assert np.array_equal(insert["hist"], np.bincount(frags, minlength=10001))
    want = im.of_lengths(frags)["report"]
    assert {k: insert["report"][k] for k in im.REPORT_COUNTS} == want and want["flags"] == im.OK
    assert want["ins_min"] <= 1400 and 1600 <= want["ins_max"] <= 3000 and 1480 <= want["mean"] <= 1520


def truth_index(S):
    import kiss_amd
    import kiss_amd.fm_index as fm
    with kiss_amd.Context(max_n=1 << 20) as c:
        sa = c.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    return fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)


def test_against_the_truth_a_library_of_1500_bases_pairs_only_with_the_estimate():
    """200 pairs of a library of 1400 .. 1600 bases: with the default parameters no pair is proper; with insert="auto" every
    pair is, with TLEN equal to its fragment length, the histogram is np.bincount of the fragment lengths and the statistics
    are the model's on those lengths.  The conditions hold on this seed in the composed CPU models:
    tests/test_fm_insert_truth_model.py.  With 24 pairs there are too few samples: nothing is applied and every other key is
    what map_pairs gives without the option."""
    from tests.test_fm_rescue_gpu import rows
    S, m1, m2, truth = insert_truth_case()
    f = truth_index(S)
    plain = f.map_pairs(m1, m2, S)
    res = f.map_pairs(m1, m2, S, insert="auto")
    few_plain = f.map_pairs(m1[:24], m2[:24], S)
    few = f.map_pairs(m1[:24], m2[:24], S, insert="auto")
    f.close()
    assert plain["pair_report"]["proper"] == 0 and res["pair_report"]["proper"] == 200 and res["insert"]["applied"]
    assert_insert_truth(rows(plain["pairs"], pm.PAIR_FIELDS), rows(res["pairs"], pm.PAIR_FIELDS), res["insert"], truth)
    used = check_insert(res, res["hits"], res["hit_index"], res["alignments"], {})
    assert used["ins_max"] >= 1600
    # too few samples
    ins = few.pop("insert")
    assert ins["applied"] is False and ins["report"]["samples"] == 24 and ins["report"]["flags"] == 0 and ins["report"]["mean"] == 0
    assert (ins["ins_min"], ins["ins_max"], ins["ins_mean"]) == (0, 1000, 400) and int(ins["hist"].sum()) == 24
    same_results(few, few_plain)
    assert few["pair_report"]["proper"] == 0


def test_with_rescue_the_plan_uses_the_estimated_bounds():
    """the 200 pairs and 10 more with a mate that has no seed: the estimate comes from the 200, the windows of the 10 lie where
    the estimated bounds put them (the rescue model on the first pass with those bounds), and all 210 pairs are proper -- with
    the default bounds a window ends 1000 bases from the partner's start and holds no mate of this library.  Explicit bounds
    in the rescue dict still win."""
    from tests import fm_rescue_model as rm
    from tests.test_fm_rescue_gpu import check_plan, rows
    S, m1, m2, truth = insert_truth_case(200, 10)
    lens = [100] * 420
    f = truth_index(S)
    res = f.map_pairs(m1, m2, S, rescue=True, insert="auto")
    wide = f.map_pairs(m1, m2, S, rescue=dict(ins_min=0, ins_max=2000), insert="auto")
    f.close()
    first = res["first_pass"]
    used = check_insert(res, first["hits"], first["hit_index"], res["alignments"][res["aln_source"] < first["alignments"]], {})
    assert res["insert"]["applied"] and res["insert"]["report"]["samples"] == 200 and res["insert"]["report"]["unmapped"] == 10
    assert first["pair_report"]["proper"] == 200 and res["pair_report"]["proper"] == 210 and res["rescue"]["rescued"] == 10
    alns1 = res["alignments"][res["aln_source"] < first["alignments"]]
    want = rm.plan(first["pairs"], first["hits"], first["hit_index"], alns1, lens, S.size, ins_min=used["ins_min"], ins_max=used["ins_max"])
    check_plan(res["rescue"], want)
    assert want["report"]["pairs_planned"] == 10 and want["report"]["chains"] >= 10
    p2 = rows(res["pairs"], pm.PAIR_FIELDS)
    for p, (a, frag) in enumerate(truth):
        assert p2[p, 2] & pm.PROPER and abs(int(p2[p, 3]) - frag) <= 5, (p, p2[p], frag)
    # both passes used the same values
    assert np.array_equal(p2, pm.pair(res["hits"], res["hit_index"], res["alignments"], **used)["pairs"])
    # explicit bounds win
    want = rm.plan(first["pairs"], first["hits"], first["hit_index"], alns1, lens, S.size, ins_min=0, ins_max=2000)
    check_plan(wide["rescue"], want)
    assert {k: wide["insert"][k] for k in used} == used and wide["first_pass"]["pairs"].tobytes() == first["pairs"].tobytes()
