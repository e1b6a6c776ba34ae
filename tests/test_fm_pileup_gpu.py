"""kiss_hip_fmi_pileup_dev on the GPU against tests/fm_pileup_model.py: every word of counts and every count of the report.
(a) records and op lists built by hand (the Batch of tests/test_fm_md_gpu.py), on arrays placed with tests/dev_place.py: text
and reads at an odd address, counts at 4, 8 and 12 bytes past a multiple of 16, guard bytes around each; (b) contention and
scale; (c) the window at every interesting place; (d) accumulate; (e) bad, filtered and unmapped items in the three modes;
(f) the error contract: counts untouched; (g) the caller's stream; (h) the host entry.  Texts of at most 2^20 bases."""
import ctypes

import numpy as np
import pytest

from tests import dev_place
from tests import fm_align_model as am
from tests import fm_pileup_model as pm
from tests.test_fm_md_gpu import Batch, D, I, M, hand_batch
from tests.test_fm_pileup_model import random_batch

pytestmark = pytest.mark.gpu
GUARD = 512
vp = ctypes.c_void_p
NAMES = ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "hits", "pairs", "counts")


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=1 << 20, device=0)
    yield c
    c.close()


def device():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def S():
    return np.random.default_rng(41).integers(0, 4, 260_000).astype(np.uint8)


def hit_rows(alns, flags=0, mapq=30):
    """hits naming the alignments `alns`: (H, 8), every field that is not read holds a pattern"""
    alns = np.asarray(alns, np.int64).ravel()
    rec = np.full((alns.size, 8), 0xDEADBEEF, np.uint32)
    rec[:, 0] = alns
    rec[:, 1] = flags
    rec[:, 2] = mapq
    return rec


def pair_rows(rows):
    """rows of (hit1, hit2, flags, mapq1, mapq2) -> (P, 10)"""
    rec = np.full((len(rows), 10), 0xDEADBEEF, np.uint32)
    for k, (h1, h2, fl, q1, q2) in enumerate(rows):
        rec[k, 0], rec[k, 1], rec[k, 2], rec[k, 7], rec[k, 8] = h1, h2, fl, q1, q2
    return rec


class Call:
    """one kiss_hip_fmi_pileup_dev call on placed arrays.  a: the arrays of Batch.arrays() (or of as_arrays()); start: what
    counts holds before the call ((8, W) u32; None: 0xEE bytes, and accumulate = 0)"""

    def __init__(self, ctx, a, hits=None, pairs=None, lo=0, hi=None, start=None, accumulate=None, byte_leads=(1, 3), counts_lead=4, fill=0x5A,
                 run=True, want=None, params=None):
        from kiss_amd import _lib
        self.lib, self.ctx, dev = ctx._lib, ctx, device()
        self.a, self.hits, self.pairs = a, hits, pairs
        self.lo, self.hi = lo, a["text"].size if hi is None else hi
        W = self.hi - self.lo
        self.params = dict(params or {})
        self.start = np.full((8, max(W, 0)), 0xEEEEEEEE, np.uint32) if start is None else np.asarray(start, np.uint32).reshape(8, W)
        self.accumulate = (start is not None) if accumulate is None else accumulate
        if want is None:
            want = pm.pileup(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], a["both"], hits=hits, pairs=pairs, lo=self.lo,
                             hi=self.hi, counts=self.start if self.accumulate else None, **self.params)
        self.want = want
        put = lambda arr, lead: dev_place.place(arr, lead, GUARD, fill, device=dev)  # noqa: E731
        self.ins = {"text": put(a["text"], byte_leads[0]), "reads": put(a["reads"], byte_leads[1]), "ridx": put(a["ridx"], 8),
                    "alns": put(a["alns"], 4), "cidx": put(a["cidx"], 8), "cigar": put(a["cigar"], 4), "oidx": put(a["oidx"], 8)}
        if hits is not None:
            self.ins["hits"] = put(np.asarray(hits, np.uint32).reshape(-1, 8), 4)
        if pairs is not None:
            self.ins["pairs"] = put(np.asarray(pairs, np.uint32).reshape(-1, 10), 4)
        self.outs = {"counts": put(self.start, counts_lead)}
        self.par = _lib.PileupParams(*[pm.params_of(**self.params)[k] for k in ("min_mapq", "skip_flags", "proper_only")], 0)
        self.rep = _lib.PileupReport()
        if run:
            self.run()

    def address(self, name):
        v = self.ins.get(name, self.outs.get(name))
        return vp(v.placement.address) if v is not None else None

    def run(self, stream=None, null=(), n=None, lo=None, hi=None, par=None, no_params=False):
        a = self.a
        p = {k: (None if k in null else self.address(k)) for k in NAMES}
        par = self.par if par is None else par
        self.rc = self.lib.kiss_hip_fmi_pileup_dev(
            self.ctx._ctx, p["text"], a["text"].size if n is None else n, p["reads"], p["ridx"], a["ridx"].size - 1, 1 if a["both"] else 0, p["alns"],
            p["cidx"], p["cigar"], p["oidx"], p["hits"], 0 if self.hits is None else len(self.hits), p["pairs"],
            0 if self.pairs is None else len(self.pairs), None if no_params else ctypes.byref(par), self.lo if lo is None else lo,
            self.hi if hi is None else hi, p["counts"], 1 if self.accumulate else 0, ctypes.byref(self.rep), stream)
        return self

    def fetch(self):
        """through kiss_hip_copy_to_host: a blocking copy on the null stream, no torch call"""
        out = np.empty(self.outs["counts"].numel(), np.uint8)
        if out.size:
            assert self.lib.kiss_hip_copy_to_host(vp(out.ctypes.data), self.address("counts"), out.size) == 0
        return out.view(np.uint32).reshape(8, self.hi - self.lo)

    def untouched(self, what=""):
        assert np.array_equal(self.fetch(), self.start), what + ": counts was written"
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())

    def check(self, what=""):
        w = self.want
        assert self.rc == 0, (what, self.rc)
        for k in pm.COUNTS:
            print("PILEUP %-44s %-14s %d (model %d)" % (what, k, getattr(self.rep, k), w[k]))
            assert getattr(self.rep, k) == w[k], (what, k)
        got = self.fetch()
        if not np.array_equal(got, w["counts"]):
            k, j = np.argwhere(got != w["counts"])[0]
            raise AssertionError("%s: plane %s, position %d: %d, model %d (%d words differ)"
                                 % (what, pm.PLANES[k], self.lo + j, got[k, j], w["counts"][k, j], int((got != w["counts"]).sum())))
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())
        return self


def full_batch(S, both):
    """the shapes of the MD test -- M ops of 1 / 63 / 64 / 65 / 129 / 300 columns with differing bases at column 0 / 63 / 64 /
    last, D ops of 1 .. 200, D-I-D and I-D, 1000 ops of one base, no-bases, tend = n, reverse strands -- and a few more"""
    b = hand_batch(S, both)
    b.add(0, [(I, 3), (M, 70)], mism=(1,))                   # an insertion first, at j = 0: no position in front
    b.add(20000, [(I, 2), (M, 64), (I, 1), (M, 64), (I, 5)])  # ... first and last elsewhere
    for ln in (2, 7, 100, 128, 199):
        b.add(21000 + 400 * ln % 3000, [(M, 3), (D, ln), (M, 3)])
    b.add(25000, [(M, 100), (D, 10), (M, 50), (I, 3), (M, 50)], mism=(0, 99, 100, 149, 150, 199), no_base=(120,))  # (the window test)
    return b


@pytest.mark.parametrize("leads", [(1, 3, 4), (3, 1, 8), (2, 5, 12)])
@pytest.mark.parametrize("both", (False, True))
def test_shapes_by_hand(ctx, S, both, leads):
    a, number = full_batch(S, both).arrays()
    c = Call(ctx, a, byte_leads=leads[:2], counts_lead=leads[2]).check("all alignments")
    w = c.want
    assert w["bad"] == 0 and w["items"] == number.size == w["counted"] and w["clipped"] == 0
    assert w["alt_columns"] > 100 and w["deleted_bases"] > 1000 and w["insertions"] > 500 and int(w["counts"][pm.ALT_N].sum()) >= 4
    C = number.size
    # hits: descending, one alignment twice; the default skips the secondary ones
    order = list(range(C - 1, -1, -1)) + [3, 3, 0, C - 1]
    hits = hit_rows(order, flags=[2 if k % 5 == 0 else k % 2 for k in range(len(order))])
    c = Call(ctx, a, hits=hits, byte_leads=leads[:2], counts_lead=leads[2]).check("hits in descending order")
    assert c.want["filtered"] == len(range(0, len(order), 5))
    Call(ctx, a, hits=np.zeros((0, 8), np.uint32), counts_lead=leads[2]).check("no hits")


def test_random_batches_in_the_three_modes(ctx):
    seen = dict.fromkeys(pm.COUNTS, 0)
    for seed in range(45):
        b = random_batch(seed)
        a = dict(text=b["text"], reads=np.concatenate(b["reads"]), read_list=b["reads"], both=b["both"], alns=b["alns"], cidx=b["cidx"],
                 cigar=b["cigar"], oidx=b["oidx"], ridx=np.concatenate([[0], np.cumsum([r.size for r in b["reads"]])]).astype(np.uint64))
        hits = None if b["mode"] == "alignments" else b["hits"]
        pairs = b["pairs"] if b["mode"] == "pairs" else None
        if b["hi"] == b["lo"]:
            continue  # (an empty window has its own test)
        start = np.random.default_rng(seed).integers(0, 1 << 32, (8, b["hi"] - b["lo"])).astype(np.uint32) if seed % 2 else None
        c = Call(ctx, a, hits=hits, pairs=pairs, lo=b["lo"], hi=b["hi"], start=start, params=b["params"]).check("seed %d %s" % (seed, b["mode"]))
        for k in pm.COUNTS:
            seen[k] += c.want[k]
    assert all(seen.values()), seen


# ---- contention and scale ----------------------------------------------------------------------------------------------------------
def test_ten_thousand_items_on_one_position(ctx, S):
    b = Batch(S, False, seed=21)
    at = 70_000
    for k in range(10_000):
        b.add(at - k % 24, [(M, 24)], mism=(k % 24,) if k % 4 == 0 else ())  # (column k % 24 lies on `at`)
    a, _ = b.arrays()
    c = Call(ctx, a, lo=at - 40, hi=at + 40).check("10^4 items on one position")
    assert c.want["counts"][pm.COV][40] == 10_000 and c.want["counts"][pm.ALT_A:pm.ALT_T + 1, 40].sum() == 2_500


def test_one_long_read_beside_ten_thousand_light_items(ctx, S):
    b = Batch(S, False, seed=5)
    L = 222_232
    b.add(100, [(M, L)], mism=(0, 63, 64, 9999, L - 1))
    rng = np.random.default_rng(9)
    for k in range(10_000):
        b.add(int(rng.integers(0, S.size - 40)), [(M, 12), (D, 1), (M, 12)] if k % 7 == 0 else [(M, 24)], mism=(k % 24,) if k % 3 else ())
    a, _ = b.arrays()
    c = Call(ctx, a).check("long and light")
    assert c.want["columns"] == L + 24 * 10_000 and c.want["counts"][pm.COV].min() == 0 and c.want["counts"][pm.COV][100:100 + L].min() >= 1


# ---- the window --------------------------------------------------------------------------------------------------------------------
def test_the_window_at_every_interesting_place(ctx, S):
    a, number = full_batch(S, True).arrays()
    n = S.size
    # the last item of full_batch: M 100 at 25000, D 10 at 25100, M 50 at 25110, I 3 counted at 25159, M 50 at 25160 .. 25210
    places = {"lo inside an M": (25050, 26000), "hi inside an M": (24000, 25050), "lo inside a D": (25105, 26000),
              "hi inside a D": (24000, 25105), "lo on an op boundary": (25100, 26000), "hi on an op boundary": (24000, 25110),
              "lo on the position of an I": (25159, 26000), "lo behind it": (25160, 26000), "hi on it": (24000, 25159),
              "hi behind it": (24000, 25160), "one position": (25159, 25160), "no item inside": (100_000, 100_100),
              "hi = n": (n - 150, n), "lo = 0": (0, 80), "the whole text": (0, n)}
    clipped = {}
    for what, (lo, hi) in places.items():
        c = Call(ctx, a, lo=lo, hi=hi).check(what)
        clipped[what] = c.want["clipped"]
        assert c.want["counted"] == number.size
    total = clipped["no item inside"]
    assert clipped["the whole text"] == 0 and total > 0 and 0 < clipped["hi = n"] < total and clipped["one position"] == total - 3
    # W = 0: counts may be NULL; everything is clipped
    for at in (0, 25100, n):
        c = Call(ctx, a, lo=at, hi=at, run=False).run(null=("counts",)).check("W = 0 at %d" % at)
        assert c.want["clipped"] == total and c.want["counts"].shape == (8, 0)


# ---- accumulate --------------------------------------------------------------------------------------------------------------------
def test_accumulate(ctx, S):
    a, _ = full_batch(S, True).arrays()
    lo, hi = 900, 27000
    W = hi - lo
    once = Call(ctx, a, lo=lo, hi=hi, start=np.full((8, W), 0xFFFFFFFF, np.uint32), accumulate=False).check("onto 0xFF bytes, accumulate = 0")
    assert once.want["counts"].max() < 100
    start = np.random.default_rng(3).integers(0, 1000, (8, W)).astype(np.uint32)
    start[pm.COV, 25000 - lo] = 0xFFFFFFFF  # one add wraps it to 0
    c = Call(ctx, a, lo=lo, hi=hi, start=start).check("accumulate = 1")
    assert c.want["counts"][pm.COV, 25000 - lo] == 0
    c.run()  # a second time onto the sums
    assert c.rc == 0 and np.array_equal(c.fetch(), start + once.want["counts"] + once.want["counts"])
    # zero items, accumulate = 0: zeroed all the same
    none = Batch(S, True)
    none.reads.append(np.array([1, 2], np.uint8))
    a0, _ = none.arrays()
    c = Call(ctx, a0, lo=5, hi=50, accumulate=False).check("no items")
    assert c.want["items"] == 0 and not c.fetch().any()
    c = Call(ctx, a0, lo=5, hi=50, start=np.full((8, 45), 7, np.uint32)).check("no items, accumulate = 1")
    assert (c.fetch() == 7).all()


# ---- bad, filtered and unmapped items ----------------------------------------------------------------------------------------------
def bad_batch(S):
    b = Batch(S, True, seed=6)
    good = [b.add(1000, [(M, 100)], mism=(50,)), b.add(2000, [(M, 50), (D, 3), (M, 50)], rev=True)]
    L, n = 100, S.size
    ok = [1, 0, 0, L, 1000, 1000 + L, 0, 0, 0, 0, 0, 0]

    def rec(**kw):
        r = list(ok)
        for k, v in kw.items():
            r[am.FIELDS.index(k)] = v
        return r

    bad = [b.more(0, False, ok, [(3, L)]),                                  # an op code above 2
           b.more(0, False, ok, [(M, 50), (15, 1), (M, 49)]),
           b.more(0, False, ok, [(M, 60), (I, 0), (M, 40)]),                 # a length of 0
           b.more(0, False, rec(rend=L - 1), [(M, L)]),                      # the read lengths do not add up
           b.more(0, False, ok, [(M, L - 1), (D, 1)]),
           b.more(0, False, rec(tend=1000 + L + 1), [(M, L)]),               # the text lengths do not add up
           b.more(0, False, ok, [(M, L - 1), (I, 1)]),
           b.more(0, False, rec(rbeg=1, rend=L + 1), [(M, L)]),              # rend > L
           b.more(0, False, rec(rbeg=0xFFFFFF00, rend=0xFFFFFF00 + L), [(M, L)]),
           b.more(0, False, rec(tbeg=n - 50, tend=n + 50), [(M, L)]),        # tend > n
           b.more(0, False, rec(tbeg=0xFFFFFF00, tend=0xFFFFFF00 + L), [(M, L)]),
           b.more(0, False, rec(rbeg=L, rend=0), [(M, L)]),                  # rbeg > rend
           b.more(0, False, rec(tbeg=1000 + L, tend=1000), [(M, L)]),        # tbeg > tend
           b.more(1, True, rec(rend=103 + 1, tbeg=2000, tend=2000 + 104), [(M, 104)])]  # rend > L on the reverse strand
    good.append(b.more(0, False, rec(rbeg=10, tbeg=1010), [(M, 90)]))        # the same read, further in
    good.append(b.more(0, False, [0] * 12, []))                              # no ops: counted, adds nothing
    return b, good, bad


def test_bad_items_beside_good_ones(ctx, S):
    b, good, bad = bad_batch(S)
    a, number = b.arrays()
    c = Call(ctx, a, lo=500, hi=3000).check("one of every kind")
    assert c.want["bad"] == len(bad) and c.want["counted"] == len(good) and c.want["columns"] == 100 + 100 + 90
    C = number.size
    hits = hit_rows([number[good[0]], C, number[bad[0]], 0xFFFFFFFF, number[good[1]], C + 1, number[good[2]]])
    c = Call(ctx, a, hits=hits, lo=500, hi=3000).check("aln out of range")
    assert c.want["bad"] == 4 and c.want["counted"] == 3


def test_min_mapq_and_every_bit_of_skip_flags(ctx, S):
    b, good, bad = bad_batch(S)
    a, number = b.arrays()
    g = [int(number[k]) for k in good[:3]]
    m = 20
    hits = hit_rows(g * 3 + [int(number[bad[0]])], mapq=[m - 1] * 3 + [m] * 3 + [m + 1] * 3 + [0], flags=[0, 1, 2, 4, 3, 5, 6, 7, 0, 0])
    for q, kept in ((m - 1, 9), (m, 6), (m + 1, 3), (0, 10), (255, 0)):
        c = Call(ctx, a, hits=hits, lo=500, hi=3000, params=dict(min_mapq=q, skip_flags=0)).check("min_mapq %d" % q)
        assert c.want["filtered"] == 10 - kept and c.want["bad"] == (1 if q == 0 else 0)  # (a filtered item's alignment is not looked at)
    for bit, dropped in ((1, 4), (2, 4), (4, 4), (7, 7), (0, 0)):
        c = Call(ctx, a, hits=hits, lo=500, hi=3000, params=dict(skip_flags=bit)).check("skip_flags %d" % bit)
        assert c.want["filtered"] == dropped
    assert Call(ctx, a, hits=hits, lo=500, hi=3000).check("the defaults").want["filtered"] == 4
    # without hits there is no filter: the params are checked and otherwise ignored
    c = Call(ctx, a, lo=500, hi=3000, params=dict(min_mapq=255, skip_flags=7, proper_only=1)).check("alignments mode ignores the filter")
    assert c.want["filtered"] == 0 and c.want["counted"] == len(good)


def test_pair_mode(ctx, S):
    b, good, bad = bad_batch(S)
    a, number = b.arrays()
    g = [int(number[k]) for k in good[:3]]
    # hit 3 is secondary in the select call's eyes: a pair that promoted it makes it the mate's primary line
    hits = hit_rows(g + [g[0], int(number[bad[3]]), number.size + 9], flags=[0, 1, 0, 2, 0, 0], mapq=[30, 30, 30, 0, 30, 30])
    H = hits.shape[0]
    NONE = 0xFFFFFFFF
    rows = [(0, 1, 1, 40, 41),            # proper, both counted
            (3, 2, 1 | 16, 25, 26),       # PROMOTED1: hit 3 counts although the hit is SECONDARY with MAPQ 0
            (0, NONE, 2, 30, 0),          # mate 2 unmapped
            (NONE, NONE, 0, 0, 0),
            (0, 1, 64, 30, 30),           # BAD_INPUT: both bad, whatever the rest holds
            (H, 1, 0, 30, 30),            # a hit index of H
            (4, 5, 1, 30, 30),            # a bad alignment; an aln past C
            (1, 2, 0, 10, 50)]            # not proper
    pairs = pair_rows(rows)
    c = Call(ctx, a, hits=hits, pairs=pairs, lo=500, hi=3000).check("pairs")
    assert [c.want[k] for k in ("items", "bad", "filtered", "unmapped", "counted")] == [16, 5, 0, 3, 8]
    c = Call(ctx, a, hits=hits, pairs=pairs, lo=500, hi=3000, params=dict(proper_only=1)).check("proper_only")
    assert [c.want[k] for k in ("bad", "filtered", "unmapped", "counted")] == [5, 4, 3, 4]
    c = Call(ctx, a, hits=hits, pairs=pairs, lo=500, hi=3000, params=dict(min_mapq=26, skip_flags=3)).check("pairs, filtered")
    assert c.want["filtered"] == 4 and c.want["counted"] == 4  # (hit 1 twice by REVERSE, mate 1 of pairs 1 and 7 by MAPQ)
    Call(ctx, a, hits=hits, pairs=np.zeros((0, 10), np.uint32), lo=500, hi=3000).check("no pairs")
    # pair mode on hit number 0 of every read with the hits' MAPQs is hits mode
    plain = hit_rows(g + g[:1], flags=[0, 1, 4, 0], mapq=[30, 5, 30, 7])
    same = pair_rows([(0, 1, 0, 30, 5), (2, 3, 0, 30, 7)])
    for par in (dict(), dict(min_mapq=6), dict(skip_flags=4)):
        x = Call(ctx, a, hits=plain, pairs=same, lo=500, hi=3000, params=par).check("as pairs")
        y = Call(ctx, a, hits=plain, lo=500, hi=3000, params=par).check("as hits")
        assert np.array_equal(x.fetch(), y.fetch()) and x.want["counted"] == y.want["counted"]


# ---- the error contract ------------------------------------------------------------------------------------------------------------
def test_error_returns_leave_counts_untouched(ctx, S):
    from kiss_amd import _lib
    a, number = full_batch(S, True).arrays()
    n = S.size
    hits = hit_rows(np.arange(number.size))
    pairs = pair_rows([(0, 1, 1, 30, 30)])
    whole = dict.fromkeys(pm.COUNTS, 0)  # (the model is not asked about calls that are refused)
    make = lambda **kw: Call(ctx, a, hits=hits, pairs=pairs, lo=100, hi=30000, run=False, want=whole, **kw)  # noqa: E731
    for k in ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "counts"):
        c = make().run(null=(k,))
        assert c.rc == _lib.KISS_HIP_E_INVALID, k
        c.untouched(k)
    cases = {"no params": dict(no_params=True), "pairs without hits": dict(null=("hits",)), "lo > hi": dict(lo=30001), "hi > n": dict(hi=n + 1),
             "reserved_": dict(par=_lib.PileupParams(0, 2, 0, 1)), "min_mapq 256": dict(par=_lib.PileupParams(256, 2, 0, 0)),
             "skip_flags 8": dict(par=_lib.PileupParams(0, 8, 0, 0))}
    for what, kw in cases.items():
        c = make().run(**kw)
        assert c.rc == _lib.KISS_HIP_E_INVALID, what
        c.untouched(what)
    assert make().run(n=_lib.MAX_N + 1).rc == _lib.KISS_HIP_E_UNSUPPORTED
    # an index that decreases, a read of length 0: nothing zeroed, nothing added (accumulate = 0 and 1)
    for name, at in (("cidx", 3), ("ridx", 2), ("oidx", 5)):
        broken = dict(a)
        broken[name] = a[name].copy()
        broken[name][at] = a[name][at + 1] + np.uint64(1)
        for start in (None, np.full((8, 29900), 5, np.uint32)):
            c = Call(ctx, broken, lo=100, hi=30000, want=whole, start=start)
            assert c.rc == _lib.KISS_HIP_E_INVALID, name
            c.untouched(name)
    empty = dict(a)
    empty["ridx"] = a["ridx"].copy()
    empty["ridx"][4] = empty["ridx"][3]
    c = Call(ctx, empty, lo=100, hi=30000, want=whole)
    assert c.rc == _lib.KISS_HIP_E_INVALID
    c.untouched("a read of length 0")
    assert make().run().rc == 0  # (and the same arrays are fine)


# ---- the caller's stream -----------------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(ctx, S):
    """tests/test_dev_stream_gpu.py's method: after a warm-up on the NULL stream the reads are overwritten with a decoy (other
    bases: other ALT counts); a delay and then the copy that puts the real reads back are queued on s; the call is made with s
    while s is busy; on return counts is read by a blocking copy on the null stream."""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    b = Batch(S, True, seed=12)
    rng = np.random.default_rng(13)
    for k in range(600):
        b.add(int(rng.integers(0, 30_000)), [(M, 70), (D, 2), (M, 78)] if k % 5 == 0 else [(M, 150)], mism=rng.integers(0, 148, 3), rev=bool(k % 2))
    a, _ = b.arrays()
    c = Call(ctx, a, lo=0, hi=31_000, accumulate=False)
    decoy = ((a["reads"].astype(np.int64) + 1) % 4).astype(np.uint8)
    s = caller_stream()
    for _ in range(2):  # 1. warm up on the NULL stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(None)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    c.check("warm-up on the NULL stream")
    staging = c.ins["reads"].clone()
    c.ins["reads"].copy_(torch.from_numpy(decoy))  # 2. the decoy; counts as before any call
    c.outs["counts"].fill_(0xEE)
    torch.cuda.synchronize()
    before = ctx.workspace_bytes()
    with Delayed(s, idle_ms) as delay:  # 3. a delay on s, and behind it the real input
        c.ins["reads"].copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.run(vp(s.cuda_stream))  # 4. the call, while s is busy
    got = c.fetch()  # 5. no torch synchronisation
    after = ctx.workspace_bytes()
    delay.check("kiss_hip_fmi_pileup_dev")
    assert after == before, "the timed call allocated work arrays (%d -> %d bytes)" % (before, after)
    assert np.array_equal(got, c.want["counts"])
    c.check("on the caller's stream")


# ---- the host entry and the Python entries -----------------------------------------------------------------------------------------
def test_the_host_entry_with_host_counts_and_with_counts_on_the_device(S):
    from kiss_amd import _lib, fm_pileup
    a, number = full_batch(S, True).arrays()
    args = (a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], True)
    hits = hit_rows(np.arange(number.size)[::-1], flags=[k % 3 for k in range(number.size)], mapq=[k % 40 for k in range(number.size)])
    want = pm.pileup(*args, hits=hits, lo=200, hi=26000, min_mapq=10)
    res = fm_pileup.pileup(a["text"], (a["reads"], a["ridx"]), a["alns"], a["cidx"], a["cigar"], a["oidx"], both_strands=True, hits=hits, lo=200,
                           hi=26000, min_mapq=10)
    assert res["counts"].dtype == np.uint32 and np.array_equal(res["counts"], want["counts"])
    for k in pm.COUNTS:
        assert res["report"][k] == want[k], k
    again = fm_pileup.pileup(*args[:6], both_strands=True, hits=hits, lo=200, hi=26000, min_mapq=10, counts=res["counts"])
    assert np.array_equal(again["counts"], want["counts"] * 2) and np.array_equal(res["counts"], want["counts"])
    pairs = pair_rows([(0, 1, 1, 30, 30), (2, 0xFFFFFFFF, 0, 5, 0)])
    want = pm.pileup(*args, hits=hits, pairs=pairs, proper_only=1)
    res = fm_pileup.pileup(*args[:6], both_strands=True, hits=hits, pairs=pairs, proper_only=1)
    assert np.array_equal(res["counts"], want["counts"]) and res["report"]["filtered"] == want["filtered"] == 1
    assert np.array_equal(fm_pileup.base_counts(res["counts"], a["text"]), pm.base_counts(want["counts"], a["text"]))
    assert fm_pileup.pileup(*args[:6], both_strands=True, lo=77, hi=77)["counts"].shape == (8, 0)
    # counts_on_device: two calls add into one device array, fetched once
    lib = _lib.load()
    lo, hi = 900, 26000
    W = hi - lo
    want = pm.pileup(*args, lo=lo, hi=hi)
    d = vp()
    assert lib.kiss_hip_alloc_dev(ctypes.byref(d), 32 * W) == 0
    try:
        par, rep = fm_pileup.pileup_params(), _lib.PileupReport()
        al = np.ascontiguousarray(a["alns"])
        for accumulate in (0, 1):
            rc = lib.kiss_hip_fmi_pileup_host(a["text"].ctypes.data, a["text"].size, a["reads"].ctypes.data, a["ridx"].ctypes.data, a["ridx"].size - 1,
                                              1, al.ctypes.data, a["cidx"].ctypes.data, a["cigar"].ctypes.data, a["oidx"].ctypes.data, None, 0,
                                              None, 0, ctypes.byref(par), lo, hi, d, 1, accumulate, ctypes.byref(rep), 0)
            assert rc == 0 and rep.columns == want["columns"] and rep.clipped == want["clipped"]
        got = np.empty((8, W), np.uint32)
        assert lib.kiss_hip_copy_to_host(vp(got.ctypes.data), d, 32 * W) == 0
        assert np.array_equal(got, want["counts"] * 2)
    finally:
        lib.kiss_hip_free_dev(d)
