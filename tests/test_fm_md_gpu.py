"""kiss_hip_fmi_md_dev on the GPU against tests/fm_md_model.py: every byte of md, md_index and md_counts and every count of the
report.  (a) records and op lists built by hand -- the call takes arrays from anywhere --, on arrays placed with
tests/dev_place.py: text, reads and md at an odd address, u32 arrays at 4, u64 arrays at 8, guard bytes around each; (b) bad
items beside good ones; (c) the capacity protocol and the error contract; (d) the caller's stream (the method of
tests/test_dev_stream_gpu.py); (e) FMIndex.map / map_pairs(want_md=True) on the texts of the FM tests: every string equals the
model's on the downloaded arrays, and the text under every hit rebuilt from the read, the ops and the string equals the text."""
import ctypes

import numpy as np
import pytest

from tests import dev_place
from tests import fm_align_model as am
from tests import fm_md_model as mm
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu
GUARD = 512
INIT = 0xEE
vp = ctypes.c_void_p
COUNTS = ("items", "bad", "md_bytes", "mismatch_columns", "deleted_bases", "longest")
M, I, D = 0, 1, 2


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


# ---- batches built by hand ---------------------------------------------------------------------------------------------------------
class Batch:
    """reads and alignments made from the text: add() lays ops over the text at tbeg and builds the read that they describe"""

    def __init__(self, S, both=False, seed=1, first=0):
        self.S, self.both, self.rng, self.first = S, both, np.random.default_rng(seed), first
        self.reads, self.alns = [], []  # alns: (v, record, op words)

    def add(self, tbeg, ops, mism=(), no_base=(), rev=False, pre=0, post=0):
        """a new read with one alignment.  mism / no_base: M columns (counted over the M ops) whose read base differs from the
        text / is a no-base; pre / post: clipped bases around the aligned part -> the number of the alignment"""
        S, rng = self.S, self.rng
        parts, j, col = [rng.integers(0, 4, pre)], tbeg, 0
        mism, no_base = np.asarray(mism, np.int64), np.asarray(no_base, np.int64)
        for op, ln in ops:
            if op == M:
                seg = S[j:j + ln].astype(np.int64)
                cols = np.arange(col, col + ln)
                seg = np.where(np.isin(cols, mism), (seg + 1 + cols % 3) % 4, seg)
                parts.append(np.where(np.isin(cols, no_base), 4, seg))
                j, col = j + ln, col + ln
            elif op == I:
                parts.append(rng.integers(0, 5, ln))  # (a no-base inside an insertion now and then)
            else:
                j += ln
        parts.append(rng.integers(0, 4, post))
        Rv = np.concatenate(parts).astype(np.uint8)
        assert self.both or not rev
        self.reads.append(am.virtual_read(Rv, rev))  # (the read as sequenced: the transform is its own inverse)
        q = len(self.reads) - 1
        rec = [1, 0, pre, Rv.size - post, tbeg, j, 0, 0, 0, 0, 0, 0]
        return self.more(q, rev, rec, ops)

    def more(self, q, rev, rec, ops):
        """one more alignment of read q, with any record and any op words"""
        words = [int(w) if not isinstance(w, tuple) else (w[1] << 4) | w[0] for w in ops]
        self.alns.append(((2 * q + int(rev)) if self.both else q, list(rec), words))
        return len(self.alns) - 1

    def arrays(self):
        """-> dict of the arrays of the call, and `number`: number[k] = where alignment k (in the order added) ended up"""
        V = (2 if self.both else 1) * len(self.reads)
        order = sorted(range(len(self.alns)), key=lambda k: self.alns[k][0])  # (stable: by virtual read)
        number = np.zeros(len(order), np.int64)
        number[order] = np.arange(len(order))
        per_v = np.bincount([a[0] for a in self.alns], minlength=V) if self.alns else np.zeros(V, np.int64)
        cidx = np.concatenate([[0], np.cumsum(per_v)]).astype(np.uint64) + np.uint64(self.first)
        alns = np.array([self.alns[k][1] for k in order], np.uint32).reshape(len(order), 12)
        cigar = np.array([w for k in order for w in self.alns[k][2]], np.uint32)
        oidx = np.concatenate([[0], np.cumsum([len(self.alns[k][2]) for k in order])]).astype(np.uint64)
        ridx = np.concatenate([[0], np.cumsum([r.size for r in self.reads])]).astype(np.uint64)
        cat = np.concatenate(self.reads) if self.reads else np.zeros(0, np.uint8)
        return dict(text=self.S, reads=cat, ridx=ridx, alns=alns, cidx=cidx, cigar=cigar, oidx=oidx, both=self.both, read_list=self.reads), number


class Call:
    """one kiss_hip_fmi_md_dev call on placed arrays"""

    def __init__(self, ctx, a, hits=None, capacity=None, items=None, byte_leads=(1, 3, 3), want_counts=True, fill=0x5A, run=True, want=None):
        from kiss_amd import _lib
        self.lib, self.ctx, dev = ctx._lib, ctx, device()
        self.a = a
        # (want: the model's answer for arrays the model is not asked about -- those the call refuses)
        self.want = want or mm.md(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], a["both"], hits)
        self.hits = None if hits is None else np.asarray(hits, np.int64)
        n_items = self.want["items"] if items is None else items
        cap = self.want["md_bytes"] if capacity is None else capacity
        put = lambda arr, lead: dev_place.place(arr, lead, GUARD, fill, device=dev)  # noqa: E731
        self.ins = {"text": put(a["text"], byte_leads[0]), "reads": put(a["reads"], byte_leads[1]), "ridx": put(a["ridx"], 8),
                    "alns": put(a["alns"], 4), "cidx": put(a["cidx"], 8), "cigar": put(a["cigar"], 4), "oidx": put(a["oidx"], 8)}
        if hits is not None:
            rec = np.full((self.hits.size, 8), 0xDEADBEEF, np.uint32)  # (no other field of a hit is read)
            rec[:, 0] = self.hits
            self.ins["hits"] = put(rec, 4)
        self.outs = {"md": dev_place.place_out(cap, byte_leads[2], GUARD, fill, device=dev),
                     "midx": dev_place.place_out(8 * (n_items + 1), 8, GUARD, fill, device=dev)}
        if want_counts:
            self.outs["counts"] = dev_place.place_out(8 * n_items, 4, GUARD, fill, device=dev)
        self.cap = cap
        self.rep = _lib.MdReport()
        if run:
            self.run()

    def address(self, name):
        v = self.ins.get(name, self.outs.get(name))
        return vp(v.placement.address) if v is not None else None

    def run(self, stream=None, null=()):
        a = self.a
        p = {k: (None if k in null else self.address(k)) for k in ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "hits", "md", "midx", "counts")}
        self.rc = self.lib.kiss_hip_fmi_md_dev(self.ctx._ctx, p["text"], a["text"].size, p["reads"], p["ridx"], a["ridx"].size - 1, 1 if a["both"] else 0,
                                               p["alns"], p["cidx"], p["cigar"], p["oidx"], p["hits"], 0 if self.hits is None else self.hits.size,
                                               p["md"], p["midx"], p["counts"], self.cap, ctypes.byref(self.rep), stream)
        return self

    def fetch(self, name, dtype=np.uint8):
        """through kiss_hip_copy_to_host: a blocking copy on the null stream, no torch call"""
        out = np.empty(self.outs[name].numel(), np.uint8)
        if out.size:
            assert self.lib.kiss_hip_copy_to_host(vp(out.ctypes.data), self.address(name), out.size) == 0
        return out.view(dtype)

    def untouched(self):
        for name in self.outs:
            assert (self.fetch(name) == INIT).all(), name + " was written"
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())

    def check(self, what=""):
        w = self.want
        assert self.rc == 0, (what, self.rc)
        for k in COUNTS:
            print("MD %-40s %-18s %d (model %d)" % (what, k, getattr(self.rep, k), w[k]))
            assert getattr(self.rep, k) == w[k], (what, k)
        midx = self.fetch("midx", np.uint64)
        assert np.array_equal(midx, w["md_index"]), what
        got = self.fetch("md")[:w["md_bytes"]].tobytes()
        if got != w["md"]:
            at = next(k for k in range(len(got)) if got[k] != w["md"][k])
            item = int(np.searchsorted(w["md_index"], at, side="right")) - 1
            b, e = int(w["md_index"][item]), int(w["md_index"][item + 1])
            raise AssertionError("%s: item %d: %r, model %r" % (what, item, got[b:e][:200], w["md"][b:e][:200]))
        assert (self.fetch("md")[w["md_bytes"]:] == INIT).all(), what
        if "counts" in self.outs:
            assert np.array_equal(self.fetch("counts", np.uint32).reshape(-1, 2), w["md_counts"]), what
        dev_place.check_canaries(*self.ins.values(), *self.outs.values())
        return self


def hand_batch(S, both):
    b = Batch(S, both, seed=3)
    n = S.size
    for L in (1, 63, 64, 65, 129, 300):  # one M op, clean, and with mismatches at the chunk boundaries
        b.add(1000 + L, [(M, L)])
        b.add(2000 + L, [(M, L)], mism=sorted({0, min(63, L - 1), min(64, L - 1), L - 1}), pre=L % 3, post=L % 2)
    b.add(3000, [(M, 200)], mism=(5, 6, 7, 63, 64, 65, 127, 128, 199))           # neighbours: A0C, and across chunks
    b.add(3500, [(M, 130)], mism=range(130))                                      # every column
    for ln in (1, 63, 64, 65, 200):
        b.add(4000 + 300 * ln % 5000, [(M, 10), (D, ln), (M, 7)], mism=(10,))     # a mismatch right behind a deletion: ^..0T
        b.add(9000 + ln, [(M, 70), (D, ln), (M, 70)], mism=(69,))                 # ... and right in front of one
    b.add(12000, [(M, 5), (D, 2), (I, 1), (D, 3), (M, 5)])                        # D I D: ^AC0^GTA
    b.add(12100, [(M, 5), (I, 2), (D, 3), (M, 5)])                                # I D
    b.add(12200, [(M, 5), (D, 3), (I, 2), (M, 5)], mism=(5,))                     # D I, a mismatch behind
    b.add(12300, [(M, 5), (D, 2), (D, 3), (M, 5)])                                # two D ops in a row: two '^'
    b.add(12400, [(D, 4), (M, 9)])                                                # a D op first
    b.add(12500, [(M, 9), (D, 4)])                                                # ... and last
    b.add(12600, [(I, 3), (M, 80), (I, 70), (M, 80), (I, 2)], mism=(79, 80))      # an insertion does not end a run
    b.add(13000, [(M, 1), (I, 1)] * 500, mism=(0, 250, 499))                      # 1000 ops of one base
    b.add(15000, [(M, 1), (D, 1)] * 100 + [(M, 1)])
    b.add(16000, [(M, 150)], no_base=(0, 10, 64, 149), mism=(10, 11))             # no-bases, over a match and over a mismatch
    b.add(n - 100, [(M, 100)], mism=(99,))                                        # tend = n
    b.add(n - 5, [(M, 2), (D, 3)])
    b.add(0, [(M, 70)], mism=(0,))                                                # tbeg = 0
    if both:
        for L in (1, 64, 65, 150):
            b.add(17000 + L, [(M, L)], mism=(0, L - 1), rev=True, pre=2, post=5)
        b.add(18000, [(M, 40), (D, 5), (M, 30), (I, 4), (M, 40)], mism=(3, 69, 70), no_base=(20,), rev=True, pre=1)
    q = len(b.reads) - 1
    b.more(q, both, [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 77], [])                    # an item with no ops (band too wide)
    b.more(0, False, [0] * 12, [])                                                # ... (not aligned), on the first read
    return b


@pytest.mark.parametrize("leads", [(1, 3, 3), (3, 1, 1)])
@pytest.mark.parametrize("both", (False, True))
def test_shapes_by_hand(ctx, S, both, leads):
    a, number = hand_batch(S, both).arrays()
    c = Call(ctx, a, byte_leads=leads).check("all alignments")
    assert c.want["bad"] == 0 and c.want["items"] == number.size
    assert any("^" in s and "0^" in s for s in c.want["strings"]) and c.want["strings"].count("") == 2
    C = number.size
    # hits: descending, one alignment twice, without the counts
    hits = list(range(C - 1, -1, -1)) + [3, 3, 0, C - 1]
    Call(ctx, a, hits=hits, byte_leads=leads, want_counts=False).check("hits in descending order")
    Call(ctx, a, hits=[], byte_leads=leads).check("no hits")


def test_a_chain_index_that_does_not_start_at_0_and_virtual_reads_without_alignments(ctx, S):
    b = Batch(S, True, seed=8, first=1 << 33)
    b.add(500, [(M, 90)], mism=(4,))
    b.reads.append(np.array([0, 1, 2], np.uint8))  # a read with no alignment: two empty segments
    b.add(700, [(M, 90)], mism=(5,), rev=True)
    b.add(900, [(M, 40), (D, 2), (M, 40)])
    a, _ = b.arrays()
    assert a["cidx"].tolist() == [(1 << 33) + x for x in (0, 1, 1, 1, 1, 1, 2, 3, 3)]
    Call(ctx, a).check("first = 2^33")


def test_digit_boundaries_and_ten_thousand_light_items_beside_a_long_one(ctx, S):
    b = Batch(S, False, seed=5)
    runs = (9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000)
    cols, at = [], 0
    for r in runs:  # a mismatch behind every run; the last column is a mismatch too
        at += r
        cols.append(at)
        at += 1
    L = at + 7
    assert 220_000 < L < 240_000
    b.add(100, [(M, L)], mism=cols)
    rng = np.random.default_rng(9)
    for k in range(10_000):
        b.add(int(rng.integers(0, S.size - 40)), [(M, 12), (D, 1), (M, 12)] if k % 7 == 0 else [(M, 24)], mism=(k % 24,) if k % 3 else ())
    a, _ = b.arrays()
    c = Call(ctx, a).check("long and light")
    assert c.want["strings"][0] == "".join("%d%s" % (r, "ACGT"[S[100 + col]]) for r, col in zip(runs, cols)) + "7"
    assert c.want["longest"] == len(c.want["strings"][0])


# ---- bad items ---------------------------------------------------------------------------------------------------------------------
def test_bad_items_beside_good_ones(ctx, S):
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
    a, number = b.arrays()
    c = Call(ctx, a).check("one of every kind")
    assert c.want["bad"] == len(bad)
    for k in bad:
        assert c.want["strings"][number[k]] == ""
    for k in good:
        assert c.want["strings"][number[k]] != ""
    C = number.size
    c = Call(ctx, a, hits=[number[good[0]], C, number[bad[0]], 0xFFFFFFFF, number[good[1]], C + 1, number[good[2]]]).check("aln out of range")
    assert c.want["bad"] == 4 and [len(s) > 0 for s in c.want["strings"]] == [True, False, False, False, True, False, True]


# ---- the capacity protocol and the error contract ----------------------------------------------------------------------------------
def test_capacity_protocol_and_error_contract(ctx, S):
    from kiss_amd import _lib
    a, number = hand_batch(S, True).arrays()
    whole = mm.md(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], True)
    total = whole["md_bytes"]
    for cap in (0, 1, total - 1):
        c = Call(ctx, a, capacity=cap)
        assert c.rc == _lib.KISS_HIP_E_INVALID
        for k in COUNTS:  # the totals are in the report
            assert getattr(c.rep, k) == c.want[k], k
        c.untouched()
    c = Call(ctx, a, capacity=0, run=False).run(null=("md", "counts"))  # md may be NULL while the capacity is 0
    assert c.rc == _lib.KISS_HIP_E_INVALID and c.rep.md_bytes == total
    c.untouched()
    Call(ctx, a, capacity=total + 100).check("room to spare")
    # a required pointer NULL; room named without md
    for k in ("text", "reads", "ridx", "alns", "cidx", "cigar", "oidx", "midx"):
        c = Call(ctx, a, run=False).run(null=(k,))
        assert c.rc == _lib.KISS_HIP_E_INVALID, k
        c.untouched()
    assert Call(ctx, a, run=False).run(null=("md",)).rc == _lib.KISS_HIP_E_INVALID
    # an index that decreases, a read of length 0: nothing written
    for name, at in (("cidx", 3), ("ridx", 2), ("oidx", 5)):
        broken = dict(a)
        broken[name] = a[name].copy()
        broken[name][at] = a[name][at + 1] + np.uint64(1)
        c = Call(ctx, broken, want=whole).run()
        assert c.rc == _lib.KISS_HIP_E_INVALID, name
        c.untouched()
    empty = dict(a)
    empty["ridx"] = a["ridx"].copy()
    empty["ridx"][4] = empty["ridx"][3]
    c = Call(ctx, empty, run=False, hits=[0]).run()
    assert c.rc == _lib.KISS_HIP_E_INVALID
    c.untouched()
    # zero items: no alignments, no reads
    none = Batch(S, True)
    none.reads.append(np.array([1, 2], np.uint8))
    a0, _ = none.arrays()
    c = Call(ctx, a0)
    assert c.rc == 0 and c.fetch("midx", np.uint64).tolist() == [0] and c.rep.items == 0 and c.rep.md_bytes == 0
    dev_place.check_canaries(*c.ins.values(), *c.outs.values())
    a0, _ = Batch(S, False).arrays()
    c = Call(ctx, a0, hits=[0, 7]).check("no reads, two hits")  # (every hit names an alignment that does not exist)
    assert c.want["bad"] == 2


def test_the_host_entry_and_md_strings(S):
    import kiss_amd
    a, number = hand_batch(S, True).arrays()
    want = mm.md(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], True)
    res = kiss_amd.md_tags(a["text"], (a["reads"], a["ridx"]), a["alns"], a["cidx"], a["cigar"], a["oidx"], both_strands=True)
    assert res["md"].tobytes() == want["md"] and np.array_equal(res["md_index"], want["md_index"])
    assert np.array_equal(res["md_counts"], want["md_counts"]) and kiss_amd.md_strings(res["md"], res["md_index"]) == want["strings"]
    for k in COUNTS:
        assert res["report"][k] == want[k], k
    hits = [5, 5, 2, number.size + 3]
    want = mm.md(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], True, hits)
    res = kiss_amd.md_tags(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], both_strands=True, hits=hits)
    assert kiss_amd.md_strings(res["md"], res["md_index"]) == want["strings"] and res["report"]["bad"] == 1
    res = kiss_amd.md_tags(a["text"], a["read_list"], a["alns"], a["cidx"], a["cigar"], a["oidx"], both_strands=True, hits=[])
    assert res["md"].size == 0 and res["md_index"].tolist() == [0]


# ---- the caller's stream -----------------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(ctx, S):
    """tests/test_dev_stream_gpu.py's method: after a warm-up on the NULL stream the reads are overwritten with a decoy (other
    bases: other strings of other lengths); a delay and then the copy that puts the real reads back are queued on s; the call
    is made with s while s is busy; on return the outputs are read by a blocking copy on the null stream."""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    b = Batch(S, True, seed=12)
    rng = np.random.default_rng(13)
    for k in range(600):
        b.add(int(rng.integers(0, S.size - 400)), [(M, 70), (D, 2), (M, 78)] if k % 5 == 0 else [(M, 150)], mism=rng.integers(0, 148, 3),
              rev=bool(k % 2))
    a, _ = b.arrays()
    c = Call(ctx, a)
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
    c.ins["reads"].copy_(torch.from_numpy(decoy))  # 2. the decoy; the outputs as before any call
    for v in c.outs.values():
        v.fill_(INIT)
    torch.cuda.synchronize()
    before = ctx.workspace_bytes()
    with Delayed(s, idle_ms) as delay:  # 3. a delay on s, and behind it the real input
        c.ins["reads"].copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.run(vp(s.cuda_stream))  # 4. the call, while s is busy
    got = c.fetch("md").tobytes()  # 5. no torch synchronisation
    after = ctx.workspace_bytes()
    delay.check("kiss_hip_fmi_md_dev")
    assert after == before, "the timed call allocated work arrays (%d -> %d bytes)" % (before, after)
    assert got == c.want["md"]
    c.check("on the caller's stream")


# ---- through the pipeline ----------------------------------------------------------------------------------------------------------
MD_KEYS = {"md", "md_index", "md_counts", "md_report"}
PARAM_SETS = (dict(), dict(align_params=dict(match=2, mismatch=3, gap_open=0, gap_extend=1, band=16), min_score=20, max_hits=3))


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


def check_pipeline(res, plain, S, reads, both):
    same_results({k: v for k, v in res.items() if k not in MD_KEYS}, plain)
    assert MD_KEYS <= res.keys() and not MD_KEYS & plain.keys()
    hits = res["hits"]
    want = mm.md(S, reads, res["alignments"], res["chain_index"], res["cigar"], res["cigar_index"], both, hits["aln"])
    assert res["md"].tobytes() == want["md"] and np.array_equal(res["md_index"], want["md_index"])
    assert np.array_equal(res["md_counts"], want["md_counts"])
    for k in COUNTS:
        assert res["md_report"][k] == want[k], k
    assert want["bad"] == 0 and want["items"] == hits.size
    cidx = [int(x) for x in res["chain_index"]]
    for h in range(hits.size):  # the inverse: SEQ, CIGAR and MD give the text back
        a = int(hits["aln"][h])
        rec = res["alignments"][a]
        v = mm.read_of(a, cidx, both)
        Rv = am.virtual_read(reads[v // 2] if both else reads[v], both and v % 2 == 1)
        ops = mm.unpack_ops(res["cigar"][int(res["cigar_index"][a]):int(res["cigar_index"][a + 1])])
        assert ops and want["strings"][h]
        rebuilt = mm.rebuild_text(Rv, rec["rbeg"], ops, want["strings"][h])
        assert rebuilt == "".join("ACGT"[c] for c in S[int(rec["tbeg"]):int(rec["tend"])]), (h, want["strings"][h])
        assert want["md_counts"][h].tolist() == [int(rec["mismatches"]), int(rec["del"])]
    return want


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_md_equals_the_model_and_gives_the_text_back(name, both):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    assert len(TEXTS) == 7
    f = index_of(name, 4)
    S = text(name)
    reads = reads_of(name)
    for params in PARAM_SETS:
        common = dict(both_strands=both, chain_params=dict(min_score=25, band=100), **params)
        res = f.map(reads, S, 15, 0, 200, want_md=True, **common)
        plain = f.map(reads, S, 15, 0, 200, **common)
        want = check_pipeline(res, plain, S, reads, both)
    if name in ("genome", "iid"):
        assert want["items"] >= 4 and want["mismatch_columns"] > 0
    with pytest.raises(ValueError):
        f.map(reads, S, want_md=True, want_cigar=False)


@pytest.mark.parametrize("rescue", (None, True))
@pytest.mark.parametrize("name", ("genome", "iid", "periodic", "n5"))
def test_map_pairs_with_md_with_and_without_rescue(name, rescue):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f = index_of(name, 4)
    S = text(name)
    m1, m2 = mates_of(name)
    reads = [r for pr in zip(m1, m2) for r in pr]
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue)
    res = f.map_pairs(m1, m2, S, 15, 0, 200, want_md=True, **common)
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, **common)
    check_pipeline(res, plain, S, reads, True)
    with pytest.raises(ValueError):
        f.map_pairs(m1, m2, S, want_md=True, want_cigar=False)
