"""The BAM records written on the device (kiss_hip_fmi_bam_dev / _host; include/kiss_hip_bam.h) against their definition,
tests/bam_model.py: every byte of bam, rec_index, read_rec and every field of the report but the times.  The batches are made by
the SAM model's make_batch and put on the device by the helpers of tests/test_fm_sam_gpu.py; outputs lie between guard bytes;
bad reads of every kind, the size-then-fill protocol, odd addresses, the caller's stream, the host entry, and arrays placed on
both sides of 2^31 and across a multiple of 2^32."""
import ctypes

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from kiss_amd.sam_writer import sam_input
from tests import bam_model as B
from tests import fm_sam_model as M
from tests.test_fm_sam_gpu import GUARD, PAD, bad_batch, guarded, guards_intact, host_arrays, put, rng_of, u64_of

pytestmark = pytest.mark.gpu

REPORT = ("records", "bam_bytes", "unmapped_records", "longest", "bad", "first_bad")


class Outputs:
    def __init__(self, dev, bam_cap, rec_cap, Q, odd=False, bam_view=None, want_index=True):
        self.bam_whole, self.bam = guarded(dev, max(bam_cap, 1), 1 if odd else 0)
        if bam_view is not None:
            self.bam_whole, self.bam = bam_view
        self.ri_whole, self.ri = guarded(dev, 8 * (rec_cap + 1), 8)
        self.rr_whole, self.rr = guarded(dev, 8 * (Q + 1), 8)
        self.bam_cap, self.rec_cap, self.want_index = bam_cap, rec_cap, want_index

    def untouched(self):
        return bool(np.all(self.bam.cpu().numpy() == GUARD) and np.all(self.ri.cpu().numpy() == GUARD) and np.all(self.rr.cpu().numpy() == GUARD))

    def intact(self):
        return guards_intact(self.bam_whole, self.bam) and guards_intact(self.ri_whole, self.ri) and guards_intact(self.rr_whole, self.rr)


def call_dev(lib, ctx, d, counts, o, stream=None, null_bam=False):
    vp = ctypes.c_void_p
    inp = sam_input({k: (None if v is None else v.data_ptr()) for k, v in d.items() if k != "_keep"}, *counts)
    rep = _lib.BamReport()
    rc = lib.kiss_hip_fmi_bam_dev(ctx._ctx, ctypes.byref(inp), None if null_bam else vp(o.bam.data_ptr()), o.bam_cap,
                                  vp(o.ri.data_ptr()) if o.want_index else None, o.rec_cap, vp(o.rr.data_ptr()), ctypes.byref(rep),
                                  vp(stream) if stream else None)
    return rc, rep


def same_as_model(want, o, rep, what):
    got = o.bam.cpu().numpy()[:len(want["bam"])].tobytes()
    if got != want["bam"]:
        k = next(i for i in range(len(got)) if got[i] != want["bam"][i])
        r = int(np.searchsorted(want["rec_index"], k, side="right")) - 1
        at = int(want["rec_index"][r])
        raise AssertionError("%s: bam differs at byte %d, byte %d of record %d: got %r, want %r"
                             % (what, k, k - at, r, got[max(at, k - 40):k + 24], want["bam"][max(at, k - 40):k + 24]))
    assert np.array_equal(u64_of(o.ri), want["rec_index"]), what
    assert np.array_equal(u64_of(o.rr), want["read_rec"]), what
    assert {k: int(getattr(rep, k)) for k in REPORT} == want["report"], what
    assert o.intact(), what


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 22, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


def check(gpu, b, what, odd=False):
    lib, ctx, dev = gpu
    want = B.bam_model(b)
    arrs, counts = host_arrays(b)
    d = put(dev, arrs, odd)
    o = Outputs(dev, len(want["bam"]), want["report"]["records"], counts[0], odd)
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0, (what, rc, int(rep.bad), int(rep.first_bad))
    same_as_model(want, o, rep, what)
    return want


def clips_of(b):
    """(alignments without a clip, with one)"""
    with_clip = 0
    for q in range(len(b["read_index"]) - 1):
        L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
        for h in range(int(b["hit_index"][q]), int(b["hit_index"][q + 1])):
            k = b["alns"][int(b["hits"][h][M.H_ALN])]
            with_clip += bool(int(k[M.A_RBEG]) or int(k[M.A_REND]) < L)
    return len(b["hits"]) - with_clip, with_clip


def shaped_batches():
    """(name, batch): the shapes at which the kernels change their path"""
    out = []
    r = rng_of(70)
    lengths = [1, 2, 63, 64, 65, 127, 128, 129, 10000, 3]  # odd and even (the nibble pad), around the 64 lanes of a step and 128 bases
    for paired in (False, True):
        b = M.make_batch(r, lengths, [2, 1, 2, 2, 2, 2, 2, 2, 2, 0], paired=paired)
        assert {int(t[M.H_FLAGS]) & 1 for t in b["hits"]} == {0, 1}  # both strands
        out.append(("lengths, paired %d" % paired, b))
    names = [bytes(r.integers(33, 127, n).astype(np.uint8)) for n in (1, 254, 63, 64, 65)]
    out.append(("names of 1 and 254 bytes", M.make_batch(r, [30] * 5, [1, 0, 2, 1, 3], names=names)))
    for md_len in (0, 1, 63, 64, 65, 1000):
        out.append(("md_len %d" % md_len, M.make_batch(r, [40, 50, 60, 70], [1, 2, 0, 3], paired=md_len % 2 == 1, md_len=md_len)))
    for n_ops in (1, 63, 64, 65, 1000):
        b = M.make_batch(r, [3100, 3200], [6, 6], paired=n_ops == 65, n_ops=n_ops)
        assert min(clips_of(b)) > 0  # with and without clips
        out.append(("n_ops %d" % n_ops, b))
    for paired in (False, True):
        out.append(("0 .. 65 hits per read, paired %d" % paired, M.make_batch(r, r.integers(20, 70, 66), list(range(66)), paired=paired)))
    for Q in (1, 257, 258):
        out.append(("Q %d" % Q, M.make_batch(r, r.integers(1, 80, Q), r.choice([0, 1, 2, 3], Q), paired=Q % 2 == 0)))
    for R in (1, 3):
        for same in (False, True):
            out.append(("R %d same %d" % (R, same), M.make_batch(r, r.integers(20, 60, 8), [2] * 8, R=R, paired=True, same_names=same)))
    for paired in (False, True):
        b = M.make_batch(r, r.integers(20, 60, 12), [3] * 12, R=3, paired=paired, big=True)  # ten-digit numbers; a TLEN that wraps
        assert max(B._pos0(b, h)[1] for h in range(36)) >= 10 ** 9
        out.append(("big, paired %d" % paired, b))
    for chosen in ("first", "middle", "last", "none"):
        out.append(("chosen " + chosen, M.make_batch(r, r.integers(20, 60, 6), [3, 3, 1, 3, 0, 3], paired=True, chosen=chosen)))
    for qual in (False, True):
        for md in (False, True):
            for source in (False, True):
                out.append(("qual %d md %d source %d" % (qual, md, source),
                            M.make_batch(r, r.integers(20, 60, 6), [2, 1, 3, 0, 1, 2], paired=True, qual=qual, md=md, source=source)))
    return out


SHAPED = shaped_batches()


def test_the_first_200_random_batches(gpu):
    r = rng_of(20250)
    done = 0
    while done < 200:
        b = M.random_batch(r)
        if not b["ref_names"]:
            continue  # (R = 0 is refused: test_no_records_is_refused)
        if B.bad_reads_first(b):  # one record of nearly 2^32 bases: positions that BAM cannot hold
            refused(gpu, b, "random batch %d" % done)
        else:
            check(gpu, b, "random batch %d" % done)
        done += 1


@pytest.mark.parametrize("k", range(len(SHAPED)), ids=[n for n, _ in SHAPED])
def test_shapes(gpu, k):
    check(gpu, SHAPED[k][1], SHAPED[k][0])


def test_ten_thousand_one_hit_reads_beside_a_read_of_65_hits(gpu):
    r = rng_of(11)
    Q = 10001
    n_hits = np.ones(Q, np.int64)
    n_hits[5000] = 65
    want = check(gpu, M.make_batch(r, r.integers(30, 50, Q), n_hits, md=False), "10^4 reads")
    assert want["report"]["records"] == 10000 + 65


def test_zero_reads_and_no_records(gpu):
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(3), [30], [1])
    arrs, counts = host_arrays(b)
    zero = dict(arrs, read_index=np.zeros(1, np.uint64), hit_index=np.zeros(1, np.uint64))
    o = Outputs(dev, 0, 0, 0)
    rc, rep = call_dev(lib, ctx, put(dev, zero), (0, 0, 3, 0), o)
    assert rc == 0 and u64_of(o.rr).tolist() == [0] and u64_of(o.ri).tolist() == [0]
    assert {k: int(getattr(rep, k)) for k in REPORT} == dict.fromkeys(REPORT, 0)
    assert np.all(o.bam.cpu().numpy() == GUARD) and o.intact()
    # R = 0: BAM needs records
    b0 = M.make_batch(rng_of(3), [30], [1], R=0)
    arrs, counts = host_arrays(b0)
    assert counts[2] == 0
    o = Outputs(dev, 1 << 12, 8, 1)
    rc, rep = call_dev(lib, ctx, put(dev, arrs), counts, o)
    assert rc == _lib.KISS_HIP_E_INVALID and o.untouched() and o.intact()


# ---- bad reads -------------------------------------------------------------------------------------------------------------
def refused(gpu, b, what):
    lib, ctx, dev = gpu
    want = B.bam_model(b)["report"]
    assert set(want) == {"bad", "first_bad"} and want["bad"] > 0, what
    arrs, counts = host_arrays(b)
    o = Outputs(dev, 1 << 20, 1 << 10, counts[0])
    rc, rep = call_dev(lib, ctx, put(dev, arrs), counts, o)
    assert rc == _lib.KISS_HIP_E_INVALID, what
    assert (int(rep.bad), int(rep.first_bad)) == (want["bad"], want["first_bad"]), what
    assert int(rep.records) == 0 and int(rep.bam_bytes) == 0, what
    assert o.untouched() and o.intact(), what
    return want


def bam_bad_batch(kind, where):
    """a valid paired batch of eight reads with one thing in read q that BAM cannot hold; the second hit of q is not the chosen one"""
    lengths = [30, 40, 50, 60, 70, 80, 90, 100]
    q = {"first": 0, "middle": 3, "last": 7}[where]
    if kind == "ops":
        lengths[q] = 65534 + 5
    b = M.make_batch(rng_of(5), lengths, [2] * 8, R=1 if kind == "pos" else 3, paired=True, chosen="first", big=kind == "pos")
    h = int(b["hit_index"][q]) + 1
    a = int(b["hits"][h][M.H_ALN])
    if kind == "name0":
        b["names"][q] = b""
    elif kind == "name255":
        b["names"][q] = b"n" * 255
    elif kind == "op_code":
        b["cigar"][int(b["cigar_index"][a])] = 7 << 4 | 3
    elif kind == "ops":  # 65534 ops and both clips: one entry more than n_cigar_op holds
        b["alns"][a][M.A_RBEG], b["alns"][a][M.A_REND] = 2, 2 + 65534
        lists = [list(b["cigar"][int(b["cigar_index"][x]):int(b["cigar_index"][x + 1])]) for x in range(len(b["alns"]))]
        lists[a] = [1 << 4 | (j & 1) for j in range(65534)]
        b["cigar"] = np.array([w for x in lists for w in x], np.uint32)
        b["cigar_index"] = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.uint64)
    elif kind == "pos":  # one record of nearly 2^32 bases; every position below 2^31 but one, which is exactly 2^31
        b["alns"][:, M.A_TBEG] %= 1 << 31
        b["alns"][:, 5] = b["alns"][:, M.A_TBEG] + 1
        b["alns"][a][M.A_TBEG] = 1 << 31
    return b, q


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["aln", "ref", "tbeg", "rbeg", "rend", "bad_input", "other_reads_hit", "name0", "name255", "op_code", "ops", "pos"])
def test_bad_reads(gpu, kind, where):
    b, q = (bam_bad_batch if kind in ("name0", "name255", "op_code", "ops", "pos") else bad_batch)(kind, where)
    want = refused(gpu, b, kind)
    assert want == {"bad": 2 if kind == "bad_input" else 1, "first_bad": min(q, q ^ 1) if kind == "bad_input" else q}


def test_a_chosen_hit_past_2_31_makes_both_mates_bad_and_ops_of_exactly_65535_are_written(gpu):
    b, q = bam_bad_batch("pos", "middle")
    mine = int(b["hit_index"][q])
    b["alns"][int(b["hits"][mine][M.H_ALN])][M.A_TBEG] = (1 << 31) + 5  # the chosen hit: the partner's PNEXT
    assert refused(gpu, b, "chosen")["bad"] == 2
    b, q = bam_bad_batch("ops", "middle")
    a = int(b["hits"][int(b["hit_index"][q]) + 1][M.H_ALN])
    b["alns"][a][M.A_RBEG] = 0  # 65534 ops and one clip
    b["cigar"][int(b["cigar_index"][a])] += 2 << 4
    want = check(gpu, b, "65535 cigar entries")
    assert want["report"]["longest"] > 4 * 65535


# ---- size, then fill -------------------------------------------------------------------------------------------------------
def test_capacity_protocol(gpu):
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(9), [30, 40, 50, 60], [2, 0, 3, 1], paired=True)
    want = B.bam_model(b)
    total, recs = len(want["bam"]), want["report"]["records"]
    arrs, counts = host_arrays(b)
    d = put(dev, arrs)
    totals = {k: want["report"][k] for k in ("records", "bam_bytes", "unmapped_records", "longest")}
    for bam_cap, rec_cap, null_bam in ((0, 0, True), (total - 1, recs, False), (total, recs - 1, False), (0, recs, False)):
        o = Outputs(dev, bam_cap, rec_cap, counts[0])
        rc, rep = call_dev(lib, ctx, d, counts, o, null_bam=null_bam)
        assert rc == _lib.KISS_HIP_E_INVALID, (bam_cap, rec_cap)
        assert {k: int(getattr(rep, k)) for k in totals} == totals and rep.bad == 0
        assert o.untouched() and o.intact()
    o = Outputs(dev, total, 0, counts[0], want_index=False)
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0 and o.bam.cpu().numpy().tobytes() == want["bam"] and np.all(o.ri.cpu().numpy() == GUARD) and o.intact()
    o = Outputs(dev, total + 100, recs + 5, counts[0])
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0 and o.bam.cpu().numpy()[:total].tobytes() == want["bam"] and np.all(o.bam.cpu().numpy()[total:] == GUARD)
    assert np.array_equal(u64_of(o.ri)[:recs + 1], want["rec_index"]) and np.all(o.ri.cpu().numpy()[8 * (recs + 1):] == GUARD) and o.intact()


# ---- alignment and stream ---------------------------------------------------------------------------------------------------
def test_odd_addresses(gpu):
    r = rng_of(13)
    check(gpu, M.make_batch(r, r.integers(1, 200, 40), r.choice([0, 1, 2, 5], 40), paired=True), "odd addresses, paired", odd=True)
    check(gpu, M.make_batch(r, r.integers(1, 200, 33), r.choice([0, 1, 2, 5], 33)), "odd addresses", odd=True)


def test_work_runs_on_the_callers_stream_and_is_done_on_return(gpu):
    """the pattern of tests/test_fm_sam_gpu.py: a decoy batch of the same shapes lies in the inputs; a delay on the caller's stream,
    and behind it the copies that put the real batch back; the call, made while the stream is busy, must see the real one and be
    finished on return"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(17), rng_of(18).integers(30, 200, 64), [2] * 64, paired=True)
    want = B.bam_model(b)
    arrs, counts = host_arrays(b)
    decoy = dict(arrs)
    decoy["reads"] = (arrs["reads"] + 1) % 6
    decoy["qual"] = 33 + (arrs["qual"] - 33 + 1) % 94
    decoy["md"] = arrs["md"][::-1].copy()
    d = put(dev, arrs)
    changed = ("reads", "qual", "md")  # (records of the same lengths, other bytes)
    staging = {k: d[k].clone() for k in changed}
    o = Outputs(dev, len(want["bam"]), want["report"]["records"], counts[0])
    for _ in range(2):  # warm up on the null stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, rep = call_dev(lib, ctx, d, counts, o)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    same_as_model(want, o, rep, "warm-up on the null stream")
    for k in changed:
        d[k].copy_(torch.from_numpy(np.ascontiguousarray(decoy[k]).reshape(-1).view(np.uint8).copy()))
    for v in (o.bam, o.ri, o.rr):
        v.fill_(GUARD)
    torch.cuda.synchronize()
    rc, rep = call_dev(lib, ctx, d, counts, o)  # (the decoy gives other bytes)
    assert rc == 0 and o.bam.cpu().numpy()[:len(want["bam"])].tobytes() != want["bam"]
    o.bam.fill_(GUARD)
    torch.cuda.synchronize()
    s = caller_stream()
    with Delayed(s, idle_ms) as delay:
        for k in changed:
            d[k].copy_(staging[k], non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    rc, rep = call_dev(lib, ctx, d, counts, o, stream=s.cuda_stream)
    got = o.bam.cpu().numpy().tobytes()  # (a copy on the null stream, which does not wait for s)
    delay.check("kiss_hip_fmi_bam_dev")
    assert rc == 0 and got == want["bam"]
    same_as_model(want, o, rep, "on the caller's stream")


# ---- the host entry ----------------------------------------------------------------------------------------------------------
def test_the_host_entry_gives_the_same_bytes():
    import kiss_amd.bam_writer as W
    picked = [b for _, b in SHAPED[::4]][:10]
    assert len(picked) == 10
    for k, b in enumerate(picked):
        want = B.bam_model(b)
        got = W.bam_records(**b)
        assert got["bam"].tobytes() == want["bam"], k
        assert np.array_equal(got["rec_index"], want["rec_index"]) and np.array_equal(got["read_rec"], want["read_rec"]), k
        assert {x: got["report"][x] for x in REPORT} == want["report"], k
    for kind in ("rend", "op_code"):
        b, q = (bam_bad_batch if kind == "op_code" else bad_batch)(kind, "middle")
        with pytest.raises(_lib.KissHipError) as e:
            W.bam_records(**b)
        assert e.value.status == _lib.KISS_HIP_E_INVALID and (e.value.report["bad"], e.value.report["first_bad"]) == (1, 3)


# ---- placement across 2^31 and 2^32 (the supposed cause of the first SAM writer's fault) -------------------------
def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    """every array of the batch is valid memory wherever it lies, so a correct kernel cannot fault here; a kernel that widens
    the low half of an address with its sign would"""
    import torch
    lib, ctx, dev = gpu
    r = rng_of(23)
    names = [bytes(r.integers(33, 127, 200).astype(np.uint8)) for _ in range(8)]
    b = M.make_batch(r, [300] * 8, [2] * 8, paired=True, names=names, md_len=150)
    want = B.bam_model(b)
    arrs, counts = host_arrays(b)
    total = len(want["bam"])
    assert min(arrs[k].size for k in ("reads", "names", "md")) > 1024 and total > 1024
    G = 1 << 32
    arena = torch.empty(G + (64 << 20), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    to_carry = (-base) % G  # the offset of the first multiple of 2^32 in the arena
    high = (to_carry + (1 << 31) + 4096) % G
    places = {"high half": high if high >= PAD else high + G, "low half": to_carry + 4096,
              "across a multiple of 2^32": to_carry - 1024 if to_carry >= 1024 + PAD else to_carry + G - 1024}
    for what, off in places.items():
        lo = (base + off) & (G - 1)
        assert {"high half": lo >= 1 << 31, "low half": lo < 1 << 31, "across a multiple of 2^32": lo == G - 1024}[what]
        assert off >= PAD and off + total + PAD <= arena.numel()
        for name in ("bam", "reads", "names", "md"):
            if name == "bam":
                whole = arena[off - PAD:off + total + PAD]
                whole.fill_(GUARD)
                d = put(dev, arrs)
                o = Outputs(dev, total, want["report"]["records"], counts[0], bam_view=(whole, whole[PAD:PAD + total]))
            else:
                d = put(dev, arrs, place={name: arena[off:]})
                o = Outputs(dev, total, want["report"]["records"], counts[0])
            rc, rep = call_dev(lib, ctx, d, counts, o)
            assert rc == 0, (what, name)
            same_as_model(want, o, rep, "%s at %s" % (name, what))
    del arena
