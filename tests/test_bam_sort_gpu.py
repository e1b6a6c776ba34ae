"""BAM records put into coordinate order on the device (kiss_hip_bam_sort_dev / _host; include/kiss_hip_bam_sort.h)
against their definition, tests/bam_sort_model.py: every byte of out, out_index and order and every count of the report.  Synthetic
records with random bodies at the shapes where a kernel changes its path -- record counts around the wave and the workgroup, key
widths around a byte of the packed key, positions around the bytes of pos + 1, record sizes at every phase of a 16-byte line and
one record of 300 000 bytes --, every pair of byte addresses of input and output, NULL outputs, every kind of BAD input, the
caller's stream, arrays on both sides of 2^31 and across a multiple of 2^32, the host entry, and the real records of
tests/test_fm_bam_gpu.py's batches.  Inputs and outputs lie between guard bytes (tests/dev_place.py)."""
import ctypes
import struct

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bam_model as B
from tests import bam_sort_model as M
from tests.dev_place import check_canaries, place, place_out, read_back

pytestmark = pytest.mark.gpu

COUNTS = ("records", "bam_bytes", "unplaced", "longest", "bad", "first_bad")
INIT = 0xEE  # what place_out leaves in an output


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 22, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


def records_of(rng, count, n_ref=3, sizes=(36, 130), refs=None, positions=None):
    """`count` records with random bodies: refs and positions drawn from few values, so that keys tie"""
    refs = [-1, 0, n_ref - 1, n_ref // 2] if refs is None else refs
    positions = [0, 1, 2, 3, 1000] if positions is None else positions
    out = []
    for _ in range(count):
        ref = int(rng.choice(refs))
        pos = -1 if ref == -1 else int(rng.choice(positions))
        out.append(M.make_record(ref, pos, rng.integers(0, 256, int(rng.integers(sizes[0], sizes[1] + 1)) - 36, dtype=np.uint8).tobytes()))
    return out


class Call:
    """one call of the device entry on placed arrays"""

    def __init__(self, gpu, bam, ri, n_ref, bam_lead=1, out_lead=3, want_index=True, want_order=True, stream=None, short=0):
        lib, ctx, dev = gpu
        self.records = records = ri.size - 1
        self.bam = place(bam, bam_lead, 64, (0xA5, 0x5A, 0x3C), dev)
        self.ri = place(ri, 8, 64, 0xC3, dev)
        self.cap = bam.size - short
        self.out = place_out(self.cap, out_lead, 256, (0x11, 0x22, 0x33), dev, init=INIT)
        self.oi = place_out(8 * (records + 1), 8, 64, 0x44, dev, init=INIT)
        self.order = place_out(4 * records, 4, 64, 0x55, dev, init=INIT)
        self.want_index, self.want_order = want_index, want_order
        self.rep = _lib.BamSortReport()
        self.rc = self.run(lib, ctx, n_ref, stream)

    def run(self, lib, ctx, n_ref, stream=None):
        vp = ctypes.c_void_p
        a = lambda v: vp(v.placement.address)  # noqa: E731
        return lib.kiss_hip_bam_sort_dev(ctx._ctx, a(self.bam) if self.bam.numel() else None, self.bam.numel(), a(self.ri), self.records, n_ref,
                                         a(self.out) if self.cap else None, self.cap, a(self.oi) if self.want_index else None,
                                         a(self.order) if self.want_order else None, ctypes.byref(self.rep), vp(stream) if stream else None)

    def counts(self):
        return {k: int(getattr(self.rep, k)) for k in COUNTS}

    def untouched(self):
        check_canaries(self.out, self.oi, self.order, self.bam, self.ri)
        return all(bool(np.all(read_back(v) == INIT)) for v in (self.out, self.oi, self.order))

    def same_as(self, want, what):
        assert self.rc == 0, (what, self.rc, self.counts())
        got = read_back(self.out)
        if not np.array_equal(got, want["bam"]):
            k = int(np.flatnonzero(got != want["bam"])[0])
            s = int(np.searchsorted(want["rec_index"], k, side="right")) - 1
            raise AssertionError("%s: out differs at byte %d, byte %d of the record in slot %d (input record %d): got %s, want %s"
                                 % (what, k, k - int(want["rec_index"][s]), s, int(want["order"][s]), got[max(0, k - 8):k + 8].tolist(),
                                    want["bam"][max(0, k - 8):k + 8].tolist()))
        if self.want_index:
            assert np.array_equal(read_back(self.oi, np.uint64), want["rec_index"]), what
        else:
            assert np.all(read_back(self.oi) == INIT), what
        if self.want_order:
            assert np.array_equal(read_back(self.order, np.uint32), want["order"]), what
        else:
            assert np.all(read_back(self.order) == INIT), what
        assert self.counts() == want["report"], what
        check_canaries(self.out, self.oi, self.order, self.bam, self.ri)


def model(bam, ri, n_ref):
    """the loops for what they can do in a moment, numpy's stable sort (held against them in tests/test_bam_sort_model.py) beyond"""
    return (M.sort if ri.size <= 300 else M.sort_fast)(bam, ri, n_ref)


def check(gpu, recs, n_ref, what, **how):
    bam, ri = M.pack(recs)
    want = model(bam, ri, n_ref)
    assert "bam" in want, what
    Call(gpu, bam, ri, n_ref, **how).same_as(want, what)
    return want


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_record_counts(gpu, count):
    want = check(gpu, records_of(np.random.default_rng(count), count), 3, "%d records" % count)
    assert want["report"]["records"] == count


def test_orders_of_the_input(gpu):
    rng = np.random.default_rng(5)
    recs = records_of(rng, 700, n_ref=4, positions=list(range(40)))
    key = lambda r: M.key_of(r, 0, 4)  # noqa: E731
    in_order = sorted(recs, key=key)
    assert check(gpu, in_order, 4, "already sorted")["order"].tolist() == list(range(700))
    want = check(gpu, in_order[::-1], 4, "reversed")
    assert want["order"].tolist() != list(range(699, -1, -1))  # (ties keep their input order: not simply the reverse)
    placed = [r for r in recs if key(r)[0] != 4]
    unplaced = records_of(rng, 300, refs=[-1])
    want = check(gpu, unplaced + placed, 4, "unplaced first in the input")
    assert want["order"][-300:].tolist() == list(range(300)) and want["report"]["unplaced"] == 300
    want = check(gpu, unplaced, 4, "all unplaced")
    assert want["order"].tolist() == list(range(300))
    want = check(gpu, unplaced, 0, "all unplaced, a header without references")
    assert want["order"].tolist() == list(range(300))


def test_ten_thousand_records_on_one_position_keep_their_order(gpu):
    rng = np.random.default_rng(6)
    recs = records_of(rng, 10000, refs=[1], positions=[77], sizes=(36, 60))
    want = check(gpu, recs, 3, "all keys equal")
    assert want["order"].tolist() == list(range(10000)) and want["bam"].tobytes() == b"".join(recs)


@pytest.mark.parametrize("n_ref", [1, 2, 255, 256, 257, 65537])
def test_reference_counts_where_the_packed_key_gains_a_byte(gpu, n_ref):
    rng = np.random.default_rng(n_ref)
    refs = sorted({-1, 0, 1 % n_ref, n_ref // 2, max(n_ref - 2, 0), n_ref - 1})
    recs = records_of(rng, 400, n_ref=n_ref, refs=refs, positions=[0, 5, (1 << 31) - 1])
    want = check(gpu, recs, n_ref, "n_ref %d" % n_ref)
    firsts = [struct.unpack_from("<i", want["bam"], int(a) + 4)[0] for a in want["rec_index"][:-1]]
    assert set(firsts) == set(refs) and firsts[-1] == -1 and firsts[0] == 0


def test_positions_at_both_ends_and_around_the_bytes_of_the_key(gpu):
    rng = np.random.default_rng(8)
    edges = [0, (1 << 31) - 1] + [(1 << b) + d for b in (8, 16, 24) for d in (-2, -1, 0, 1)]
    recs = records_of(rng, 600, positions=edges) + [M.make_record(-1, -1, b"x"), M.make_record(-1, 0, b"unplaced, with a position")]
    perm = rng.permutation(len(recs))
    want = check(gpu, [recs[i] for i in perm], 3, "positions")
    got = {struct.unpack_from("<i", want["bam"], int(a) + 8)[0] for a in want["rec_index"][:-1]}
    assert got == set(edges) | {-1}


@pytest.mark.parametrize("sizes", [tuple(range(36, 53)), (63, 64, 65), (255, 256, 257)], ids=["36..52", "63..65", "255..257"])
def test_record_sizes_at_every_phase(gpu, sizes):
    rng = np.random.default_rng(sizes[0])
    recs = []
    for k in range(40 * len(sizes)):  # every size behind every other one: every phase of source and destination
        size = sizes[(k * 7 + k // len(sizes)) % len(sizes)]
        recs.append(M.make_record(int(rng.integers(-1, 3)), int(rng.integers(0, 9)), rng.integers(0, 256, size - 36, dtype=np.uint8).tobytes()))
    assert {len(r) for r in recs} == set(sizes)
    for bam_lead, out_lead in ((0, 0), (1, 3), (5, 2), (15, 1)):
        check(gpu, recs, 3, "sizes %r at %d -> %d" % (sizes, bam_lead, out_lead), bam_lead=bam_lead, out_lead=out_lead)


def test_one_record_of_300000_bytes_beside_ten_thousand_light_ones(gpu):
    rng = np.random.default_rng(10)
    recs = records_of(rng, 10000, sizes=(36, 90), positions=list(range(50)))
    recs.insert(4321, M.make_record(1, 25, rng.integers(0, 256, 300000 - 36, dtype=np.uint8).tobytes()))
    want = check(gpu, recs, 3, "a long record")
    assert want["report"]["longest"] == 300000
    slot = int(np.flatnonzero(want["order"] == 4321)[0])
    assert 0 < slot < 10000  # (in the middle of the output: light records on both sides of it)
    check(gpu, recs[4321:4322], 3, "a long record alone", bam_lead=7, out_lead=2)


def test_every_address_of_the_input_against_seven_of_the_output(gpu):
    rng = np.random.default_rng(11)
    recs = records_of(rng, 90, sizes=(36, 140))
    bam, ri = M.pack(recs)
    want = M.sort(bam, ri, 3)
    for bam_lead in range(16):
        for out_lead in (0, 1, 2, 3, 4, 8, 15):
            Call(gpu, bam, ri, 3, bam_lead=bam_lead, out_lead=out_lead).same_as(want, "bam at %d, out at %d mod 16" % (bam_lead, out_lead))


@pytest.mark.parametrize("want_index,want_order", [(False, True), (True, False), (False, False)])
def test_optional_outputs(gpu, want_index, want_order):
    recs = records_of(np.random.default_rng(12), 300)
    check(gpu, recs, 3, "index %d order %d" % (want_index, want_order), want_index=want_index, want_order=want_order)


# ---- BAD input ---------------------------------------------------------------------------------------------------------------
def bad_input(kind, where, count=200):
    """good records with one thing wrong in record `where` -> (bam, rec_index, n_ref)"""
    recs = records_of(np.random.default_rng(13), count)
    r = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    body = recs[r][36:]
    if kind == "short":
        recs[r] = struct.pack("<iii", 31, 0, 0) + bytes(23)  # 35 bytes, and a block_size that agrees
    elif kind == "block_size":
        recs[r] = M.make_record(0, 0, body, block_size=len(body) + 33)
    elif kind == "negative block_size":
        recs[r] = M.make_record(0, 0, body, block_size=-1)
    elif kind == "ref below -1":
        recs[r] = M.make_record(-2, 0, body)
    elif kind == "ref = n_ref":
        recs[r] = M.make_record(3, 0, body)
    elif kind == "pos below -1":
        recs[r] = M.make_record(1, -2, body)
    bam, ri = M.pack(recs)
    if kind == "index[0]":
        ri[0] = 1
    elif kind == "empty":
        ri[r + 1] = ri[r]  # (record r has no bytes; its neighbour takes them and its block_size is off)
    elif kind == "descending":
        ri[r + 1] = ri[r] - 1 if r else ri[r + 2]
    elif kind == "total short":
        bam = bam[:-1]
    elif kind == "total long":
        bam = np.concatenate((bam, np.zeros(5, np.uint8)))
    return bam, ri, 3


BAD = ([(k, w) for k in ("short", "block_size", "negative block_size", "ref below -1", "ref = n_ref", "pos below -1", "empty")
        for w in ("first", "middle", "last")] + [("descending", "first"), ("descending", "middle"), ("index[0]", "first"),
                                                 ("total short", "last"), ("total long", "last")])


@pytest.mark.parametrize("kind,where", BAD, ids=["%s, %s" % x for x in BAD])
def test_bad_input(gpu, kind, where):
    bam, ri, n_ref = bad_input(kind, where)
    bad = M.bad_records(bam, ri, n_ref)
    r = {"first": 0, "middle": 100, "last": 199}[where]
    assert bad and (r in bad or kind in ("descending", "empty")) and len(bad) <= 3, bad
    c = Call(gpu, bam, ri, n_ref)
    assert c.rc == _lib.KISS_HIP_E_INVALID
    assert c.counts() == dict(records=200, bam_bytes=bam.size, unplaced=0, longest=0, bad=len(bad), first_bad=bad[0]), (kind, where, bad)
    assert c.untouched()


def test_an_index_of_wild_values_reads_nothing_outside_the_bytes(gpu):
    recs = records_of(np.random.default_rng(14), 50)
    bam, ri = M.pack(recs)
    wild = ri.copy()
    wild[10:20] = np.uint64(1) << np.uint64(60)
    wild[30] = np.uint64(0xFFFFFFFFFFFFFFF0)
    bad = M.bad_records(bam, wild, 3)
    c = Call(gpu, bam, wild, 3)
    assert c.rc == _lib.KISS_HIP_E_INVALID and (int(c.rep.bad), int(c.rep.first_bad)) == (len(bad), bad[0]) and c.untouched()


def test_a_capacity_one_short_writes_nothing(gpu):
    recs = records_of(np.random.default_rng(15), 100)
    bam, ri = M.pack(recs)
    c = Call(gpu, bam, ri, 3, short=1)
    assert c.rc == _lib.KISS_HIP_E_INVALID
    assert c.counts() == dict(records=100, bam_bytes=bam.size, unplaced=0, longest=0, bad=0, first_bad=0) and c.untouched()


def test_more_records_than_the_ctx_sorts_are_unsupported():
    import torch
    small = kiss_amd.Context(max_n=1 << 20, device=0)
    try:
        count = 1 << 20  # (the LMS arrays of a ctx hold about 0.32 max_n entries)
        one = M.make_record(0, 0)
        bam = np.frombuffer(one * count, np.uint8)
        ri = np.arange(count + 1, dtype=np.uint64) * np.uint64(36)
        c = Call((_lib.load(), small, torch.device("cuda", 0)), bam, ri, 1)
        assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED and c.untouched()
    finally:
        small.close()


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(gpu):
    """the pattern of tests/test_fm_bam_gpu.py: a decoy of the same shapes lies in the input; a delay on the caller's stream, and
    behind it the copy that puts the real records back; the call, made while the stream is busy, must see the real ones and be
    finished on return"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    lib, ctx, dev = gpu
    rng = np.random.default_rng(16)
    recs = records_of(rng, 3000, positions=list(range(500)))
    bam, ri = M.pack(recs)
    want = model(bam, ri, 3)
    decoy = bam.copy()  # the same sizes, other places and other bodies
    for r in range(3000):
        at = int(ri[r])
        decoy[at + 4:at + 12] = np.frombuffer(struct.pack("<ii", r % 3, 3000 - r), np.uint8)
        decoy[at + 36:int(ri[r + 1])] ^= 0x5A
    assert not np.array_equal(model(decoy, ri, 3)["order"], want["order"])
    c = Call(gpu, bam, ri, 3)
    for _ in range(2):  # warm up on the null stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = c.run(lib, ctx, 3)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    c.rc = rc
    c.same_as(want, "warm-up on the null stream")
    staging = c.bam.clone()
    c.bam.copy_(torch.from_numpy(decoy))
    for v in (c.out, c.oi, c.order):
        v.fill_(INIT)
    torch.cuda.synchronize()
    assert c.run(lib, ctx, 3) == 0 and not np.array_equal(read_back(c.out), want["bam"])  # (the decoy gives other bytes)
    c.out.fill_(INIT)
    torch.cuda.synchronize()
    s = caller_stream()
    with Delayed(s, idle_ms) as delay:
        c.bam.copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.rc = c.run(lib, ctx, 3, stream=s.cuda_stream)
    got = read_back(c.out)  # (a copy on the null stream, which does not wait for s)
    delay.check("kiss_hip_bam_sort_dev")
    assert c.rc == 0 and np.array_equal(got, want["bam"])
    c.same_as(want, "on the caller's stream")


# ---- placement across 2^31 and 2^32 ---------------------------------------------------------------------------------------------
def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    """every array is valid memory wherever it lies, so a correct kernel cannot fault here; a kernel that widens the low half of
    an address with its sign would (the arena and the places of tests/test_fm_bam_gpu.py)"""
    import torch
    from tests.test_fm_sam_gpu import GUARD, PAD
    lib, ctx, dev = gpu
    vp = ctypes.c_void_p
    rng = np.random.default_rng(17)
    recs = records_of(rng, 400, sizes=(36, 300))
    bam, ri = M.pack(recs)
    want = M.sort_fast(bam, ri, 3)
    total, records = bam.size, 400
    assert total > 8192 and 8 * (records + 1) > 2048
    G = 1 << 32
    arena = torch.empty(G + (64 << 20), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    assert base % 8 == 0
    to_carry = (-base) % G  # the offset of the first multiple of 2^32 in the arena
    high = (to_carry + (1 << 31) + 4096) % G
    places = {"high half": high if high >= PAD else high + G, "low half": to_carry + 4096,
              "across a multiple of 2^32": to_carry - 1024 if to_carry >= 1024 + PAD else to_carry + G - 1024}
    d_bam, d_ri = torch.from_numpy(bam).to(dev), torch.from_numpy(ri.view(np.int64)).to(dev)
    for what, off in places.items():
        lo = (base + off) & (G - 1)
        assert {"high half": lo >= 1 << 31, "low half": lo < 1 << 31, "across a multiple of 2^32": lo == G - 1024}[what]
        assert off >= PAD and off + total + PAD <= arena.numel()
        for name in ("bam", "out", "rec_index", "out_index"):
            size = total if name in ("bam", "out") else 8 * (records + 1)
            shift = 3 if name in ("bam", "out") else 0  # (the byte arrays at an odd address as well)
            whole = arena[off - PAD:off + shift + size + PAD]
            whole.fill_(GUARD)
            view = whole[PAD + shift:PAD + shift + size]
            out = torch.full((total,), INIT, dtype=torch.uint8, device=dev)
            oi = torch.full((records + 1,), -1, dtype=torch.int64, device=dev)
            order = torch.zeros(records, dtype=torch.int32, device=dev)
            src, idx = d_bam, d_ri
            if name == "bam":
                view.copy_(d_bam)
                src = view
            elif name == "rec_index":
                view.copy_(d_ri.view(torch.uint8))
                idx = view
            elif name == "out":
                out = view
            else:
                oi = view
            rep = _lib.BamSortReport()
            rc = lib.kiss_hip_bam_sort_dev(ctx._ctx, vp(src.data_ptr()), total, vp(idx.data_ptr()), records, 3, vp(out.data_ptr()), total,
                                           vp(oi.data_ptr()), vp(order.data_ptr()), ctypes.byref(rep), None)
            assert rc == 0, (what, name)
            assert np.array_equal(out.cpu().numpy(), want["bam"]), (what, name)
            assert np.array_equal(oi.cpu().numpy().view(np.uint64).ravel(), want["rec_index"]), (what, name)
            assert np.array_equal(order.cpu().numpy().view(np.uint32), want["order"]), (what, name)
            w = whole.cpu().numpy()
            assert np.all(w[:PAD + shift] == GUARD) and np.all(w[PAD + shift + size:] == GUARD), (what, name)
    del arena


# ---- the host entry ------------------------------------------------------------------------------------------------------------
def test_the_host_entry_gives_the_same_bytes():
    import kiss_amd.bam_writer as W
    rng = np.random.default_rng(18)
    long_one = [M.make_record(0, 3, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())]
    for what, recs, n_ref in (("one record", records_of(rng, 1), 3), ("257 records", records_of(rng, 257, n_ref=300), 300),
                              ("4097 records and a long one", records_of(rng, 4097) + long_one, 3)):
        bam, ri = M.pack(recs)
        want = model(bam, ri, n_ref)
        got = W.bam_sort(bam, ri, n_ref)
        assert np.array_equal(got["bam"], want["bam"]) and np.array_equal(got["rec_index"], want["rec_index"]), what
        assert np.array_equal(got["order"], want["order"]) and {k: got["report"][k] for k in COUNTS} == want["report"], what
    bam, ri, n_ref = bad_input("pos below -1", "middle")
    with pytest.raises(_lib.KissHipError) as e:
        W.bam_sort(bam, ri, n_ref)
    assert e.value.status == _lib.KISS_HIP_E_INVALID and (e.value.report["bad"], e.value.report["first_bad"]) == (1, 100)


# ---- real records --------------------------------------------------------------------------------------------------------------
def test_the_records_of_the_shaped_batches_sorted_decode_to_the_sorted_lines(gpu):
    from tests.test_fm_bam_gpu import SHAPED
    assert len(SHAPED) == 37
    for name, b in SHAPED:
        made = B.bam_model(b)
        n_ref = len(b["ref_names"])
        bam, ri = np.frombuffer(made["bam"], np.uint8), made["rec_index"]
        want = model(bam, ri, n_ref)
        c = Call(gpu, bam, ri, n_ref)
        c.same_as(want, name)
        lines = [B.bam_to_sam(r, b["ref_names"]) for r in made["records"]]
        got = [B.bam_to_sam(r, b["ref_names"]) for r in B.split_records(read_back(c.out).tobytes())]
        assert got == [lines[r] for r in want["order"]], name
