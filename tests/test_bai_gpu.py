"""The BAI index built on the device (kiss_hip_bai_dev / _host; include/kiss_hip_bai.h) against its definition,
tests/bai_model.py: every byte of bai, between guard bytes (tests/dev_place.py), and every count of the report.  Synthetic sorted
records at the shapes where a kernel changes its path -- record counts around the wave and the workgroup, intervals on either side
of every bin level's edge, a record over all 32768 windows, cigars around the lane / wave threshold and at 65535 ops, references
without records, every framing -- then every BAD kind with nothing written, the caller's stream, the host entry, and the real
records of tests/test_fm_bam_gpu.py's batches sorted by kiss_hip_bam_sort_dev."""
import ctypes
import random
import struct

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bai_model as M
from tests import bam_model as B
from tests import bam_sort_model as SM
from tests.dev_place import check_canaries, place, place_out, read_back
from tests.test_bai_model import random_cigar, random_set

pytestmark = pytest.mark.gpu

COUNTS = ("records", "bam_bytes", "bai_bytes", "chunks", "bins", "windows", "mapped", "unmapped_placed", "no_coor", "bad", "first_bad")
INIT = 0xEE
STATUS = {"ok": 0, "invalid": _lib.KISS_HIP_E_INVALID, "unsupported": _lib.KISS_HIP_E_UNSUPPORTED}


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 22, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


class Call:
    """the device entry on placed arrays: cap bytes of room for bai (None: what the model says) at bai_lead mod 256"""

    def __init__(self, gpu, bam, ri, n_ref, bb=0, bi=None, base=0, cap=None, want=None, bam_lead=1, bai_lead=3, stream=None):
        lib, ctx, dev = gpu
        self.n_ref, self.bb, self.base, self.records = n_ref, bb, base, ri.size - 1
        self.want = M.build(bam, ri, n_ref, bb, bi, base) if want is None else want
        self.cap = self.want["report"]["bai_bytes"] if cap is None else cap
        self.bam = place(bam, bam_lead, 64, (0xA5, 0x5A, 0x3C), dev)
        self.ri = place(ri, 8, 64, 0xC3, dev)
        self.bi = None if bi is None else place(np.asarray(bi, np.uint64), 8, 64, 0x99, dev)
        self.bai = place_out(self.cap, bai_lead, 256, (0x11, 0x22, 0x33), dev, init=INIT)
        self.rep = _lib.BaiReport()
        self.rc = self.run(lib, ctx, stream)

    def run(self, lib, ctx, stream=None):
        vp = ctypes.c_void_p
        a = lambda v: vp(v.placement.address)  # noqa: E731
        return lib.kiss_hip_bai_dev(ctx._ctx, a(self.bam) if self.bam.numel() else None, self.bam.numel(), a(self.ri), self.records, self.n_ref, self.bb,
                                    None if self.bi is None else a(self.bi), self.base, a(self.bai) if self.cap else None, self.cap,
                                    ctypes.byref(self.rep), vp(stream) if stream else None)

    def counts(self):
        return {k: int(getattr(self.rep, k)) for k in COUNTS}

    def untouched(self):
        check_canaries(self.bai, self.bam, self.ri)
        return bool(np.all(read_back(self.bai) == INIT))

    def same(self, what):
        want = self.want
        assert self.rc == STATUS[want["status"]], (what, self.rc, self.counts())
        if want["status"] != "ok":
            assert self.untouched(), what
            assert {k: self.counts()[k] for k in ("bad", "first_bad", "bai_bytes")} == {k: want["report"][k] for k in ("bad", "first_bad", "bai_bytes")}, what
            return self
        got = read_back(self.bai).tobytes()
        if got != want["bai"]:
            k = next(i for i in range(len(got)) if got[i] != want["bai"][i])
            raise AssertionError("%s: bai differs at byte %d of %d: got %s, want %s" % (what, k, len(got), got[max(0, k - 8):k + 16].hex(),
                                                                                       want["bai"][max(0, k - 8):k + 16].hex()))
        assert self.counts() == want["report"], what
        check_canaries(self.bai, self.bam, self.ri)
        return self


def check(gpu, recs, n_ref, what, **how):
    bam, ri = SM.pack(recs)
    c = Call(gpu, bam, ri, n_ref, **how).same(what)
    assert c.want["status"] == "ok", (what, c.want["report"])
    return c.want


def rec(ref, pos, reflen=None, flag=0, cigar=None, tail=b"", name=b"q"):
    if cigar is None:  # (the length of an op has 28 bits)
        top = (1 << 28) - 1
        cigar = [] if reflen is None else [(top, 0)] * (reflen // top) + ([(reflen % top, 0)] if reflen % top else [])
    return M.make_record(ref, pos, flag, cigar, name, tail)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, 257, 4097])
def test_record_counts(gpu, count):
    recs, n_ref, _ = random_set(random.Random(count), records=count, n_ref=3)
    want = check(gpu, recs, n_ref, "%d records" % count)
    assert want["report"]["records"] == count


def test_intervals_on_either_side_of_every_level(gpu):
    recs = []
    for shift in (14, 17, 20, 23, 26):
        e = 1 << shift
        for pos, length in ((e - 2, 1), (e - 2, 2), (e - 2, 3), (e - 1, 1), (e - 1, 2), (e, 1), (e, 5), (e + 1, 1), (e - 200, 200), (e - 200, 201)):
            recs.append((pos, rec(0, pos, length)))
    recs.append(((1 << 29) - 9, rec(0, (1 << 29) - 9, 9)))                        # ends exactly at 2^29
    recs.append(((1 << 29) - 1, rec(0, (1 << 29) - 1, 1)))
    recs.sort(key=lambda t: t[0])
    want = check(gpu, [r for _, r in recs], 1, "edges")
    assert want["report"]["windows"] == 32768 and want["report"]["bins"] >= 12
    assert check(gpu, [rec(0, 0, 1 << 29)], 1, "one record over everything")["report"]["windows"] == 32768


def test_one_record_over_all_windows_beside_a_thousand_light_ones(gpu):
    rng = random.Random(3)
    light = sorted(rng.randrange(0, (1 << 29) - 300) for _ in range(1000))
    recs = [rec(0, p, rng.randint(1, 200)) for p in light]
    recs.insert(0, rec(0, 0, 1 << 29))                                            # bin 0, 32768 windows: every ioffset is its voff
    want = check(gpu, recs, 1, "a record over [0, 2^29)")
    t = M.parse(want["bai"])["refs"][0]
    assert t["bins"][0][0] == (0, len(recs[0]))
    assert set(t["ioffset"]) == {0} and len(t["ioffset"]) == 32768
    recs = recs[1:] + []                                                          # ... and one that starts in the middle of them
    recs.insert(500, rec(0, light[499], (1 << 29) - light[499]))
    check(gpu, recs, 1, "a record over the rest of the reference")


@pytest.mark.parametrize("ops", [1, 8, 9, 63, 64, 65, 65535])
def test_cigars_around_the_lane_and_the_wave(gpu, ops):
    rng = random.Random(ops)
    cigars = [[(rng.randint(1, 30), rng.choice((0, 1, 2, 3, 4, 5, 6, 7, 8))) for _ in range(ops)] for _ in range(3 if ops > 1000 else 70)]
    recs = [rec(0, 100 + i, cigar=c, tail=bytes(i % 5)) for i, c in enumerate(cigars)]
    recs += [rec(1, 5, 7), rec(1, 6, cigar=[(3, op) for op in range(9)])]         # every op code once
    want = check(gpu, recs, 2, "%d ops" % ops)
    assert want["report"]["mapped"] == len(recs)


def test_an_unmapped_record_with_a_wild_cigar_is_not_read(gpu):
    wild = rec(0, 50, flag=4 | 1 | 8)
    wild = wild[:16] + struct.pack("<HH", 65535, 4 | 1 | 8) + wild[20:]            # 65535 ops that are not there
    ops15 = rec(0, 51, flag=4, cigar=[(5, 15), (1 << 27, 0)])                     # op code 15 and 2^27 bases: not looked at
    recs = [rec(0, 50, 30), wild, ops15, rec(0, 60, 5), rec(-1, -1, flag=4), rec(-1, 7, 3)]
    want = check(gpu, recs, 1, "unmapped records")
    assert (want["report"]["unmapped_placed"], want["report"]["mapped"], want["report"]["no_coor"]) == (2, 2, 2)


@pytest.mark.parametrize("n_ref", [1, 2, 257])
def test_references_without_records_first_in_the_middle_and_last(gpu, n_ref):
    rng = random.Random(n_ref)
    for what, used in (("first", range(n_ref // 2, n_ref)), ("middle", [0, n_ref - 1]), ("last", range(0, max(1, n_ref // 2))), ("every second", range(0, n_ref, 2))):
        recs = []
        for ref in sorted(set(used)):
            for p in sorted(rng.randrange(100000) for _ in range(rng.randint(1, 5))):
                recs.append(rec(ref, p, rng.randint(1, 40000)))
        check(gpu, recs, n_ref, "n_ref %d, empty %s" % (n_ref, what))


def test_unplaced_records_none_all_and_mates_at_their_partner(gpu):
    placed = [rec(0, p, 100, flag=99) for p in range(0, 3000, 7)]
    unplaced = [rec(-1, -1, flag=77, name=b"u%d" % i) for i in range(300)]
    assert check(gpu, unplaced, 2, "all unplaced")["report"]["no_coor"] == 300
    assert check(gpu, unplaced, 0, "all unplaced, no reference")["report"]["bai_bytes"] == 16
    assert check(gpu, placed, 2, "none unplaced")["report"]["no_coor"] == 0
    mates = []
    for i, r in enumerate(placed):
        mates += [r, rec(0, 7 * i, flag=4 | 1 | 128, name=b"mate")] if i % 3 == 0 else [r]
    want = check(gpu, mates + unplaced, 2, "mates at their partner")
    assert want["report"]["unmapped_placed"] == len(mates) - len(placed)


def test_ten_thousand_records_on_one_position(gpu):
    rng = random.Random(6)
    recs = [rec(1, 77777, rng.choice((1, 1, 1, 20000)), tail=bytes(rng.randrange(9))) for _ in range(10000)]
    want = check(gpu, recs, 3, "one position")
    assert want["report"]["chunks"] > 1000 and want["report"]["bins"] == 2


def test_record_sizes_at_every_phase(gpu):
    rng = random.Random(7)
    recs, pos = [], 0
    for k in range(16 * 12):
        pos += rng.randrange(3)
        recs.append(rec(0, pos, rng.randint(1, 5), cigar=random_cigar(rng, rng.randint(1, 9)), tail=bytes((k * 7 + k // 16) % 16), name=b"n" * (1 + k % 3)))
    assert {len(r) % 16 for r in recs} == set(range(16))
    for bam_lead in (0, 1, 2, 3, 5, 15):
        check(gpu, recs, 1, "phases, bam at %d" % bam_lead, bam_lead=bam_lead)


# ---- the frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb", [1, 7, 64, 65280])
def test_block_bytes(gpu, bb):
    rng = random.Random(bb)
    recs, n_ref, _ = random_set(rng, records=40, n_ref=2)
    recs = [rec(0, 0, 3, tail=bytes(64 - 42))] + [r for r in recs if M.interval(r)[0] == 0]   # the first one ends exactly on the end of block 0 of 64
    pad = (-(sum(len(r) for r in recs) + 42)) % 448                              # bam_bytes a multiple of 1, 7 and 64
    recs.append(rec(1, 300000, 10, tail=bytes(pad)))
    recs.append(rec(1, 300001, 10, tail=bytes(200000)))                          # ... and one across many blocks
    check(gpu, recs[:-1], n_ref, "block_bytes %d, the bytes a multiple" % bb, bb=bb, base=0)
    bam, _ = SM.pack(recs[:-1])
    assert bb == 65280 or bam.size % bb == 0
    check(gpu, recs, n_ref, "block_bytes %d, behind a header" % bb, bb=bb, base=12345)


@pytest.mark.parametrize("bb", [7, 64, 0])
def test_a_block_index(gpu, bb):
    rng = random.Random(bb + 100)
    recs, n_ref, _ = random_set(rng, records=200, n_ref=3)
    bam, ri = SM.pack(recs)
    blocks = -(-bam.size // (bb or 65280))
    bi = np.cumsum([0] + [rng.choice((0, 1, 19, 65536)) for _ in range(blocks)]).astype(np.uint64)   # (never decreasing; equal entries too)
    Call(gpu, bam, ri, n_ref, bb=bb, bi=bi, base=77).same("a synthetic block index")
    top = int(bi[bam.size // (bb or 65280)])
    c = Call(gpu, bam, ri, n_ref, bb=bb, bi=bi, base=(1 << 48) - 1 - top).same("coff just below 2^48")
    assert c.rc == 0
    c = Call(gpu, bam, ri, n_ref, bb=bb, bi=bi, base=(1 << 48) - top).same("coff at 2^48")
    assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED
    if blocks >= 3:
        down = bi.copy()
        down[blocks // 2] = down[blocks // 2 - 1] - np.uint64(1) if down[blocks // 2 - 1] else down[blocks // 2 + 1] + np.uint64(1)
        c = Call(gpu, bam, ri, n_ref, bb=bb, bi=down, base=77).same("a block index that decreases")
        assert c.rc == _lib.KISS_HIP_E_INVALID and c.counts()["bad"] == 0
    c = Call(gpu, bam, ri, n_ref, bb=7, base=(1 << 48) - 38 * (bam.size // 7)).same("stored blocks, coff at 2^48")
    assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED


def test_bai_at_every_address_and_short_capacities(gpu):
    recs, n_ref, _ = random_set(random.Random(9), records=120, n_ref=3)
    bam, ri = SM.pack(recs)
    want = M.build(bam, ri, n_ref, 0, None, 5)
    for lead in range(8):
        Call(gpu, bam, ri, n_ref, base=5, want=want, bai_lead=lead).same("bai at %d mod 8" % lead)
    totals = dict(want["report"], bai_bytes=want["report"]["bai_bytes"])
    for cap in (want["report"]["bai_bytes"] - 1, 0):
        c = Call(gpu, bam, ri, n_ref, base=5, want=want, cap=cap)
        assert c.rc == _lib.KISS_HIP_E_INVALID and c.counts() == totals and c.untouched(), cap
    empty = Call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 5, cap=0)
    assert empty.rc == _lib.KISS_HIP_E_INVALID and empty.counts()["bai_bytes"] == 56


# ---- BAD input ---------------------------------------------------------------------------------------------------------------
def bad_input(kind, where, count=200):
    recs = [rec(i * 3 // count, 10 * i, 1 + i % 50, tail=bytes(i % 4)) for i in range(count)]
    r = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    ref, pos = r * 3 // count, 10 * r
    recs[r] = {"index[0]": recs[r], "empty": recs[r], "descending": recs[r], "past the bytes": recs[r], "total short": recs[r], "total long": recs[r],
               "short": struct.pack("<iii", 31, ref, pos) + bytes(23),
               "block_size": SM.make_record(ref, pos, block_size=99),
               "negative block_size": SM.make_record(ref, pos, block_size=-1),
               "ref below -1": rec(-2, pos, 5), "ref = n_ref": rec(3, pos, 5), "pos below -1": rec(ref, -2, 5),
               "placed at -1": rec(ref, -1, 5),
               "cigar bytes": recs[r][:16] + struct.pack("<H", 3) + recs[r][18:],
               "cigar bytes, many": recs[r][:16] + struct.pack("<H", 65535) + recs[r][18:],
               "op code": rec(ref, pos, cigar=[(4, 0), (1, 9)]),
               "op code, long cigar": rec(ref, pos, cigar=[(1, 0)] * 99 + [(1, 15)] + [(1, 1)] * 30),
               "end": rec(ref, pos, (1 << 29) - pos + 1),
               "end, far": rec(ref, pos, cigar=[((1 << 28) - 1, 3)] * 40)}[kind]
    bam, ri = SM.pack(recs)
    # the kinds of rec_index itself, as tests/test_bam_sort_gpu.py has them: they keep the head and the cigar from being read past bam
    if kind == "index[0]":
        ri[0] = 1
    elif kind == "empty":
        ri[r + 1] = ri[r]  # (record r has no bytes; its neighbour takes them and its block_size is off)
    elif kind == "descending":
        ri[r + 1] = ri[r] - 1 if r else ri[r + 2]
    elif kind == "past the bytes":
        ri[r + 1] = np.uint64(1) << np.uint64(60) if r else np.uint64(0xFFFFFFFFFFFFFFF0)
    elif kind == "total short":
        bam = bam[:-1]
    elif kind == "total long":
        bam = np.concatenate((bam, np.zeros(5, np.uint8)))
    return bam, ri, 3


BAD = [("index[0]", "first"), ("descending", "first"), ("descending", "middle"), ("past the bytes", "first"), ("past the bytes", "middle"),
       ("total short", "last"), ("total long", "last")]
BAD += [(k, w) for k in ("empty", "negative block_size", "short", "block_size", "ref below -1", "ref = n_ref", "pos below -1", "placed at -1", "cigar bytes", "cigar bytes, many",
                        "op code", "op code, long cigar", "end", "end, far") for w in ("first", "middle", "last")]


@pytest.mark.parametrize("kind,where", BAD, ids=["%s, %s" % x for x in BAD])
def test_bad_input(gpu, kind, where):
    bam, ri, n_ref = bad_input(kind, where)
    c = Call(gpu, bam, ri, n_ref, cap=4096).same("%s, %s" % (kind, where))
    r = {"first": 0, "middle": 100, "last": 199}[where]
    assert c.want["status"] == "invalid" and c.want["report"]["bad"] >= 1 and c.want["report"]["first_bad"] <= r, c.want["report"]
    assert c.counts()["bai_bytes"] == 0 and c.counts()["bad"] == c.want["report"]["bad"] and c.untouched()


def test_an_index_of_wild_values_reads_nothing_outside_the_bytes(gpu):
    recs = [rec(0, 10 * i, 1 + i % 50, tail=bytes(i % 4)) for i in range(50)]
    bam, ri = SM.pack(recs)
    wild = ri.copy()
    wild[10:20] = np.uint64(1) << np.uint64(60)
    wild[30] = np.uint64(0xFFFFFFFFFFFFFFF0)
    c = Call(gpu, bam, wild, 1, cap=4096).same("wild values")
    assert c.rc == _lib.KISS_HIP_E_INVALID and c.want["report"]["bad"] >= 11 and c.untouched()


def test_a_bad_record_is_reported_before_an_offset_beyond_48_bits(gpu):
    """BAD and too far at once is BAD, with stored blocks and with a block index alike, as the model has it"""
    bam, ri, n_ref = bad_input("op code", "middle")
    blocks = -(-bam.size // 64)
    far = (1 << 48) - 1
    for what, how in (("stored", dict(bb=64, base=far)), ("indexed", dict(bb=64, bi=np.arange(blocks + 1, dtype=np.uint64) * np.uint64(70), base=far))):
        c = Call(gpu, bam, ri, n_ref, cap=4096, **how).same(what)
        assert c.rc == _lib.KISS_HIP_E_INVALID and (c.counts()["bad"], c.counts()["first_bad"]) == (1, 100), what
    good = SM.pack([rec(0, 10 * i, 5) for i in range(200)])
    for what, how in (("stored", dict(bb=64, base=far)), ("indexed", dict(bb=64, bi=np.arange(-(-good[0].size // 64) + 1, dtype=np.uint64) * np.uint64(70), base=far))):
        assert Call(gpu, good[0], good[1], 1, cap=4096, **how).same(what).rc == _lib.KISS_HIP_E_UNSUPPORTED, what


def test_unsorted_by_one_swap(gpu):
    recs, n_ref, _ = random_set(random.Random(12), records=300, n_ref=3)
    keys = [SM.key_of(r, 0, n_ref) for r in recs]
    for r in (next(i for i in range(299) if keys[i] < keys[i + 1]), 150 + next(i for i in range(149) if keys[150 + i] < keys[151 + i])):
        swapped = list(recs)
        swapped[r], swapped[r + 1] = swapped[r + 1], swapped[r]
        bam, ri = SM.pack(swapped)
        c = Call(gpu, bam, ri, n_ref, cap=1 << 16).same("records %d and %d swapped" % (r, r + 1))
        assert c.rc == _lib.KISS_HIP_E_INVALID and c.counts()["first_bad"] == r + 1


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(gpu):
    """the pattern of tests/test_bam_sort_gpu.py: a decoy lies in the input; a delay on the caller's stream, and behind it the copy
    that puts the real records back; the call, made while the stream is busy, must see the real ones and be finished on return"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    lib, ctx, dev = gpu
    recs = [rec(0, 40 * i, 1 if i % 10 == 0 else 1 + i % 90, tail=bytes(i % 3)) for i in range(3000)]
    # the decoy: the same sizes and intervals, every tenth record unmapped: the same bytes of index but for the pseudo-bin's counts
    decoys = [rec(0, 40 * i, 1 if i % 10 == 0 else 1 + i % 90, flag=4 if i % 10 == 0 else 0, tail=bytes(i % 3)) for i in range(3000)]
    bam, ri = SM.pack(recs)
    decoy, _ = SM.pack(decoys)
    want, other = M.build(bam, ri, 1), M.build(decoy, ri, 1)
    assert decoy.size == bam.size and other["status"] == "ok" and other["report"]["bai_bytes"] == want["report"]["bai_bytes"] and other["bai"] != want["bai"]
    c = Call(gpu, bam, ri, 1, want=want)
    for _ in range(2):  # warm up on the null stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = c.run(lib, ctx)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    c.rc = rc
    c.same("warm-up on the null stream")
    staging = c.bam.clone()
    c.bam.copy_(torch.from_numpy(decoy))
    c.bai.fill_(INIT)
    torch.cuda.synchronize()
    assert c.run(lib, ctx) == 0 and read_back(c.bai).tobytes() == other["bai"]
    c.bai.fill_(INIT)
    torch.cuda.synchronize()
    s = caller_stream()
    with Delayed(s, idle_ms) as delay:
        c.bam.copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.rc = c.run(lib, ctx, stream=s.cuda_stream)
    got = read_back(c.bai).tobytes()  # (a copy on the null stream, which does not wait for s)
    delay.check("kiss_hip_bai_dev")
    assert c.rc == 0 and got == want["bai"]
    c.same("on the caller's stream")


# ---- the host entry ------------------------------------------------------------------------------------------------------------
def test_the_host_entry_gives_the_same_bytes():
    import kiss_amd.bam_writer as W
    rng = random.Random(18)
    for what, count, n_ref, bb in (("one record", 1, 1, 65280), ("257 records", 257, 300, 7), ("4097 records", 4097, 3, 0)):
        recs, n_ref, _ = random_set(rng, records=count, n_ref=n_ref)
        bam, ri = SM.pack(recs)
        bi = None if bb != 7 else np.arange(-(-bam.size // 7) + 1, dtype=np.uint64) * np.uint64(11)
        want = M.build(bam, ri, n_ref, bb, bi, 99)
        got = W.bam_index(bam, ri, n_ref, bb, bi, 99)
        assert got["bai"] == want["bai"] and {k: got["report"][k] for k in COUNTS} == want["report"], what
    bam, ri, n_ref = bad_input("op code", "middle")
    with pytest.raises(_lib.KissHipError) as e:
        W.bam_index(bam, ri, n_ref)
    assert e.value.status == _lib.KISS_HIP_E_INVALID and (e.value.report["bad"], e.value.report["first_bad"]) == (1, 100)


# ---- real records --------------------------------------------------------------------------------------------------------------
def test_the_records_of_the_shaped_batches_sorted_on_the_device(gpu):
    from tests.test_fm_bam_gpu import SHAPED
    import kiss_amd.bam_writer as W
    assert len(SHAPED) == 37
    BEYOND = ("big, paired 0", "big, paired 1")   # ten-digit positions: ends beyond 2^29, refused by the model and by the device
    indexed = 0
    for name, b in SHAPED:
        made = B.bam_model(b)
        n_ref = len(b["ref_names"])
        got = W.bam_sort(np.frombuffer(made["bam"], np.uint8), made["rec_index"], n_ref)
        c = Call(gpu, got["bam"], got["rec_index"], n_ref, bb=300, base=1000, cap=None).same(name)
        indexed += c.want["status"] == "ok"
        assert (c.want["status"] == "ok") == (name not in BEYOND), name
    assert indexed == 35, indexed
