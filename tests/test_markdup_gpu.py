"""Duplicate templates marked on the device (kiss_hip_bam_markdup_dev / _host; include/kiss_hip_markdup.h) against
their definition, tests/markdup_model.py: every byte of bam and dup and every count of the report.  Synthetic templates whose ends
collide, at the shapes where a kernel changes its path -- record counts around the wave and the workgroup, runs of equal keys around
the wave and of 10^4 items, names of 1 and 254 bytes, cigars up to 65535 ops on both sides of what a lane sums itself, a read of
10 000 bases, ends below zero and above 2^31, reference counts around a byte of the packed end --, every byte address of bam, dup
NULL, every kind of BAD input, the caller's stream, arrays on both sides of 2^31 and across a multiple of 2^32, the host entry, and
the real records of tests/test_fm_bam_gpu.py's batches.  The arrays lie between guard bytes (tests/dev_place.py)."""
import ctypes
import struct

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bam_model as B
from tests import markdup_cases as C
from tests import markdup_model as M
from tests.dev_place import check_canaries, place, place_out, read_back

pytestmark = pytest.mark.gpu

COUNTS = ("records", "templates", "pairs", "fragments", "unmapped_templates", "ambiguous", "dup_pairs", "dup_fragments", "dup_records", "bad",
          "first_bad")
INIT = 0xEE  # what place_out leaves in an output


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 22, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


class Call:
    """one call of the device entry on placed arrays; bam is marked in place"""

    def __init__(self, gpu, bam, ri, n_ref, min_qual=15, bam_lead=1, dup_lead=3, want_dup=True, stream=None):
        lib, ctx, dev = gpu
        self.records = records = ri.size - 1
        self.given = np.array(bam, np.uint8)
        self.bam = place(self.given, bam_lead, 64, (0xA5, 0x5A, 0x3C), dev)
        self.ri = place(ri, 8, 64, 0xC3, dev)
        self.dup = place_out(records, dup_lead, 64, (0x11, 0x22, 0x33), dev, init=INIT)
        self.want_dup = want_dup
        self.rep = _lib.MarkdupReport()
        self.rc = self.run(lib, ctx, n_ref, min_qual, stream)

    def run(self, lib, ctx, n_ref, min_qual=15, stream=None):
        vp = ctypes.c_void_p
        a = lambda v: vp(v.placement.address)  # noqa: E731
        return lib.kiss_hip_bam_markdup_dev(ctx._ctx, a(self.bam) if self.bam.numel() else None, self.bam.numel(), a(self.ri), self.records, n_ref,
                                            min_qual, a(self.dup) if self.want_dup else None, ctypes.byref(self.rep), vp(stream) if stream else None)

    def counts(self):
        return {k: int(getattr(self.rep, k)) for k in COUNTS}

    def untouched(self):
        check_canaries(self.bam, self.ri, self.dup)
        return bool(np.array_equal(read_back(self.bam), self.given)) and bool(np.all(read_back(self.dup) == INIT))

    def same_as(self, want, what):
        assert self.rc == 0, (what, self.rc, self.counts())
        got = read_back(self.bam)
        if not np.array_equal(got, want["bam"]):
            k = int(np.flatnonzero(got != want["bam"])[0])
            r = int(np.searchsorted(read_back(self.ri, np.uint64), k, side="right")) - 1
            raise AssertionError("%s: bam differs at byte %d, in record %d: got 0x%02x, want 0x%02x (%d bytes differ)"
                                 % (what, k, r, int(got[k]), int(want["bam"][k]), int(np.count_nonzero(got != want["bam"]))))
        if self.want_dup:
            assert np.array_equal(read_back(self.dup), want["dup"]), what
        else:
            assert np.all(read_back(self.dup) == INIT), what
        assert self.counts() == want["report"], (what, self.counts(), want["report"])
        check_canaries(self.bam, self.ri, self.dup)


def model(bam, ri, n_ref, min_qual=15):
    """the loops for what they do in a moment, the dictionaries (held against them in tests/test_markdup_model.py) beyond"""
    return M.markdup_model(bam, ri, n_ref, min_qual, decide=M.duplicates_by_loops if ri.size <= 300 else M.duplicates_by_dicts)


def check(gpu, recs, n_ref, what, min_qual=15, **how):
    bam, ri = M.join(recs)
    want = model(bam, ri, n_ref, min_qual)
    assert "bam" in want, (what, want)
    Call(gpu, bam, ri, n_ref, min_qual, **how).same_as(want, what)
    return want


def fragment(name, pos, qual, reverse=False, ref=0, cigar=((20, "M"),), flag=0):
    return M.record(name, flag | (16 if reverse else 0), ref, pos, cigar, qual)


def flat(q, n=20):
    return bytes([q]) * n


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 4097])
def test_record_counts(gpu, count):
    rng = np.random.default_rng(count)
    recs = C.random_set(rng, count)[:count]  # (cut inside a template: its head alone is one too)
    want = check(gpu, recs, 3, "%d records" % count)
    assert want["report"]["records"] == count and (count < 63 or want["report"]["dup_records"] > 0)


@pytest.mark.parametrize("run", [1, 2, 64, 65, 10000])
def test_runs_of_pairs_on_one_key_and_of_fragments_on_one_end(gpu, run):
    rng = np.random.default_rng(run)
    scores = rng.integers(20, 24, run)  # few values: the best score is shared, the first of its holders is kept
    pairs = [r for t in range(run) for r in C.pair(b"p%d" % t, rng, 1, 500, 900, qual=flat(int(scores[t])))]
    frags = [fragment(b"f%d" % t, 77, flat(int(scores[t]))) for t in range(run)]
    others = C.random_set(rng, 30)
    want = check(gpu, others[:20] + pairs + others[20:40] + frags + others[40:], 3, "runs of %d" % run)
    assert want["report"]["dup_pairs"] >= run - 1 and want["report"]["dup_fragments"] >= run - 1
    best = int(np.flatnonzero(scores == scores.max())[0])
    kept = [t["first"] for i, t in enumerate(want["templates"]) if i not in want["dup_templates"] and t["cls"] == "pair" and t["ends"][0][1] == 500]
    assert kept == [20 + 2 * best]


def test_ten_thousand_fragments_on_a_pairs_end(gpu):
    rng = np.random.default_rng(3)
    frags = [fragment(b"f%d" % t, 500, flat(40)) for t in range(5000)] + [fragment(b"g%d" % t, 900, flat(40), reverse=True) for t in range(5000)]
    pair = C.pair(b"the pair", rng, 0, 500, 900, qual=flat(16))  # its ends: (0, 500, +) and (0, 919, -); the lowest score of all
    want = check(gpu, frags[:7000] + pair + frags[7000:], 1, "fragments on a pair's end")
    assert want["report"]["dup_fragments"] == 10000 and want["report"]["dup_pairs"] == 0 and want["report"]["dup_records"] == 10000


def test_names_of_1_and_254_bytes_and_a_name_that_is_a_prefix_of_the_next(gpu):
    long = b"n" * 253
    recs = []
    for name in (b"a", b"b", long + b"x", long + b"y", long, long[:-1], b"ab", b"abc", b"abc", b"ab"):
        recs += [fragment(name, 100, flat(30), flag=0x41), fragment(name, 300, flat(30), reverse=True, flag=0x81)]
    want = check(gpu, recs, 1, "names")
    assert want["report"]["templates"] == 9 and want["report"]["pairs"] == 8 and want["report"]["ambiguous"] == 1  # (abc twice: four mates)
    # the same names one record each: every name ends where the next one begins
    singles = [fragment(name, 100 + i, flat(30)) for i, name in enumerate((long + b"x", long + b"y", b"a", b"b", b"a", b"ab", b"a"))]
    assert check(gpu, singles, 1, "single names")["report"]["templates"] == 7
    # names that differ in every single byte position, at every phase of a word
    base = bytearray(b"0123456789abcdefghij")
    recs = [fragment(bytes(base), 5, flat(30))]
    for i in range(len(base)):
        other = bytearray(base)
        other[i] ^= 1
        recs += [fragment(bytes(other), 5, flat(30)), fragment(bytes(base), 5, flat(30))]
    assert check(gpu, recs, 1, "one byte differs", bam_lead=2)["report"]["templates"] == len(recs)


@pytest.mark.parametrize("ops", [1, 2, 8, 9, 63, 64, 65, 129, 4000, 65535])
def test_cigars_with_clips_on_both_sides_of_what_a_lane_sums(gpu, ops):
    rng = np.random.default_rng(ops)
    recs = []
    for t in range(24):
        reverse, hard = bool(t & 1), bool(t & 2)
        lead = min(int(rng.integers(0, 4)), max(ops - 1, 0))
        trail = min(int(rng.integers(0, 4)), max(ops - 1 - lead, 0))
        body = ops - lead - trail
        # clips of 1 .. 3 bases in front and behind; the body alternates M with I, D, N, =, X, P (and S and H inside, which are no clips there)
        cigar = [(int(rng.integers(1, 4)), "H" if hard and i == 0 else "S") for i in range(lead)]
        cigar += [(int(rng.integers(1, 3)), "M" if i % 2 == 0 or i == body - 1 else "IDN=XPSH"[int(rng.integers(0, 8))]) for i in range(body)]
        cigar += [(int(rng.integers(1, 4)), "H" if hard and i == trail - 1 else "S") for i in range(trail)]
        assert len(cigar) == ops
        reflen = sum(n for n, op in cigar if op in "MDN=X")
        u5 = 200000 + (int(rng.integers(0, 2)) if t >= 4 else 0)  # two places: the clips and the lengths are undone by pos
        pos = u5 - (reflen - 1 + sum(n for n, _ in cigar[ops - trail:])) if reverse else u5 + sum(n for n, _ in cigar[:lead])
        recs.append(fragment(b"c%d" % t, pos, C.quals(rng, 12), reverse=reverse, cigar=cigar))
        if ops >= 4000 and t >= 3:
            break
    recs += C.random_set(rng, 20)
    want = check(gpu, recs, 3, "%d ops" % ops)
    assert {t["ends"][0][1] for t in want["templates"][:4]} <= {200000, 200001} and want["report"]["dup_fragments"] >= 2


def test_a_cigar_of_nothing_but_clips(gpu):
    recs = [fragment(b"a", 100, flat(30, 5), cigar=((2, "H"), (3, "S"))), fragment(b"b", 95, flat(30), reverse=False),
            fragment(b"c", 100, flat(30, 5), reverse=True, cigar=((2, "H"), (3, "S"))), fragment(b"d", 85, flat(30), reverse=True),
            fragment(b"e", 100, flat(30, 10), cigar=tuple([(1, "S")] * 10))]
    want = check(gpu, recs, 1, "clips alone")
    assert [t["ends"][0] for t in want["templates"]] == [(0, 95, 0), (0, 95, 0), (0, 104, 1), (0, 104, 1), (0, 90, 0)]


def test_ends_below_zero_and_above_2_31(gpu):
    big = (1 << 31) - 1
    recs = []
    for t, (pos, cigar, reverse) in enumerate([(2, ((5, "H"), (1, "M")), False), (-1, ((2, "H"), (1, "M")), False), (0, ((3, "S"), (1, "M")), False),
                                               (big, ((10, "M"), (7, "H")), True), (big - 7, ((24, "M"),), True), (big, ((1, "M"),), False),
                                               (big, ((1, "M"),), True), (0, (((1 << 28) - 1, "H"),) * 15 + ((1, "M"),), False),
                                               (big, ((1, "M"),) + ((1 << 27, "H"),) * 14, True), (1, ((1, "M"),), False)]):
        n = sum(k for k, op in cigar if op in "MS")
        recs += [fragment(b"u%d" % t, pos, flat(30 - t, n), reverse=reverse, cigar=cigar, ref=1)]
        recs += [fragment(b"v%d" % t, pos, flat(20, n), reverse=reverse, cigar=cigar, ref=1)]
    want = check(gpu, recs, 2, "ends")
    ends = [t["ends"][0][1] for t in want["templates"]]
    assert min(ends) == -15 * ((1 << 28) - 1) and max(ends) == big + 14 * (1 << 27) and ends[0] == ends[2] == ends[4] == -3
    assert want["report"]["dup_fragments"] == 10 + 2 + 1  # every v; the two u that share -3 with a better one, and the one at 2^31 + 15


def test_both_strands_all_four_combinations_and_the_mates_swapped(gpu):
    rng = np.random.default_rng(5)
    recs = []
    for t, (r1, r2) in enumerate([(False, False), (False, True), (True, False), (True, True)]):
        for copy in range(3):
            recs += C.pair(b"s%d.%d" % (t, copy), rng, 0, 100, 300, r1, r2, swap=copy == 1, qual=flat(30 - copy))
        # the mates exchanged: the first mate at 300 with the second one's strand, the second at 100
        recs += [fragment(b"x%d" % t, 100, flat(20), reverse=r1, flag=0x81), fragment(b"x%d" % t, 300, flat(20), reverse=r2, flag=0x41)]
    want = check(gpu, recs, 1, "strands")
    assert want["report"]["pairs"] == 16 and want["report"]["dup_pairs"] == 12
    assert len({tuple(t["ends"]) for t in want["templates"]}) == 4


@pytest.mark.parametrize("n_ref", [1, 2, 257])
def test_reference_counts(gpu, n_ref):
    rng = np.random.default_rng(n_ref)
    recs = C.random_set(rng, 300, n_ref=n_ref)
    if n_ref > 2:  # the same places on the last reference and on the one that differs from it in the ninth bit
        recs += [r for ref in (0, 255, 256) for c in range(2) for r in C.pair(b"r%d.%d" % (ref, c), rng, ref, 100, 130)]
    recs += [fragment(b"fa", 7, flat(30), ref=n_ref - 1), fragment(b"fb", 7, flat(20), ref=n_ref - 1)]
    want = check(gpu, recs, n_ref, "n_ref %d" % n_ref)
    assert want["report"]["dup_pairs"] > 0 and want["report"]["dup_fragments"] > 0


def test_qualities_at_the_threshold_and_score_ties(gpu):
    recs = []
    for t, q in enumerate([bytes([14] * 20), bytes([15] * 20), bytes([14] * 19 + [15]), bytes([0xFF] * 20), bytes([0xFF] * 19 + [16]),
                           bytes([0] * 20), bytes([254] * 20), bytes([15] * 20), bytes([255] * 10 + [254] * 10)]):
        recs.append(fragment(b"q%d" % t, 10, q))
    for mq in (15, 14, 16, 0, 255, 254, 1000):
        want = check(gpu, recs, 1, "min_qual %d" % mq, min_qual=mq)
        assert want["report"]["dup_fragments"] == 8
    want = check(gpu, recs, 1, "min_qual 15")
    assert [t["score"] for t in want["templates"]] == [0, 300, 15, 0, 16, 0, 254 * 20, 300, 2540] and 6 not in want["dup_templates"]
    assert model(*M.join(recs), 1, 255)["dup_templates"] == list(range(1, 9))  # nothing counts: all tie, the first is kept


def test_one_read_of_10000_bases_beside_ten_thousand_light_ones(gpu):
    rng = np.random.default_rng(7)
    recs = C.random_set(rng, 6000)[:10000]
    long_q = C.quals(rng, 10000, 0, 60)
    recs.insert(4321, M.record(b"long one", 0, 1, 7777, ((10000, "M"),), long_q))
    recs.insert(4322, M.record(b"long too", 0, 1, 7780, ((3, "S"), (9994, "M"), (3, "S")), long_q[:-1] + bytes([(long_q[-1] + 20) % 60])))
    recs.insert(9000, M.record(b"257 bases", 0x10, 1, 8100, ((257, "M"),), C.quals(rng, 257)))
    recs.insert(9001, M.record(b"256 bases", 0x10, 1, 8101, ((256, "M"),), C.quals(rng, 256)))
    want = check(gpu, recs, 3, "a long read")
    long_ones = [t for t in want["templates"] if t["first"] in (4321, 4322)]
    assert len(long_ones) == 2 and abs(long_ones[0]["score"] - long_ones[1]["score"]) <= 60
    assert sum(int(want["dup"][r]) for r in (4321, 4322)) == 1 and sum(int(want["dup"][r]) for r in (9000, 9001)) == 1


def test_bam_at_every_address_mod_16_and_dup_at_four(gpu):
    rng = np.random.default_rng(8)
    recs = C.random_set(rng, 50) + [M.record(b"w", 0, 0, 7, ((300, "M"),), C.quals(rng, 300)), M.record(b"w2", 0, 0, 7, ((301, "M"),), C.quals(rng, 301))]
    bam, ri = M.join(recs)
    want = model(bam, ri, 3)
    assert want["report"]["dup_records"] > 10
    for bam_lead in range(16):
        Call(gpu, bam, ri, 3, bam_lead=bam_lead, dup_lead=bam_lead % 4).same_as(want, "bam at %d mod 16" % bam_lead)


def test_dup_null(gpu):
    check(gpu, C.random_set(np.random.default_rng(9), 200), 3, "no dup", want_dup=False)


# ---- BAD input ---------------------------------------------------------------------------------------------------------------
def bad_input(kind, where, count=200):
    """good records with one thing wrong in record `where` -> (bam, rec_index, n_ref)"""
    rng = np.random.default_rng(13)
    recs = C.random_set(rng, count)[:count]
    r = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    good = M.record(b"bad one", 0, 0, 50, ((20, "M"),), flat(30))
    edit = bytearray(good)
    if kind == "short":
        edit = bytearray(struct.pack("<iii", 31, 0, 0) + bytes(23))  # 35 bytes, and a block_size that agrees
    elif kind == "block_size":
        edit[0:4] = struct.pack("<i", len(good) - 3)
    elif kind == "ref below -1":
        edit[4:8] = struct.pack("<i", -2)
    elif kind == "ref = n_ref":
        edit[4:8] = struct.pack("<i", 3)
    elif kind == "pos below -1":
        edit[8:12] = struct.pack("<i", -2)
    elif kind == "no name":
        edit[12] = 0
    elif kind == "op code 9":
        edit[36 + 8:36 + 12] = struct.pack("<I", 20 << 4 | 9)
    elif kind == "op code 15 in a long cigar":
        cigar = [(1, "M")] * 70
        cigar[69] = (1, 15)
        edit = bytearray(M.record(b"bad one", 4, -1, -1, cigar, flat(30)))  # (an unmapped record: its cigar is checked all the same)
    elif kind == "l_seq one more":
        edit[20:24] = struct.pack("<I", 21)
    elif kind == "l_seq 2^32 - 1":
        edit[20:24] = struct.pack("<I", 0xFFFFFFFF)
    elif kind == "n_cigar_op 65535":
        edit[16:18] = struct.pack("<H", 65535)
    elif kind == "l_read_name past the record":
        edit[12] = 255
    elif kind == "u5 below -2^32":
        edit = bytearray(M.record(b"bad one", 0, 0, 0, (((1 << 28) - 1, "H"),) * 17 + ((1, "M"),), b"\x1e"))
    elif kind == "u5 2^32":
        edit = bytearray(M.record(b"bad one", 16, 0, 0, ((1, "M"),) + (((1 << 28) - 1, "H"),) * 17, b"\x1e"))
    recs[r] = bytes(edit)
    bam, ri = M.join(recs)
    if kind == "index[0]":
        ri[0] = 1
    elif kind == "empty":
        ri[r + 1] = ri[r]
    elif kind == "total short":
        bam = bam[:-1]
    elif kind == "total long":
        bam = np.concatenate((bam, np.zeros(5, np.uint8)))
    return bam, ri, 3


BAD = ([(k, w) for k in ("short", "block_size", "ref below -1", "ref = n_ref", "pos below -1", "no name", "op code 9", "op code 15 in a long cigar",
                         "l_seq one more", "l_seq 2^32 - 1", "n_cigar_op 65535", "l_read_name past the record", "u5 below -2^32", "u5 2^32", "empty")
        for w in ("first", "middle", "last")] + [("index[0]", "first"), ("total short", "last"), ("total long", "last")])


@pytest.mark.parametrize("kind,where", BAD, ids=["%s, %s" % x for x in BAD])
def test_bad_input(gpu, kind, where):
    bam, ri, n_ref = bad_input(kind, where)
    want = M.markdup_model(bam, ri, n_ref)
    r = {"first": 0, "middle": 100, "last": 199}[where]
    assert "bam" not in want and 1 <= want["report"]["bad"] <= 3, want
    bad, _ = M.bad_records(bam, ri, n_ref)
    assert r in bad or kind == "empty"
    c = Call(gpu, bam, ri, n_ref)
    assert c.rc == _lib.KISS_HIP_E_INVALID
    assert c.counts() == dict({k: 0 for k in COUNTS}, **want["report"]), (kind, where, want)
    assert c.untouched()


def test_an_index_of_wild_values_reads_nothing_outside_the_bytes(gpu):
    bam, ri = M.join(C.random_set(np.random.default_rng(14), 40)[:50])
    wild = ri.copy()
    wild[10:20] = np.uint64(1) << np.uint64(60)
    wild[30] = np.uint64(0xFFFFFFFFFFFFFFF0)
    bad, _ = M.bad_records(bam, wild, 3)
    c = Call(gpu, bam, wild, 3)
    assert c.rc == _lib.KISS_HIP_E_INVALID and (int(c.rep.bad), int(c.rep.first_bad)) == (len(bad), bad[0]) and c.untouched()


def test_more_records_than_the_ctx_sorts_and_too_many_references_are_unsupported(gpu):
    import torch
    small = kiss_amd.Context(max_n=1 << 20, device=0)
    try:
        count = 1 << 20  # (the LMS arrays of a ctx hold about 0.32 max_n entries)
        one = M.record(b"", 4, -1, -1, (), b"")
        assert len(one) == 37
        bam = np.frombuffer(one * count, np.uint8)
        ri = np.arange(count + 1, dtype=np.uint64) * np.uint64(37)
        c = Call((_lib.load(), small, torch.device("cuda", 0)), bam, ri, 1)
        assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED and c.untouched()
    finally:
        small.close()
    bam, ri = M.join(C.random_set(np.random.default_rng(15), 10))
    c = Call(gpu, bam, ri, 1 << 30)
    assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED and c.untouched()
    Call(gpu, bam, ri, (1 << 30) - 1).same_as(model(bam, ri, (1 << 30) - 1), "the most references")


# ---- the caller's stream -----------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(gpu):
    """the pattern of tests/test_bam_sort_gpu.py: a decoy of the same shapes lies in bam; a delay on the caller's stream, and behind
    it the copy that puts the real records back; the call, made while the stream is busy, must see the real ones and be finished on
    return"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    lib, ctx, dev = gpu
    rng = np.random.default_rng(16)
    bam, ri = M.join(C.random_set(rng, 2000))
    want = model(bam, ri, 3)
    decoy = bam.copy()  # the same sizes and names; every record at a place of its own, so that nothing is a duplicate
    for r in range(ri.size - 1):
        decoy[int(ri[r]) + 8:int(ri[r]) + 12] = np.frombuffer(struct.pack("<i", 100000 + 100 * r), np.uint8)
    want_decoy = model(decoy, ri, 3)
    assert want["report"]["dup_records"] > 500 and want_decoy["report"]["dup_records"] == 0
    c = Call(gpu, bam, ri, 3)
    c.same_as(want, "on the null stream")
    staging = torch.from_numpy(bam).to(dev)
    for _ in range(2):  # the second call is the idle duration
        c.bam.copy_(staging)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = c.run(lib, ctx, 3)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0
    c.bam.copy_(torch.from_numpy(decoy))
    c.dup.fill_(INIT)
    torch.cuda.synchronize()
    c.rc = c.run(lib, ctx, 3)
    c.same_as(want_decoy, "the decoy")
    c.dup.fill_(INIT)
    torch.cuda.synchronize()
    s = caller_stream()
    with Delayed(s, idle_ms) as delay:
        c.bam.copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.rc = c.run(lib, ctx, 3, stream=s.cuda_stream)
    got = read_back(c.dup)  # (a copy on the null stream, which does not wait for s)
    delay.check("kiss_hip_bam_markdup_dev")
    assert c.rc == 0 and np.array_equal(got, want["dup"])
    c.same_as(want, "on the caller's stream")


# ---- placement across 2^31 and 2^32 ---------------------------------------------------------------------------------------------
def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    """every array is valid memory wherever it lies, so a correct kernel cannot fault here; a kernel that widens the low half of
    an address with its sign would (the arena and the places of tests/test_bam_sort_gpu.py)"""
    import torch
    from tests.test_fm_sam_gpu import GUARD, PAD
    lib, ctx, dev = gpu
    vp = ctypes.c_void_p
    rng = np.random.default_rng(17)
    bam, ri = M.join(C.random_set(rng, 300))
    want = model(bam, ri, 3)
    total, records = bam.size, ri.size - 1
    assert total > 8192 and 8 * (records + 1) > 2048 and records > 256
    G = 1 << 32
    arena = torch.empty(G + (64 << 20), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    assert base % 8 == 0
    to_carry = (-base) % G  # the offset of the first multiple of 2^32 in the arena
    high = (to_carry + (1 << 31) + 4096) % G
    places = {"high half": high if high >= PAD else high + G, "low half": to_carry + 4096,
              "across a multiple of 2^32": to_carry - 256 if to_carry >= 256 + PAD else to_carry + G - 256}
    d_bam, d_ri = torch.from_numpy(bam).to(dev), torch.from_numpy(ri.view(np.int64)).to(dev)
    for what, off in places.items():
        lo = (base + off) & (G - 1)
        assert {"high half": lo >= 1 << 31, "low half": lo < 1 << 31, "across a multiple of 2^32": lo == G - 256}[what]
        assert off >= PAD and off + total + PAD <= arena.numel()
        for name in ("bam", "rec_index", "dup"):
            size = {"bam": total, "rec_index": 8 * (records + 1), "dup": records}[name]
            shift = 0 if name == "rec_index" else 3  # (the byte arrays at an odd address as well)
            whole = arena[off - PAD:off + shift + size + PAD]
            whole.fill_(GUARD)
            view = whole[PAD + shift:PAD + shift + size]
            marked, idx = d_bam.clone(), d_ri
            dup = torch.full((records,), INIT, dtype=torch.uint8, device=dev)
            if name == "bam":
                view.copy_(d_bam)
                marked = view
            elif name == "rec_index":
                view.copy_(d_ri.view(torch.uint8))
                idx = view
            else:
                dup = view
            rep = _lib.MarkdupReport()
            rc = lib.kiss_hip_bam_markdup_dev(ctx._ctx, vp(marked.data_ptr()), total, vp(idx.data_ptr()), records, 3, 15, vp(dup.data_ptr()),
                                              ctypes.byref(rep), None)
            assert rc == 0, (what, name)
            assert np.array_equal(marked.cpu().numpy(), want["bam"]), (what, name)
            assert np.array_equal(dup.cpu().numpy(), want["dup"]), (what, name)
            assert {k: int(getattr(rep, k)) for k in COUNTS} == want["report"], (what, name)
            w = whole.cpu().numpy()
            assert np.all(w[:PAD + shift] == GUARD) and np.all(w[PAD + shift + size:] == GUARD), (what, name)
    del arena


# ---- the host entry ------------------------------------------------------------------------------------------------------------
def test_the_host_entry_gives_the_same_bytes():
    import kiss_amd.bam_writer as W
    rng = np.random.default_rng(18)
    for what, recs, n_ref in (("one record", C.random_set(rng, 1)[:1], 3), ("300 templates", C.random_set(rng, 300, n_ref=300), 300),
                              ("4000 templates", C.random_set(rng, 4000), 3)):
        bam, ri = M.join(recs)
        want = model(bam, ri, n_ref, 17)
        got = W.bam_markdup(bam.tobytes(), ri, n_ref, min_qual=17)
        assert np.array_equal(got["bam"], want["bam"]) and np.array_equal(got["dup"], want["dup"]), what
        assert {k: got["report"][k] for k in COUNTS} == want["report"], what
    got = W.bam_markdup(b"", np.zeros(1, np.uint64), 3)
    assert got["bam"].size == 0 and got["dup"].size == 0 and got["report"]["records"] == 0
    bam, ri, n_ref = bad_input("op code 9", "middle")
    with pytest.raises(_lib.KissHipError) as e:
        W.bam_markdup(bam, ri, n_ref)
    assert e.value.status == _lib.KISS_HIP_E_INVALID and (e.value.report["bad"], e.value.report["first_bad"]) == (1, 100)


# ---- real records --------------------------------------------------------------------------------------------------------------
def test_the_records_of_the_shaped_batches(gpu):
    from tests.test_fm_bam_gpu import SHAPED
    assert len(SHAPED) == 37
    marked = 0
    for name, b in SHAPED:
        made = B.bam_model(b)
        n_ref = len(b["ref_names"])
        bam, ri = np.frombuffer(made["bam"], np.uint8), made["rec_index"]
        want = model(bam, ri, n_ref)
        assert "bam" in want, name
        Call(gpu, bam, ri, n_ref).same_as(want, name)
        # every batch once more, behind itself under other names' absence: the second copy of every template is a duplicate
        twice = np.concatenate((bam, bam))
        ri2 = np.concatenate((ri, ri[1:] + ri[-1]))
        want2 = model(twice, ri2, n_ref)
        Call(gpu, twice, ri2, n_ref).same_as(want2, name + ", twice")
        marked += want2["report"]["dup_records"]
    assert marked > 100
