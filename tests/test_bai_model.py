"""tests/bai_model.py, the restatement of include/kiss_hip_bai.h, held against what an index is for: on 500 random sorted record
sets, framed by the CPU framing models (tests/bam_model.frame: stored, the even sets; tests/deflate_model.frame_report: deflated,
the odd ones) behind a framed header, the records a reader fetches through the index are exactly the ones that overlap the region,
for a grid of regions.  Then the structure of the bytes, every BAD kind, and a file of three records whose index is written out by
hand.  No GPU needed; the generators here also feed tests/test_bai_gpu.py."""
import random
import struct

import numpy as np
import pytest

from tests import bai_model as M
from tests import bam_model as B
from tests import bam_sort_model as SM
from tests import deflate_model as D

REF_LENGTHS = (40000, 300000, 5_000_000, 1 << 29)


def random_cigar(rng, reflen):
    """ops that consume reflen bases of the reference, with ops that consume none in between"""
    ops, left = [], reflen
    if rng.random() < 0.3:
        ops.append((rng.randint(1, 30), 4))
    while left:
        n = left if rng.random() < 0.5 else rng.randint(1, left)
        ops.append((n, rng.choice(M.REF_OPS)))
        left -= n
        if left and rng.random() < 0.5:
            ops.append((rng.randint(1, 9), rng.choice((1, 4, 5, 6))))
    return ops


def random_set(rng, records=None, n_ref=None):
    """-> (the records in coordinate order, n_ref, the reference lengths)"""
    n_ref = n_ref or rng.randint(1, 4)
    lengths = [rng.choice(REF_LENGTHS) for _ in range(n_ref)]
    recs = []
    for _ in range(rng.randint(1, 40) if records is None else records):
        ref = rng.randrange(n_ref)
        L = lengths[ref]
        if rng.random() < 0.1:
            recs.append((n_ref, 0, M.make_record(-1, -1, 4 | 1, name=b"u%d" % rng.randrange(1000))))
            continue
        beg = rng.randrange(L - 1) if rng.random() < 0.7 else rng.choice([x for x in (0, 16383, 16384, 131071, 131072, L - 2) if x < L - 1])
        end = min(L, beg + rng.choice([1, 1, 50, 150, 150, 16384, 20000, 200000, L]))
        name = b"n" * rng.randint(1, 9)
        if rng.random() < 0.1:  # an unmapped mate at its partner's place: the cigar is not there to be read
            recs.append((ref, beg + 1, M.make_record(ref, beg, 4 | 1 | 8, name=name, tail=bytes(rng.randrange(7)))))
        else:
            recs.append((ref, beg + 1, M.make_record(ref, beg, rng.choice((0, 16, 99)), random_cigar(rng, end - beg), name, bytes(rng.randrange(40)))))
    recs.sort(key=lambda t: t[:2])
    return [r for _, _, r in recs], n_ref, lengths


def regions(rng, recs, n_ref, lengths):
    """a grid: whole references, the ends of records, window and bin edges, one base, the space behind the last record"""
    out = []
    for ref in range(n_ref):
        L = lengths[ref]
        out.append((ref, 0, L))
        out.append((ref, L - 1, L))
        for edge in (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26):
            if edge < L:
                out += [(ref, edge - 1, edge), (ref, edge, edge + 1), (ref, edge - 1, edge + 1), (ref, max(0, edge - (1 << 14)), edge)]
        last = 0
        for rec in rng.sample(recs, min(len(recs), 6)):
            r, b, e, _, _ = M.interval(rec)
            if r == ref:
                out += [(ref, b, b + 1), (ref, e - 1, e), (ref, e, e + 1), (ref, max(0, b - 1), b), (ref, b >> 14 << 14, ((b >> 14) + 1) << 14)]
        for rec in recs:
            r, b, e, _, _ = M.interval(rec)
            if r == ref:
                last = max(last, e)
        if last < L:
            out += [(ref, last, L), (ref, last, last + 1)]
        for _ in range(4):
            b = rng.randrange(L)
            out.append((ref, b, min(L, b + rng.choice([1, 100, 16384, 100000, L]))))
    return [(r, b, e) for r, b, e in out if b < e]


def framed_file(rng, recs, deflated):
    """the records behind a framed header and in front of the end-of-file block -> (file bytes, block_bytes, block_index, file_base)"""
    bam, _ = SM.pack(recs)
    bb = rng.choice((64, 300, 0) if deflated else (7, 64, 300, 0))  # (the deflate model is slow on thousands of tiny blocks)
    head = B.frame(b"H" * rng.randint(1, 200), 0)
    if deflated:
        blocks, index, _ = D.frame_report(bam.tobytes(), bb)
        return head + blocks + B.BGZF_EOF, bb, index, len(head)
    return head + B.frame(bam.tobytes(), bb) + B.BGZF_EOF, bb, None, len(head)


def check_structure(parsed, report, records):
    placed = 0
    for t in parsed["refs"]:
        real = [b for b in t["order"] if b != M.PSEUDO_BIN]
        assert real == sorted(set(real)) and all(b < M.PSEUDO_BIN for b in real)
        assert (t["pseudo"] is not None) == bool(real) == bool(t["ioffset"])
        assert not real or t["order"][-1] == M.PSEUDO_BIN
        for chunks in t["bins"].values():
            assert chunks and all(cb < ce for cb, ce in chunks)
            assert all(chunks[i][1] <= chunks[i + 1][0] for i in range(len(chunks) - 1))
        assert t["ioffset"] == sorted(t["ioffset"])
        if t["pseudo"]:
            first, last, mapped, unmapped = t["pseudo"]
            assert first == min(c[0] for ch in t["bins"].values() for c in ch) and last == max(c[1] for ch in t["bins"].values() for c in ch)
            assert t["ioffset"][0] >= first
            placed += mapped + unmapped
    assert placed + parsed["n_no_coor"] == records == report["records"]
    assert placed == report["mapped"] + report["unmapped_placed"] and parsed["n_no_coor"] == report["no_coor"]
    assert report["bins"] == sum(len(t["bins"]) for t in parsed["refs"])
    assert report["chunks"] == sum(len(c) for t in parsed["refs"] for c in t["bins"].values())
    assert report["windows"] == sum(len(t["ioffset"]) for t in parsed["refs"])


def test_fetch_through_the_index_is_brute_force_on_500_random_sets():
    rng = random.Random(20240)
    queries = 0
    for case in range(500):
        recs, n_ref, lengths = random_set(rng)
        data, bb, index, base = framed_file(rng, recs, deflated=bool(case & 1))
        bam, ri = SM.pack(recs)
        got = M.build(bam, ri, n_ref, bb, index, base)
        assert got["status"] == "ok" and got["report"]["bai_bytes"] == len(got["bai"])
        parsed = M.parse(got["bai"])
        check_structure(parsed, got["report"], len(recs))
        reader = M.BgzfReader(data)
        for ref, beg, end in regions(rng, recs, n_ref, lengths):
            assert M.fetch(reader, parsed, ref, beg, end) == M.overlapping(recs, ref, beg, end), (case, ref, beg, end)
            queries += 1
    assert queries > 10000


def test_the_index_of_three_records_written_out_by_hand():
    # reference 0: [100, 110) in window 0 (bin 4681), then [16380, 16390) across the first window edge (bin 585 = level 17 bits);
    # reference 1: nothing; one record without a place.  name "r": l_read_name 2, so 42 bytes with one op and 38 without.
    # One stored block behind 100 bytes of header: coff = 100 = 0x64; the records start at 0, 42 = 0x2a, 84 = 0x54 (and end at 122).
    recs = [M.make_record(0, 100, 0, [(10, 0)]), M.make_record(0, 16380, 16, [(10, 0)]), M.make_record(-1, -1, 4)]
    assert [len(r) for r in recs] == [42, 42, 38]
    bam, ri = SM.pack(recs)
    by_hand = bytes.fromhex(
        "42414901" "02000000"                                             # BAI\1, n_ref = 2
        "03000000"                                                         # reference 0: two bins and the pseudo-bin
        "49020000" "01000000" "2a00640000000000" "5400640000000000"       # bin 585: the second record
        "49120000" "01000000" "0000640000000000" "2a00640000000000"       # bin 4681: the first record
        "4a920000" "02000000" "0000640000000000" "5400640000000000"       # bin 37450: the reference's records ...
        "0200000000000000" "0000000000000000"                             # ... 2 mapped, 0 unmapped
        "02000000" "0000640000000000" "2a00640000000000"                  # two windows: both records cover window 0, the second window 1
        "00000000" "00000000"                                             # reference 1: no bin, no window
        "0100000000000000")                                                # one record without a place
    got = M.build(bam, ri, 2, 0, None, 100)
    assert got["bai"] == by_hand
    assert got["report"] == dict(records=3, bam_bytes=122, bai_bytes=len(by_hand), chunks=2, bins=2, windows=2, mapped=2, unmapped_placed=0, no_coor=1,
                                 bad=0, first_bad=0)
    # the same records in blocks of 42 bytes: each record ends exactly on a block's end, at offset 0 of the next block
    got = M.parse(M.build(bam, ri, 2, 42, None, 0)["bai"])
    assert got["refs"][0]["bins"] == {4681: [(0, 73 << 16)], 585: [(73 << 16, 146 << 16)]} and got["refs"][0]["pseudo"][:2] == (0, 146 << 16)
    # ... and with a block index: [0, 50, 90, 130]
    got = M.parse(M.build(bam, ri, 2, 42, [0, 50, 90, 130], 7)["bai"])
    assert got["refs"][0]["bins"] == {4681: [(7 << 16, 57 << 16)], 585: [(57 << 16, 97 << 16)]}


def test_no_record_and_references_without_records():
    got = M.build(b"", [0], 3)
    assert got["bai"] == b"BAI\1" + struct.pack("<i", 3) + bytes(24) + bytes(8) and got["report"]["bai_bytes"] == 40
    recs = [M.make_record(1, 5, 0, [(3, 0)]), M.make_record(3, 5, 0, [(3, 0)])]
    bam, ri = SM.pack(recs)
    parsed = M.parse(M.build(bam, ri, 5)["bai"])
    assert [bool(t["bins"]) for t in parsed["refs"]] == [False, True, False, True, False]
    assert [len(t["ioffset"]) for t in parsed["refs"]] == [0, 1, 0, 1, 0]


def bad_cases():
    """name -> (records, n_ref, the BAD record); each is fine without its one fault"""
    ok = lambda pos=10: M.make_record(0, pos, 0, [(5, 0)])  # noqa: E731
    long_ops = M.make_record(0, 10, 0, [(5, 0)])
    three = [ok(), ok(11), ok(12)]
    sizes = [len(r) for r in three]
    return {
        # the kinds of rec_index itself (the model hands them to tests/bam_sort_model.py): ("index", ...) holds the index to use,
        # ("bytes", n) the bytes of bam
        "index[0]": (three, 1, 0, ("index", [1, sizes[0], sum(sizes[:2]), sum(sizes)])),
        "empty": (three, 1, 1, ("index", [0, sizes[0], sizes[0], sum(sizes)])),
        "descending": (three, 1, 1, ("index", [0, sizes[0], sizes[0] - 1, sum(sizes)])),
        "past the bytes": (three, 1, 1, ("index", [0, sizes[0], 1 << 60, sum(sizes)])),
        "total short": (three, 1, 2, ("bytes", sum(sizes) - 1)),
        "total long": (three, 1, 2, ("bytes", sum(sizes) + 5)),
        "negative block_size": ([ok(), SM.make_record(0, 10, block_size=-1), ok(11)], 1, 1),
        "short": ([ok(), struct.pack("<iii", 28, 0, 10) + bytes(20), ok(11)], 1, 1),
        "block_size": ([ok(), SM.make_record(0, 10, block_size=5), ok(11)], 1, 1),
        "refID high": ([ok(), M.make_record(1, 10, 0, [(5, 0)]), ok(11)], 1, 1),
        "refID low": ([ok(), M.make_record(-2, 10, 0, [(5, 0)]), ok(11)], 1, 1),
        "pos low": ([M.make_record(0, -2, 0, [(5, 0)]), ok(), ok(11)], 1, 0),
        "unsorted": ([ok(10), ok(12), ok(11)], 1, 2),
        "unsorted reference": ([M.make_record(1, 1, 0, [(5, 0)]), ok(), ok(11)], 2, 1),
        "unplaced first": ([M.make_record(-1, -1, 4), ok(), ok(11)], 1, 1),
        "placed at -1": ([M.make_record(0, -1, 0, [(5, 0)]), ok(), ok(11)], 1, 0),
        "cigar bytes": ([ok(), long_ops[:16] + struct.pack("<H", 2) + long_ops[18:], ok(11)], 1, 1),
        "op code": ([ok(), ok(), M.make_record(0, 11, 0, [(5, 0), (1, 9)])], 1, 2),
        "end": ([ok(), ok(), M.make_record(0, (1 << 29) - 4, 0, [(5, 0)])], 1, 2),
    }


@pytest.mark.parametrize("kind", sorted(bad_cases()))
def test_every_bad_kind(kind):
    recs, n_ref, which, *how = bad_cases()[kind]
    bam, ri = SM.pack(recs)
    assert M.build(bam, ri, n_ref)["status"] == ("ok" if how else "invalid")      # (only the index or the byte count is wrong)
    if how and how[0][0] == "index":
        ri = np.array(how[0][1], np.uint64)
    elif how:
        bam = np.concatenate((bam, np.zeros(5, np.uint8)))[:how[0][1]]
    got = M.build(bam, ri, n_ref)
    assert got["status"] == "invalid" and "bai" not in got
    bad = M.bad_records(bam, ri, n_ref)
    assert which in bad and (got["report"]["bad"], got["report"]["first_bad"], got["report"]["bai_bytes"]) == (len(bad), bad[0], 0)
    assert len(bad) == 1 or kind in ("empty", "descending", "past the bytes"), bad   # (a wrong entry is the end of one record and the start of the next)
    assert bad[0] == which


def test_the_edges_that_are_not_bad():
    # an unmapped record's cigar is not read: a wild count, wild op codes; an end of exactly 2^29; a cigar without reference bases
    recs = [M.make_record(0, 3, 4, name=b"x")[:16] + struct.pack("<HH", 65535, 4) + M.make_record(0, 3, 4, name=b"x")[20:],
            M.make_record(0, 7, 0, [(4, 1), (2, 4)]), M.make_record(0, (1 << 29) - 5, 0, [(5, 0)])]
    bam, ri = SM.pack(recs)
    got = M.build(bam, ri, 1)
    assert got["status"] == "ok" and got["report"]["windows"] == 32768 and got["report"]["unmapped_placed"] == 1
    t = M.parse(got["bai"])["refs"][0]
    assert sorted(t["bins"]) == [4681, 4681 + 32767] and len(t["bins"][4681]) == 1   # (3, 4) and (7, 8) share a bin: one chunk
    assert t["ioffset"][1:] == [t["bins"][4681 + 32767][0][0]] * 32767               # every window in between takes the one to its right


def test_the_block_index_and_the_48_bits():
    recs = [M.make_record(0, 3, 0, [(5, 0)]), M.make_record(0, 4, 0, [(5, 0)])]
    bam, ri = SM.pack(recs)
    assert M.build(bam, ri, 1, 42, [0, 60, 59])["status"] == "invalid"
    top = (1 << 48) - 1
    assert M.build(bam, ri, 1, 42, [0, 60, top - 5], 5)["status"] == "ok"
    assert M.build(bam, ri, 1, 42, [0, 60, top - 5], 6)["status"] == "unsupported"
    assert M.build(bam, ri, 1, 50, [0, 60, 1 << 48], 0)["status"] == "ok"             # (84 bytes end inside block 1: entry 2 is not used)
    assert M.build(bam, ri, 1, 42, None, (1 << 48) - 2 * 73)["status"] == "unsupported" and M.build(bam, ri, 1, 42, None, (1 << 48) - 2 * 73 - 1)["status"] == "ok"
