"""tests/markdup_model.py, the plain-loop statement of include/kiss_hip_markdup.h, held against a second, independent statement
(dictionaries from end and from pair of ends to lists of templates, max by (score, -index)) on 500 random record sets; cases
worked by hand; and the properties a duplicate marker has."""
import struct

import numpy as np
import pytest

from tests import markdup_cases as C
from tests import markdup_model as M

Q30 = b"\x1e" * 20  # a score of 600
Q20 = b"\x14" * 20  # 400
Q10 = b"\x0a" * 20  # nothing counts at min_qual 15


def run(recs, n_ref=2, min_qual=15, **how):
    bam, ri = M.join(recs)
    got = M.markdup_model(bam, ri, n_ref, min_qual, **how)
    if "bam" in got:
        got["flags"] = M.flags_of(got["bam"], ri)
    return got


def fwd(name, flag, pos, qual=Q30, cigar=((20, "M"),), ref=0):
    return M.record(name, flag, ref, pos, cigar, qual)


def rev(name, flag, pos, qual=Q30, cigar=((20, "M"),), ref=0):
    return M.record(name, flag | 16, ref, pos, cigar, qual)


def a_pair(name, q1=Q30, q2=Q30, p1=100, p2=300):
    return [fwd(name, 0x41, p1, q1), rev(name, 0x81, p2, q2)]


def test_random_sets_loops_against_dictionaries():
    rng = np.random.default_rng(2024)
    marked = 0
    for case in range(500):
        recs = C.random_set(rng, int(rng.integers(1, 40)), n_ref=int(rng.integers(1, 4)))
        bam, ri = M.join(recs)
        n_ref, mq = 3, int(rng.choice([0, 15, 16, 255]))
        a = M.markdup_model(bam, ri, n_ref, mq)
        b = M.markdup_model(bam, ri, n_ref, mq, decide=M.duplicates_by_dicts)
        assert a["dup_templates"] == b["dup_templates"] and a["report"] == b["report"], case
        assert np.array_equal(a["bam"], b["bam"]) and np.array_equal(a["dup"], b["dup"]), case
        marked += a["report"]["dup_records"]
    assert marked > 1000


# ---- worked by hand ------------------------------------------------------------------------------------------------------------
def test_three_copies_of_a_pair_only_the_best_stays():
    got = run(a_pair(b"a", Q20, Q20) + a_pair(b"b", Q30, Q20) + a_pair(b"c", Q20, Q10))
    assert [t["score"] for t in got["templates"]] == [800, 1000, 400]
    assert got["dup_templates"] == [0, 2] and got["dup"].tolist() == [1, 1, 0, 0, 1, 1]
    assert got["flags"] == [0x441, 0x491, 0x41, 0x91, 0x441, 0x491]
    assert got["report"] == dict(records=6, templates=3, pairs=3, fragments=0, unmapped_templates=0, ambiguous=0, dup_pairs=2, dup_fragments=0,
                                 dup_records=4, bad=0, first_bad=0)


def test_a_fragment_on_a_pairs_end_is_a_duplicate_whatever_its_score():
    got = run([fwd(b"f", 0, 100, b"\x28" * 20)] + a_pair(b"p", Q10, Q10) + [rev(b"g", 0, 300), fwd(b"h", 0, 300), rev(b"i", 0, 100)])
    # f: the pair's forward end (0, 100, +); g: its reverse end (0, 319, -); h and i: the other strand at those places
    assert [t["ends"] for t in got["templates"]] == [[(0, 100, 0)], [(0, 100, 0), (0, 319, 1)], [(0, 319, 1)], [(0, 300, 0)], [(0, 119, 1)]]
    assert got["dup_templates"] == [0, 2] and got["report"]["dup_fragments"] == 2 and got["report"]["dup_pairs"] == 0


def test_two_fragments_on_one_end_with_equal_scores_the_first_is_kept():
    got = run([fwd(b"a", 0, 50), fwd(b"b", 0, 50), fwd(b"c", 0, 50, Q20), fwd(b"d", 0, 51)])
    assert got["dup_templates"] == [1, 2]
    got = run([fwd(b"c", 0, 50, Q20), fwd(b"a", 0, 50), fwd(b"b", 0, 50)])
    assert got["dup_templates"] == [0, 2]


def test_a_soft_clip_moves_u5_onto_another_reads_end():
    got = run([fwd(b"a", 0, 100), fwd(b"b", 0, 105, Q20 + Q20[:5], ((5, "S"), (20, "M"))), fwd(b"c", 0, 105, Q20),
               fwd(b"d", 0, 103, Q20 + Q20[:2], ((1, "H"), (2, "S"), (20, "M")))])
    assert [t["ends"][0][1] for t in got["templates"]] == [100, 100, 105, 100]
    assert got["dup_templates"] == [1, 3]  # (b scores 500: 25 qualities of 20)


def test_a_reverse_read_with_a_trailing_clip():
    # 20M at 100 ends at 119; 15M2D3M5S at 100 covers 20 reference bases and its 5 clipped bases reach 124
    a = rev(b"a", 0, 100, Q30 + Q30[:5], ((20, "M"), (5, "S")))
    b = rev(b"b", 0, 105, Q20)
    c = rev(b"c", 0, 100, Q20 + Q20[:3], ((15, "M"), (2, "D"), (3, "M"), (5, "S")))
    d = rev(b"d", 0, 100, Q20, ((3, "S"), (17, "M")))  # a leading clip does not move a reverse read's end: 116
    got = run([a, b, c, d])
    assert [t["ends"][0] for t in got["templates"]] == [(0, 124, 1), (0, 124, 1), (0, 124, 1), (0, 116, 1)]
    assert got["dup_templates"] == [1, 2]


def test_secondary_supplementary_and_unmapped_mate_follow_their_template():
    keep = [fwd(b"k", 0x49, 100, b"\x28" * 20), M.record(b"k", 0x85, 0, 100, (), Q30)]
    lose = [M.record(b"l", 0x85, 0, 100, (), Q10), fwd(b"l", 0x49, 100, Q20), fwd(b"l", 0x849, 700, Q30), fwd(b"l", 0x149, 900, Q30)]
    got = run(keep + lose)
    assert [t["cls"] for t in got["templates"]] == ["fragment", "fragment"]
    assert [t["score"] for t in got["templates"]] == [800 + 600, 400]  # the unmapped mate counts, secondary and supplementary do not
    assert got["dup"].tolist() == [0, 0, 1, 1, 1, 1] and got["flags"][2:] == [0x485, 0x449, 0xC49, 0x549]
    assert got["report"]["dup_records"] == 4 and got["report"]["dup_fragments"] == 1


def test_a_stale_bit_is_cleared():
    got = run([fwd(b"a", 0x400, 10), fwd(b"b", 0x400, 10, Q20), M.record(b"u", 0x404, -1, -1, (), Q30)])
    assert got["flags"] == [0, 0x400, 4] and got["report"]["dup_records"] == 1


def test_an_ambiguous_template_is_left_alone_and_causes_nothing():
    two_singles = [fwd(b"x", 0, 100), fwd(b"x", 0, 100)]
    got = run(two_singles + [fwd(b"y", 0, 100, Q10)] + a_pair(b"z") + [fwd(b"z", 0x81, 100)] + a_pair(b"w", Q10, Q10))
    assert [t["cls"] for t in got["templates"]] == ["ambiguous", "fragment", "ambiguous", "pair"]
    assert got["dup_templates"] == [1]  # y lies on the end of the pair w; the ambiguous ones neither mark nor are marked
    assert got["report"]["ambiguous"] == 2


def test_the_key_of_a_pair_holds_both_strands_and_not_the_mates():
    base = a_pair(b"a")
    swapped = [rev(b"b", 0x41, 300, Q20), fwd(b"b", 0x81, 100, Q20)]  # the mates exchanged: the same two ends
    other = [fwd(b"c", 0x41, 100, Q20), fwd(b"c", 0x81, 300, Q20)]    # another strand: another key
    got = run(base + swapped + other)
    assert got["dup_templates"] == [1]
    assert got["templates"][0]["ends"] == got["templates"][1]["ends"] != got["templates"][2]["ends"]


def test_names_that_differ_in_the_last_byte_or_in_length_are_other_templates():
    got = run([fwd(b"ab", 0x41, 100), rev(b"ac", 0x81, 300), fwd(b"a", 0, 7), fwd(b"ab", 0, 8), fwd(b"ab", 0x100, 9)])
    assert [(t["first"], t["count"], t["cls"]) for t in got["templates"]] == [(0, 1, "fragment"), (1, 1, "fragment"), (2, 1, "fragment"),
                                                                                (3, 2, "fragment")]


def test_u5_below_zero_and_above_2_31_order_as_numbers():
    big = (1 << 31) - 1
    recs = [fwd(b"a", 0, 2, Q30[:0], ((5, "H"), (1, "M")), ref=1), fwd(b"b", 0, -1, Q30[:0], ((2, "H"), (1, "M")), ref=1),
            rev(b"c", 0, big, Q30[:0], ((10, "M"), (7, "H")), ref=1), rev(b"d", 0, big - 7, Q30[:0], ((24, "M"),), ref=1)]
    got = run(recs)
    assert [t["ends"][0][1] for t in got["templates"]] == [-3, -3, big + 16, big + 16]
    assert got["dup_templates"] == [1, 3]


def test_quality_thresholds():
    q = bytes([14, 15, 0xFF, 0, 255 - 1])
    recs = [fwd(b"a", 0, 1, q, ((5, "M"),))]
    for mq, want in ((15, 15 + 254), (14, 14 + 15 + 254), (16, 254), (0, 14 + 15 + 254), (255, 0), (300, 0)):
        assert run(recs, min_qual=mq)["templates"][0]["score"] == want, mq


# ---- BAD input -------------------------------------------------------------------------------------------------------------------
def test_bad_kinds():
    good = [fwd(b"g%d" % i, 0, i) for i in range(5)]

    def bad_at(r, rec):
        recs = list(good)
        recs[r] = rec
        return run(recs)["report"]

    no_name = bytearray(M.record(b"", 0, 0, 1, ((20, "M"),), Q30))  # l_read_name 1: the NUL alone
    assert bad_at(2, bytes(no_name))["bad"] == 0
    no_name[12] = 0
    no_name = no_name[:36] + no_name[37:]
    no_name[0:4] = struct.pack("<i", len(no_name) - 4)
    assert bad_at(2, bytes(no_name)) == dict(records=5, bad=1, first_bad=2)
    assert bad_at(4, M.record(b"x", 0, 0, 1, ((20, 9),), Q30)) == dict(records=5, bad=1, first_bad=4)
    assert bad_at(0, M.record(b"x", 4, -1, -1, ((20, 15),), Q30)) == dict(records=5, bad=1, first_bad=0)  # an unmapped record's cigar too
    assert bad_at(3, M.record(b"x", 0, 0, 1, ((20, "M"),), Q30, l_seq=21)) == dict(records=5, bad=1, first_bad=3)
    assert bad_at(1, M.record(b"x", 0, 0, 0, (((1 << 28) - 1, "H"),) * 17 + ((1, "M"),), b"\x1e")) == dict(records=5, bad=1, first_bad=1)
    assert bad_at(1, M.record(b"x", 0, 0, 0, (((1 << 28) - 1, "H"),) * 15 + ((1, "M"),), b"\x1e"))["bad"] == 0
    assert bad_at(1, M.record(b"x", 0, 2, 0, ((1, "M"),), b"\x1e")) == dict(records=5, bad=1, first_bad=1)  # refID = n_ref


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_permuting_whole_templates_changes_the_kept_one_only_on_score_ties(seed):
    rng = np.random.default_rng(seed)
    recs = C.random_set(rng, 60)
    bam, ri = M.join(recs)
    a = M.markdup_model(bam, ri, 3)
    tm = a["templates"]
    perm = [int(x) for x in rng.permutation(len(tm))]
    moved = [r for t in perm for r in recs[tm[t]["first"]:tm[t]["first"] + tm[t]["count"]]]
    b = M.markdup_model(*M.join(moved), 3)
    assert b["report"] == a["report"]
    was, now = set(a["dup_templates"]), {perm[i] for i in b["dup_templates"]}
    for t in was ^ now:  # a template whose verdict changed has a rival of its class, its key and its score
        assert any(u is not tm[t] and u["cls"] == tm[t]["cls"] and u["ends"] == tm[t]["ends"] and u["score"] == tm[t]["score"] for u in tm), t


@pytest.mark.parametrize("seed", range(6))
def test_marking_is_idempotent_and_counts_the_set_flags(seed):
    rng = np.random.default_rng(100 + seed)
    bam, ri = M.join(C.random_set(rng, 80))
    a = M.markdup_model(bam, ri, 3)
    b = M.markdup_model(a["bam"], ri, 3)
    assert np.array_equal(a["bam"], b["bam"]) and np.array_equal(a["dup"], b["dup"]) and a["report"] == b["report"]
    flags = M.flags_of(a["bam"], ri)
    assert a["report"]["dup_records"] == sum(1 for f in flags if f & 0x400) == int(a["dup"].sum())
    changed = np.flatnonzero(a["bam"] != bam)
    assert all(int(k) - int(ri[np.searchsorted(ri, k, side="right") - 1]) == 19 for k in changed)  # only the byte that holds 0x400
