"""The definition of the MD strings without a device (tests/fm_md_model.py; include/kiss_hip_md.h).

The model is held against statements that do not share its loop: the regular expression of the SAM specification, the sums
(numbers + letters = tend - tbeg; mismatch letters = `mismatches` and '^' letters = `del` of the record that
tests/fm_align_model.py wrote), and the inverse -- the text under the alignment rebuilt from the read, the ops and the string
alone equals the text.  Then strings worked out by hand, and every kind of bad item.
"""
import re

import numpy as np
import pytest

from tests import fm_align_model as am
from tests import fm_md_model as mm

PARAM_SETS = (dict(match=1, mismatch=4, gap_open=6, gap_extend=1), dict(match=2, mismatch=3, gap_open=0, gap_extend=1),
              dict(match=1, mismatch=1, gap_open=1, gap_extend=0), dict(match=3, mismatch=0, gap_open=0, gap_extend=0))
NO_BASE = 78


def mutated_case(rng, t):
    """a text, a read cut from it with substitutions, insertions, deletions and no-bases, a chain over the whole read"""
    n = int(rng.integers(20, 90))
    S = np.tile([0, 1], n // 2 + 1)[:n] if t % 5 == 0 else rng.integers(0, 4 if t % 3 else 2, n)  # (AC)^k every fifth
    p = int(rng.integers(0, n - 10))
    R = S[p:p + int(rng.integers(8, 50))].copy()
    for _ in range(int(rng.integers(0, 5))):
        k = int(rng.integers(0, R.size + 1))
        R = np.concatenate([R[:k], rng.integers(0, 4, int(rng.integers(0, 3))), R[k + int(rng.integers(0, 3)):]])
    if R.size == 0:
        R = S[:1].copy()
    R = np.where(rng.random(R.size) < 0.06, NO_BASE, R)
    return S, R, (0, R.size, p, min(n, p + R.size)), int(rng.integers(2, 8))


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(16)
    out = []
    for t in range(500):
        S, R, chain, band = mutated_case(rng, t)
        p = PARAM_SETS[t % len(PARAM_SETS)]
        odd = t % 2 == 1
        Rv = am.virtual_read(R, odd)  # (the alignment is of the virtual read, whichever strand it is)
        rec, ops = am.align_rows(S, Rv, *chain, band=band, **p)
        if ops:
            out.append((S, Rv, rec, ops, p))
    assert len(out) > 400
    return out


def letters_of(s):
    """(the letters outside a deletion, the letters behind a '^', the sum of the numbers)"""
    toks = mm.parse_md(s)
    return (sum(1 for t in toks if isinstance(t, str) and t[0] != "^"), sum(len(t) - 1 for t in toks if isinstance(t, str) and t[0] == "^"),
            sum(t for t in toks if isinstance(t, int)))


def test_random_alignments_regex_sums_counts_and_inverse(cases):
    adjacent = no_base = ac = 0
    for S, Rv, rec, ops, p in cases:
        s, mism, dele = mm.md_of(S, Rv, rec["rbeg"], rec["tbeg"], ops)
        assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", s), s
        single, deleted, numbers = letters_of(s)
        assert numbers + single + deleted == rec["tend"] - rec["tbeg"], (s, rec)
        assert single == mism == rec["mismatches"] and deleted == dele == rec["del"] and numbers == rec["matches"], (s, rec)
        want = "".join("ACGT"[int(c)] for c in S[rec["tbeg"]:rec["tend"]])
        assert mm.rebuild_text(Rv, rec["rbeg"], ops, s) == want, (s, ops)
        assert not mm.is_bad((rec["rbeg"], rec["rend"], rec["tbeg"], rec["tend"]), ops, len(Rv), len(S))
        adjacent += any(a[0] and b[0] for a, b in zip(ops, ops[1:]))
        no_base += any(int(x) > 3 for x in Rv[rec["rbeg"]:rec["rend"]])
        ac += len(S) > 1 and all(int(S[k]) == k % 2 for k in range(len(S)))
    assert adjacent >= 1 and no_base > 20 and ac > 50, (adjacent, no_base, ac)


def one(S, R, ops, rbeg=0, tbeg=0):
    return mm.md_of(S, R, rbeg, tbeg, ops)[0]


def test_hand_worked_strings():
    rng = np.random.default_rng(3)
    S = rng.integers(0, 4, 100)
    assert one(S, S, [(0, 100)]) == "100"
    R = S.copy()
    R[0] = (R[0] + 1) % 4
    assert one(S, R, [(0, 100)]) == "0%s99" % "ACGT"[S[0]]
    R = S.copy()
    R[99] = (R[99] + 1) % 4
    assert one(S, R, [(0, 100)]) == "99%s0" % "ACGT"[S[99]]
    #            text A  C  G  T  A  C
    S = np.array([0, 1, 2, 3, 0, 1])
    assert one(S, np.array([0, 3, 3, 3, 0, 1]), [(0, 6)]) == "1C0G3"          # two neighbouring mismatches: ..C0G..
    assert one(S, np.array([2, 2, 3, 0, 1]), [(0, 1), (2, 1), (0, 4)]) == "0A0^C4"  # a deletion right behind a mismatch
    assert one(S, np.array([0, 2, 0, 1]), [(0, 1), (2, 2), (0, 3)]) == "1^CG0T2"  # a mismatch right behind a deletion: ^CG0T
    assert one(S, np.array([3, 3]), [(2, 2), (1, 1), (2, 3), (0, 1)]) == "0^AC0^GTA0C0"  # 2D1I3D: the '^' belongs to the op
    assert one(S, np.array([0, 1, 3, 3, 2, 3]), [(0, 2), (1, 2), (0, 2)]) == "4"  # an insertion does not end a run
    assert one(S, np.array([NO_BASE, 1]), [(0, 2)]) == "0A1"                       # a no-base never matches
    assert one(S, np.array([1]), [(0, 1)], tbeg=5) == "1"                         # tend = n
    # the reverse strand: the read as sequenced is the reverse complement of text[1:5) with its last base changed
    read = np.array([3 - 0, 3 - 3, 3 - 2, 3 - 2], np.uint8)  # revcomp -> C G T A against C G T A... but base 0 is G: one mismatch
    out = mm.md(S, [read], np.array([[9, 0, 0, 4, 1, 5, 0, 0, 0, 0, 0, 0]]), [0, 0, 1], np.array([4 << 4], np.uint32), [0, 1], both_strands=True)
    assert out["strings"] == ["0C3"] and out["md_counts"].tolist() == [[1, 0]]


def test_every_bad_kind_and_the_items_that_are_not_bad():
    S = np.array([0, 1, 2, 3, 0, 1, 2, 3])
    reads = [np.array([0, 1, 2, 3]), np.array([1, 2, 3, 0, 1])]
    M = lambda ln, op=0: (ln << 4) | op  # noqa: E731
    rec = lambda rbeg, rend, tbeg, tend: [1, 0, rbeg, rend, tbeg, tend, 0, 0, 0, 0, 0, 0]  # noqa: E731
    alns = np.array([rec(0, 4, 0, 4),   # 0 good
                     rec(0, 4, 0, 4),   # 1 an op code above 2
                     rec(0, 4, 0, 4),   # 2 an op of length 0
                     rec(0, 3, 0, 4),   # 3 the read lengths do not add up
                     rec(0, 4, 0, 5),   # 4 the text lengths do not add up
                     rec(2, 6, 0, 4),   # 5 rend > L (read 1 has 5 bases)
                     rec(0, 4, 5, 9),   # 6 tend > n
                     rec(4, 0, 0, 4),   # 7 rbeg > rend
                     rec(0, 4, 4, 0),   # 8 tbeg > tend
                     rec(7, 9, 7, 9),   # 9 no ops: not bad, whatever the record holds
                     rec(0, 4, 1, 5)])  # 10 good
    ops = [[M(4)], [M(4, 3)], [M(2), M(0, 1), M(2)], [M(4)], [M(4)], [M(4)], [M(4)], [M(4)], [M(4)], [], [M(4)]]
    cigar = np.array([w for o in ops for w in o], np.uint32)
    oidx = np.concatenate([[0], np.cumsum([len(o) for o in ops])])
    cidx = [0, 5, 11]  # alignments 0..4 on read 0, 5..10 on read 1
    out = mm.md(S, reads, alns, cidx, cigar, oidx)
    assert out["strings"] == ["4"] + [""] * 9 + ["4"] and out["bad"] == 8 and out["items"] == 11
    # an aln out of range among the hits; one alignment named twice, in descending order
    out = mm.md(S, reads, alns, cidx, cigar, oidx, hits=[10, 11, 0, 10, 1 << 31, 9])
    assert out["strings"] == ["4", "", "4", "4", "", ""] and out["bad"] == 2
    assert out["md_index"].tolist() == [0, 1, 1, 2, 3, 3, 3] and out["md"] == b"444" and out["longest"] == 1


def test_an_alignment_belongs_to_the_largest_virtual_read_with_empty_segments():
    assert mm.read_of(0, [0, 0, 0, 2, 2], False) == 2 and mm.read_of(1, [0, 0, 0, 2, 2], False) == 2
    assert mm.read_of(0, [5, 6, 6, 7], False) == 0 and mm.read_of(1, [5, 6, 6, 7], False) == 2
