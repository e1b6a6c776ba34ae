"""The yardstick of the byte FM-index checked where no GPU is needed: tests/fm8_model.py (suffix array by sorting suffixes,
BWT, C, sampled SA, backward search on plain arrays) against brute force (bytes.find) on the text families of the GPU test."""
import numpy as np
import pytest

from tests import fm8_model as m

SIZES = (0, 1, 2, 255, 256, 257, 700)


@pytest.mark.parametrize("n", SIZES)
def test_doubling_sa_equals_sorted_suffixes(n):
    for name, S in m.families(n, 11 + n).items():
        assert np.array_equal(m.exact_sa_doubling(S), m.exact_sa(S)), name


@pytest.mark.parametrize("sa_intv", (1, 2, 4, 7, 32))
@pytest.mark.parametrize("n", SIZES)
def test_model_search_and_locate_equal_brute_force(n, sa_intv):
    for name, S in m.families(n, 5 + n).items():
        fm = m.Model(S, sa_intv)
        assert fm.bwt.size == n + 1 and fm.bwt[fm.pri] == 0 and fm.SA[fm.pri] == 0
        assert int(fm.C[256]) == n + 1 and fm.C[0] == 1
        assert fm.sa.size == m.sizes(n, sa_intv, fm.sigma)["sa_entries"]
        pats = m.patterns_for(S, 25, 3 + n)
        assert any(len(P) > n for P in pats)
        for P in pats:
            want = m.brute(S, P)
            beg, end = fm.search(P)
            assert end - beg == len(want), (name, P)
            assert fm.locate(P) == want, (name, P)


def test_brute_counts_overlapping_hits():
    assert m.brute(b"aaaa", b"aa") == [0, 1, 2]
    assert m.brute(b"abcabc", b"bc") == [1, 4]
    assert m.brute(b"abc", b"abcd") == [] and m.brute(b"", b"a") == []
    assert m.brute(b"\x00\xff\x00", b"\x00") == [0, 2]
    counts, index, positions, checksum = m.brute_batch(b"abab", [b"ab", b"x", b"b"])
    assert counts.tolist() == [2, 0, 2] and index.tolist() == [0, 2, 2, 4] and positions.tolist() == [0, 2, 1, 3]
    assert checksum == 6


def test_pattern_families_cover_the_cases_of_the_issue():
    S = m.families(700, 1)["english"]
    pats = m.patterns_for(S, 40, 2)
    assert S in pats and any(len(P) > len(S) for P in pats) and m.absent_byte(S) in pats
    assert S[-17:] in pats and any(m.brute(S, P) == [] for P in pats) and max(len(P) for P in pats if len(P) < 700) > 100
    assert min(len(P) for P in pats) == 1
