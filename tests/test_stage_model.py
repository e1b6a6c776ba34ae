"""tests/stage_model.py against the CPU oracle: this is what makes the model the reference of tests/test_stage_*_gpu.py.
No GPU, no library."""
import numpy as np
import pytest

from tests import stage_cases as sc
from tests import stage_model as sm

ALL_TEXTS = sc.BIG_TEXTS + sc.TINY_TEXTS + ("tandem", "deep", "genome120k")

# ACGTT ACGTA CCGGT TAACC GGTTA ACGTA CGTAC GTACG
HAND = np.array([0, 1, 2, 3, 3, 0, 1, 2, 3, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0,
                 1, 2], dtype=np.uint8)


def test_keys_and_context_words_written_out_by_hand():
    assert HAND.size == 40 and sm.lms(HAND).tolist() == [5, 9, 16, 24, 29, 33, 37]
    # p = 0: AC GT TA CG TA CC GG TT AA CC = 1 B C 6 C 5 A F 0 5; no base in front: the empty word
    assert sm.key_of(HAND, 0) == 0x1BC6C5AF05000001
    # p = 5: AC GT AC CG GT TA AC CG GT TA = 1 B 1 6 B C 1 6 B C; in front T T G C A: marker bit 10, fields 00 01 10 11 11
    assert sm.key_of(HAND, 5) == 0x1B16BC16BC00046F
    # p = 33: AC GT AC G + 13 A behind the end = 1 B 1 8 0 0 0 0 0 0; in front T G C A T G C A A T T: marker bit 22,
    # fields (from bit 21 down) 11 11 00 00 01 10 11 00 01 10 11
    assert sm.key_of(HAND, 33) == 0x1B180000007C1B1B
    assert sm.ctx_word(HAND, 33, 15) == 0x56BC1B1B  # ... then G G C C and the marker in bit 30
    assert sm.ctx_word(HAND, 0, 15) == 1 and sm.ctx_word(HAND, 5, 15) == 0x46F
    for w in (0, 0x7C1B1B, 0x56BC1B1B, sm.TAINT, sm.TAINT | 0x7C1B1B, sm.TAINT | 0x56BC1B1B):
        assert sm.valid_ctx_word(HAND, 33, w)
    for w in (1, 0x7C1B1A, 0x3C1B1B, 0x46F, 0x16BC1B1B, 0x7C1B1B << 2):
        assert not sm.valid_ctx_word(HAND, 33, w)
    assert sm.valid_ctx_word(HAND, 5, 0x46F) and not sm.valid_ctx_word(HAND, 5, 0x06F)
    keys, pos, m_far = sm.local_list(HAND, sc.K_EXACT, 5, 34)
    assert pos.tolist() == [5, 9, 16, 24, 29, 33] and m_far == 6
    assert int(keys[0]) == 0x1B16BC16BC00046F and int(keys[-1]) == 0x1B180000007C1B1B


def test_depth_and_far():
    assert sm.depth_of(1000, 32) == 125 and sm.depth_of(1000, 256) == 375 and sm.depth_of(1000, 124) == 125
    assert sm.depth_of(1000, 125) == 250 and sm.depth_of(1000, 999) == 1000 and sm.depth_of(1000, 1000) == 0
    assert sm.depth_of(1000, sc.K_EXACT) == 0
    assert sm.is_far(1000, 32, 875) and not sm.is_far(1000, 32, 876) and sm.is_far(1000, 1000, 999)
    assert not sm.is_far(100, 32, 0)  # (D > n: no position is far)


@pytest.mark.parametrize("name", ALL_TEXTS)
def test_types_and_positions_equal_the_oracle(oracle, name):
    S = sc.text(name)
    got, _ = oracle.get_lms(S)
    assert got[-1] == S.size and np.array_equal(got[:-1], sm.lms(S))
    t = sm.types(S)
    assert t[-1] == 0 and all(t[p] == 1 and t[p - 1] == 0 for p in sm.lms(S).tolist())
    if name == "no_lms" or name == "n1":
        assert sm.lms(S).size == 0
    if name == "CA":
        assert sm.lms(S).tolist() == list(range(1, S.size - 1, 2))  # every second base, 16 in a word


def oracle_counts(S, k):
    from tests.test_multi_gpu import OracleBackend
    return OracleBackend(S, k)


@pytest.mark.parametrize("name", sc.BIG_TEXTS)
def test_counts_equal_the_oracle_stand_in_window_by_window(oracle, name):
    """every window of the GPU test at every k of the GPU test"""
    S = sc.text(name)
    n = S.size
    for k in sc.ks_of(S):
        ob = oracle_counts(S, k)
        wins = sc.windows(name, k)
        for tl in sc.tilings(n).values():
            wins.update({"tiling(%d, %d)" % w: w for w in tl})
        for wname, (lo, hi) in wins.items():
            if not wname.startswith("tiling"):
                sc.claim(name, k, wname, lo, hi)
            want = ob.classify(lo, hi)
            assert sm.counts13(S, k, lo, hi) == want, (name, k, wname, lo, hi)
            keys, pos, m_far = sm.local_list(S, k, lo, hi)
            assert np.array_equal(pos, ob._pos) and m_far == ob._mfar == want[12], (name, k, wname)
            # the oracle stand-in's key is the first 32 bases: the first 20 of them are the model's key bits 63..24
            assert np.array_equal(keys >> np.uint64(24), ob._keys >> np.uint64(24)), (name, k, wname)


@pytest.mark.parametrize("name", sc.TINY_TEXTS)
def test_counts_of_tiny_texts(oracle, name):
    S = sc.text(name)
    for k in (32, S.size - 1, S.size, sc.K_EXACT):
        ob = oracle_counts(S, k)
        for lo, hi in sc.tiny_windows(S.size):
            assert sm.counts13(S, k, lo, hi) == ob.classify(lo, hi), (name, k, lo, hi)
            assert np.array_equal(sm.local_list(S, k, lo, hi)[1], ob._pos)


def test_far_cut_texts(oracle):
    cuts = sc.far_cut_texts()
    for S, cut, q in cuts:
        L = sm.lms(S).tolist()
        assert q in L and cut == S.size - 125 and q - cut in (0, 1)
        c = sm.counts13(S, 32, 0, S.size)
        ob = oracle_counts(S, 32)
        assert c == ob.classify(0, S.size)
        for lo, hi in ((cut - 40, cut + 40), (q, q + 1)):  # the windows of the GPU test
            assert sm.counts13(S, 32, lo, hi) == ob.classify(lo, hi) and np.array_equal(sm.local_list(S, 32, lo, hi)[1], ob._pos)
        assert c[12] == sum(1 for p in L if p <= cut) and (c[12] < len(L))
        assert sm.is_far(S.size, 32, q) == (q == cut)


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", sc.SORT_TEXTS)
def test_sort_list_equals_the_oracle(oracle, name, k):
    S = sc.text(name)
    n = S.size
    far = np.array([p for p in sm.lms(S).tolist() if sm.is_far(n, k, p)], dtype=np.uint32)
    full = sm.sort_list(S, k, far)
    assert np.array_equal(full, oracle.lms_sort(S, k, far)), (name, k)
    # the oracle's whole sort: its k-ordered LMS list without the sentinel and the near-end suffixes is the same order
    sa, lms_sorted = oracle.suffix_sort(S, k, stages=True)
    lms_sorted = lms_sorted[1:]
    assert np.array_equal(lms_sorted[[sm.is_far(n, k, int(p)) for p in lms_sorted]], full), (name, k)
    rng = np.random.default_rng([n, k & 0xFFFF])
    for _ in range(2):
        sub = far[rng.random(far.size) < 0.37]
        assert np.array_equal(sm.sort_list(S, k, sub), oracle.lms_sort(S, k, sub)), (name, k)
    if k == sc.K_EXACT:
        assert np.array_equal(sm.suffix_array(S), sa)
    elif name == "tandem":
        t = sm.tied(S, k, far)
        assert len(t) > 100 and all(sm.prefix(S, k, p) in {sm.prefix(S, k, q) for q in t if q != p} for p in list(t)[:20])
