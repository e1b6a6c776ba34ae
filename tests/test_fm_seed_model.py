"""The model of the seeds (tests/fm_seed_model.py) against the definitions it stands for, without a GPU: ms by binary search
equals ms length by length, the end rule equals the maximal elements under containment, a no-base is in no match, and the
virtual reads are what both_strands says."""
import numpy as np
import pytest

from tests import fm_seed_model as sm
from tests import gen

TEXTS = {
    "genome": lambda: gen.genome_like(6000, 5),
    "periodic": lambda: gen.periodic(3000, 7, 1, mutations=12),
    "iid": lambda: gen.iid(4000, 2),
    "allA": lambda: np.zeros(500, np.uint8),
    "n0": lambda: np.zeros(0, np.uint8),
    "n1": lambda: np.array([2], np.uint8),
    "n5": lambda: np.array([0, 1, 0, 1, 3], np.uint8),
}
PARAMS = ((1, 0), (19, 0), (12, 32), (7, 7), (3, 5))


def reads_for(S, seed):
    rng = np.random.default_rng(seed)
    out = []
    for L in (1, 2, 9, 31, 65):
        out.append(rng.integers(0, 4, L, dtype=np.uint8))
        if S.size >= L:
            p = int(rng.integers(0, S.size - L + 1))
            cut = S[p:p + L].copy()
            out.append(cut.copy())
            for _ in range(1 + L // 20):
                j = int(rng.integers(0, L))
                cut[j] = (cut[j] + 1 + rng.integers(0, 3)) & 3
            out.append(cut)
            nb = S[p:p + L].copy()
            nb[L // 2] = 4
            out.append(nb)
    return out


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_rule_equals_maximal_elements(name):
    S = TEXTS[name]()
    T = sm.text_bytes(S)
    cases = 0
    for R in reads_for(S, 3):
        for min_len, max_len in PARAMS:
            ms = sm.ms_of(T, R, max_len)
            assert np.array_equal(ms, sm.ms_brute(T, R, max_len))
            start = np.arange(1, R.size + 1) - ms
            assert np.all(np.diff(start) >= 0)  # start is monotone
            by_rule = sm.seeds_from_ms(ms, min_len)
            assert by_rule == sm.seeds_by_enumeration(T, R, min_len, max_len), (name, R.tolist(), min_len, max_len)
            assert all(a[0] < b[0] for a, b in zip(by_rule, by_rule[1:]))  # ascending e is strictly ascending start
            cases += 1
    assert cases >= 25


def test_no_base_is_in_no_match():
    S = gen.iid(3000, 8)
    T = sm.text_bytes(S)
    R = S[100:160].copy()
    assert sm.seeds_from_ms(sm.ms_of(T, R), 19) == [(0, 60)]
    R[30] = 78  # 'N' & 3 == 2: the pattern calls would read it as G
    ms = sm.ms_of(T, R)
    assert ms[30] == 0 and ms[29] == 30 and ms[59] == 29
    assert sm.seeds_from_ms(ms, 19) == [(0, 30), (31, 29)]
    for v in (4, 7, 255):
        assert not sm.ms_of(T, np.full(12, v, np.uint8)).any()
    ends = S[200:240].copy()
    ends[0] = ends[-1] = 4
    assert sm.seeds_from_ms(sm.ms_of(T, ends), 19) == [(1, 38)]
    assert sm.lf_pairs_of(ends, sm.ms_of(T, ends)) == sum(range(1, 39))  # every walk stops at the no-base: no pair wasted


def test_virtual_reads_of_both_strands():
    R = np.array([0, 1, 1, 4, 3, 2, 200], np.uint8)
    assert sm.revcomp(R).tolist() == [200, 1, 0, 4, 2, 2, 3]
    assert np.array_equal(sm.revcomp(sm.revcomp(R)), R)
    reads = [R, np.array([2], np.uint8)]
    v1, v2 = sm.virtual_reads(reads, False), sm.virtual_reads(reads, True)
    assert len(v1) == 2 and len(v2) == 4
    assert np.array_equal(v2[0], R) and np.array_equal(v2[1], sm.revcomp(R)) and v2[3].tolist() == [1]
    # a read cut from the reverse strand is found on the virtual read 2 q + 1, in that read's coordinates
    S = gen.iid(2000, 4)
    cut = sm.revcomp(S[500:540])
    b = sm.Batch(S, [cut], True)
    got = b.seeds(19, 0)
    assert got["seed_index"].tolist()[-2:] == [got["seed_index"][1], got["len"].size]
    k = int(got["seed_index"][1])
    assert (int(got["start"][k]), int(got["len"][k])) == (0, 40) and 500 in got["positions"][got["pos_index"][k]:got["pos_index"][k + 1]]


def test_batch_layout_and_max_occ():
    S = np.zeros(300, np.uint8)
    b = sm.Batch(S, [np.zeros(10, np.uint8), np.ones(4, np.uint8), np.zeros(1, np.uint8)], False)
    assert b.bases == 15 and b.ms.tolist() == list(range(1, 11)) + [0] * 4 + [1]
    got = b.seeds(1, 3)
    assert got["seed_index"].tolist() == [0, 1, 1, 2] and got["count"].tolist() == [291, 300]
    assert got["pos_index"].tolist() == [0, 0, 0] and got["located_seeds"] == 0 and got["positions"].size == 0
    got = b.seeds(1, 0)
    assert got["pos_index"].tolist() == [0, 291, 591] and got["positions"][:291].tolist() == list(range(291))
    assert got["positions"][291:].tolist() == list(range(300))
    assert got["checksum"] == sum(range(291)) + sum(range(300))
    assert b.lf_pairs == sum(range(1, 11)) + 4 + 1


def test_a_capped_batch_is_the_uncapped_one_cut_down():
    S = gen.genome_like(6000, 5)
    reads = reads_for(S, 9)
    whole = sm.Batch(S, reads, True)
    for max_len in (7, 32):
        a, b = whole.capped(max_len), sm.Batch(S, reads, True, max_len)
        assert np.array_equal(a.ms, b.ms) and a.lf_pairs == b.lf_pairs and a.bases == b.bases
        for x, y in zip(a.seeds(3, 5).values(), b.seeds(3, 5).values()):
            assert np.array_equal(x, y)
    f = whole.forward_only()
    g = sm.Batch(S, reads, False)
    assert np.array_equal(f.ms, g.ms) and f.lf_pairs == g.lf_pairs and (f.Q, f.V) == (g.Q, g.V)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_the_window_tables_answer_as_bytes_find_does(name):
    S = TEXTS[name]()
    T, W = sm.text_bytes(S), sm.Windows(S)
    rng = np.random.default_rng(12)
    for R in reads_for(S, 5):
        assert np.array_equal(sm.ms_of(W, R), sm.ms_of(T, R)) and np.array_equal(sm.ms_of(W, R, 7), sm.ms_of(T, R, 7))
    for L in (1, 2, 3, 5, 11, 12, 13, 20):
        for k in range(6):
            if S.size >= L and k % 2:
                p = int(rng.integers(0, S.size - L + 1))
                P = S[p:p + L].tobytes()
            else:
                P = rng.integers(0, 4 if k else 5, L, dtype=np.uint8).tobytes()
            assert np.array_equal(W.find_all(P), sm.occurrences(T, P)), (L, P)
            assert W.occurs(P) == (T.find(P) >= 0)
