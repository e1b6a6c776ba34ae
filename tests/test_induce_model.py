"""The sequential model of the induction (tests/induce_model.py) itself, on the CPU: against the oracle, against a
brute-force suffix array, its two forms against each other, and the constructed texts of tests/test_induce_paths_gpu.py
against what they claim and what the rows of the GPU grid (tests/induce_cases.py) say about them."""
import numpy as np
import pytest

from tests import induce_model as im
from tests import induce_cases as paths

K_EXACT = 0xFFFFFFFF
TEXTS = im.texts()


def _order(oracle, S, k):
    sa, lms_sorted = oracle.suffix_sort(S, k, stages=True)
    return sa, lms_sorted[1:].astype(np.int64)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_induce_equals_the_oracle(oracle, name):
    S = TEXTS[name][0]()
    for k in (32, 256, K_EXACT):
        sa, order = _order(oracle, S, k)
        msg = im.compare(im.induce(S, order), sa, None, "%s k=%d" % (name, k))
        assert msg is None, msg


def _brute_force(S):
    n = len(S)
    s = bytes(S.tolist())
    return np.asarray([n] + sorted(range(n), key=lambda i: s[i:]), dtype=np.uint32)  # a shorter suffix that is a prefix sorts first


def test_induce_equals_brute_force(oracle):
    from tests.test_suffix_sort_gpu import _random_text
    rng = np.random.default_rng(77)
    for t in range(200):
        n = int(rng.integers(1, 61))
        S = _random_text(rng, n)
        want = _brute_force(S)
        stype, lms, counts = im.types(S)
        is_lms = np.zeros(n + 1, dtype=bool)
        is_lms[lms] = True
        order = want[is_lms[want]].astype(np.int64)        # the LMS suffixes in brute-force order: no oracle involved
        assert np.array_equal(im.induce(S, order), want), S.tolist()
        assert np.array_equal(im.schedule(S, order).SA, want), S.tolist()
        assert np.array_equal(oracle.suffix_sort(S, K_EXACT), want), S.tolist()
        # types against the definition
        for i in range(n):
            assert stype[i] == (bytes(S[i:].tolist()) < bytes(S[i + 1:].tolist())), (S.tolist(), i)


def test_types_counts_and_lms_equal_the_oracle(oracle):
    for name in ("iid40k", "genome60k", "planted", "stairs_A", "blocks", "TATA", "near65"):
        S = TEXTS[name][0]()
        stype, lms, counts = im.types(S)
        lms_ref, hist = oracle.get_lms(S)
        assert np.array_equal(lms, lms_ref[:-1]), name
        assert counts[0:4] == hist[4, :4].tolist() and counts[8:12] == hist[2, :4].tolist(), name
        assert sum(counts[4:8]) == int(stype[:-1].sum())


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_schedule_is_consistent_with_induce(oracle, name):
    S = TEXTS[name][0]()
    k = TEXTS[name][1][-1]
    sa, order = _order(oracle, S, k)
    for lms_order in (order, im.shuffled_in_groups(S, order, 3)):
        sch = im.schedule(S, lms_order)
        assert np.array_equal(sch.SA, im.induce(S, lms_order)), name
        assert set(sch.writes) == {1}, name + ": a slot with no writer or two"
        assert all(w is not None for w in sch.writer)
        for c in range(4):
            assert sum(sch.chains[("L", c)]) == sch.cntL[c], name
            assert sum(sch.chains[("S", c)]) == sch.cntS[c], name
            assert sch.lms_pass[c] == sch.cntLMS[c]
        # every slot lies in the part its writer feeds
        for slot in (1, len(S) // 2, len(S)):
            sweep, seg, rnd = sch.writer[slot]
            assert sch.part_of(slot).startswith("L-part" if sweep == "L" else "S-part"), (name, slot)
    assert np.array_equal(im.schedule(S, order).SA, sa)


def test_any_grouped_order_is_accepted(oracle):
    S = TEXTS["iid40k"][0]()
    sa, order = _order(oracle, S, 256)
    shuffled = im.shuffled_in_groups(S, order, 5)
    assert sorted(shuffled.tolist()) == sorted(order.tolist()) and not np.array_equal(shuffled, order)
    assert np.array_equal(S[shuffled], S[order])           # still grouped A, C, G, T
    got = im.induce(S, shuffled)
    assert sorted(got.tolist()) == list(range(S.size + 1)) and not np.array_equal(got, sa)
    with pytest.raises(AssertionError):
        im.induce(S, order[:-1])


def test_split_near_and_depth():
    assert [im.depth_of(10_000, k) for k in (1, 32, 124, 125, 256, 1000, 9999, 10_000, K_EXACT)] == \
        [125, 125, 125, 250, 375, 1125, 10_000, 0, 0]
    S = TEXTS["iid40k"][0]()
    stype, lms, counts = im.types(S)
    for k in (32, 256, 1000):
        far, near = im.split_near(S, lms, k)
        D = im.depth_of(S.size, k)
        assert far.size + near.size == lms.size and (far + D <= S.size).all() and (near + D > S.size).all()
    far, near = im.split_near(S, lms, K_EXACT)
    assert near.size == 0
    far, near = im.split_near(S[:100], im.types(S[:100])[1], 32)     # D = 125 > n: no suffix is far
    assert far.size == 0


def test_ctx_word():
    S = np.array([3, 3, 0, 1, 2] + [1] * 20, dtype=np.uint8)
    assert im.ctx_word(S, 0) == im.EMPTY_CTX and im.ctx_word(S, 9, 0) == im.EMPTY_CTX
    assert im.ctx_word(S, 3) == 0x40 | 0x3C            # three bases: marker at bit 6, base 2 (A) in bits 1:0
    assert im.ctx_word(S, 5, 2) == 0x10 | (1 << 2) | 2  # bases 3, 4 = C, G
    w = im.ctx_word(S, 25)
    assert w >> 30 == 1 and (w & 3) == 1 and w < (1 << 31)
    rng = np.random.default_rng(1)
    v, b = rng.integers(0, 25, 100), rng.integers(0, 16, 100)
    assert im.ctx_words(S, v, b).tolist() == [im.ctx_word(S, int(x), int(y)) for x, y in zip(v, b)]
    # an induced item's word is its parent's without the nearest base
    for x in range(1, 25):
        assert im.ctx_word(S, x) >> 2 == im.ctx_word(S, x - 1, min(14, x - 1))


# ---- the constructed texts are what they claim ------------------------------------------------------------------------

def test_planted_runs():
    for name, lengths in (("planted", im.RUNS_LONG), ("planted_short", im.RUNS_SHORT)):
        S = TEXTS[name][0]()
        assert S.size <= 120_000
        runs = im.run_lengths(S)
        longer = sorted((ln, c) for a, ln, c in runs if ln >= 15)
        assert longer == sorted((ln, c) for ln in lengths for c in range(4)), name
        assert runs[0][1] >= 15 and runs[-1][1] >= 15      # one run starts at position 0, one ends at n


def test_staircase_and_giant_runs(oracle):
    for name, first in (("stairs_T", im.T_), ("stairs_A", im.A_)):
        S = TEXTS[name][0]()
        runs = im.run_lengths(S)
        assert [ln for a, ln, c in runs if ln > 1] == [1500] * 16 and runs[0] == (0, 1500, first)
        assert sum(1 for a, ln, c in runs if ln == 1) == 15 and len(runs) == 31
        sa, order = _order(oracle, S, 256)
        sch = im.schedule(S, order)
        assert max(len(r) for r in sch.chains.values()) == 1500 and max(N for r in sch.chains.values() for N in r) <= 16
    S = TEXTS["giant"][0]()
    runs = im.run_lengths(S)
    assert sorted((ln, c) for a, ln, c in runs if ln > 1000) == sorted((ln, c) for ln in im.GIANT for c in (im.A_, im.T_))
    stype = im.types(S)[0]
    for a, ln, c in runs:
        if ln > 1000:
            assert bool(stype[a]) == (c == im.A_)          # the A runs are S-type (S chains), the T runs L-type (L chains)


def test_texts_without_lms_and_two_letter_texts():
    for name in ("blocks", "blocks_rev"):
        S = TEXTS[name][0]()
        assert S.size == 2000 and im.types(S)[1].size == 0 and im.types(S)[2][0:4] == [500] * 4
    for name, letters in (("AT", (0, 3)), ("CG", (1, 2)), ("AC", (0, 1))):
        stype, lms, counts = im.types(TEXTS[name][0]())
        assert [c for c in range(4) if counts[c]] == list(letters)
        assert [c for c in range(4) if counts[8 + c]] == [letters[0]]      # LMS suffixes of the smaller letter only
    for name in ("ACAC", "TATA"):
        S = TEXTS[name][0]()
        assert im.types(S)[1].size == S.size // 2 - 1                       # every second position but the first / last


def test_tile_edge_and_near_end_texts():
    for name in TEXTS:
        if name.startswith("edge"):
            S = TEXTS[name][0]()
            stype, lms, counts = im.types(S)
            x = int(name[4:].split("_")[0])
            assert counts[8:12] == [x, 0, 0, 0], name
            assert im.split_near(S, lms, 32)[1].size == 0, name
    begins = set()
    for j in range(16):
        S = TEXTS["edge2049_A%d" % j][0]()
        begins.add((1 + im.types(S)[2][0]) % 16)                            # start of bucket C
    assert begins == set(range(16))
    for E in im.NEAR_E:
        S = TEXTS["near%d" % E][0]()
        stype, lms, counts = im.types(S)
        far, near = im.split_near(S, lms, im.NEAR_K)
        assert near.size == E and (S[near] == im.A_).all(), E
        assert far.size > 11_000


# ---- every row of the GPU file's grids has the premises it claims (the model's side of each case, no GPU) ---------------

def test_gpu_grid_premises(oracle):
    seen = set()
    for name, k, config, claim in paths.GRID:
        assert name in TEXTS and config in paths.CONFIGS and k in TEXTS[name][1], (name, k, config)
        r = paths.plan(paths.case_of(oracle, name, k), config, claim)
        if config.startswith("tiles") and not name.startswith(("edge", "blocks", "stairs")):
            assert r.tile > 0, (name, config)
        seen.add(config)
    assert seen == set(paths.CONFIGS)
    # the one-workgroup kernel's self-class loop is reached where the row says so, and only there
    c = paths.case_of(oracle, "iid40k", 256)
    assert paths.plan(c, "small_chain", "small_chain").chased > 0 and paths.plan(c, "shipped").chased == 0
    for config in ("shipped", "tiles", "cap3"):
        for name, k in paths.FORM_TEXTS[config]:
            paths.plan(paths.case_of(oracle, name, k), config)
    # giant runs: a first call of 65 535 steps that no capacity shortens, then a wide one, in both sweeps
    r = paths.plan(paths.case_of(oracle, "giant", 256), "shipped", "wide")
    assert sorted(s[3][0] for s in r.steps if s[2] == 70_000) == [im.COLLAPSE_RCAP] * 2
    # contexts of the text's own size: capacity limits the steps under the shipped thresholds
    for name, config in paths.TIGHT:
        c = paths.case_of(oracle, name, 256)
        r = paths.plan(c, config, "capacity" if config == "shipped" else None, max_n=c.n)
        assert config != "tiles" or r.tile > 0
    paths.forget_all()


def test_collapse_steps():
    assert im.default_m_cap(6_000_000) == 1_924_096 and im.default_m_cap(1000) == 502
    assert im.collapse_steps([5] * 10, 0, 1000, 3) == [3, 3, 3, 3]      # rounds 0, 3, 6, 9 each start a call
    assert im.collapse_steps([5] * 10, 4, 20) == [4, 4]                       # capacity: 20 / 5 steps a call
    assert im.collapse_steps([3] * 65_535 + [2] * 4465, 0, 1_924_096) == [65_535, 962_048]
    assert im.collapse_steps([3] * 65_535, 0, 1_924_096) == [65_535]          # nothing left: no wide call
