"""Tied pairs decided from pair records (kiss_amd/csrc/flag_compact.hip: k_fc0_onepass<true>, lms_sort.hip: k_pair_finish).

Round 0's one-pass flag + compact takes the tied segments of exactly two items out of the survivor stream and writes one
record per pair; one lane per record decides it.  The result must be what the survivor stream's pair path gives
(KISS_HIP_NO_PAIR_RECORDS, hooks build) and what the count / scan / compact form gives (KISS_HIP_NO_FC0_ONEPASS), which is
the oracle's.

The texts are the smallest that reach the one-pass form (at least 8 tiles of 8192 far LMS suffixes) and put pairs on
every boundary of k_fc0_onepass: lane, 128-item chunk, 512-item wave stretch, 8192-item tile.  A pair whose first member
is the last item of a wave's stretch stays in the survivor stream, so the number of records is the number of pairs minus
those: the test counts both on the CPU from the 20-base keys of the far LMS suffixes, for the depth the sort ran at, and
asserts equality; and it asserts the bound computed for k = 256 when the change was specified (PAIRS_K256)."""
import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

K_UNBOUNDED = 0xFFFFFFFF
MODES = [(32, 0), (256, 0), (K_UNBOUNDED, 0), (K_UNBOUNDED, 1)]  # (k, algo); algo 1 = PREFIX_DOUBLING
ROUND0_BASES = 20
STRETCH = 512  # items of one wave of k_fc0_onepass
# pairs among the far LMS suffixes at k = 256 (depth 375), counted on the CPU
PAIRS_K256 = {"genome_like": 24_614, "copies_exact": 116_664, "copies_diverged": 100_189}


def _texts():
    rng = np.random.default_rng(7)
    b = rng.integers(0, 4, 400_000, dtype=np.uint8)
    gap = rng.integers(0, 4, 5_000, dtype=np.uint8)
    c = b.copy()
    hit = rng.random(c.size) < 0.01
    c[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    return {
        "genome_like": gen.genome_like(1_000_000, 31),       # pairs, segments of 3-24 and big segments: the mixed stream
        "copies_exact": np.concatenate([b, gap, b]),         # 99 % of the list is pair members, nearly every walk ends tied
        "copies_diverged": np.concatenate([b, gap, c]),      # walks end on a difference, about half of the pairs swap
    }


@pytest.fixture(scope="module")
def texts():
    return _texts()


@pytest.fixture(scope="module")
def refs(texts, oracle):
    """(text name, k) -> (suffix array, sorted LMS list without the sentinel) of the oracle, computed once."""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            sa, lms_sorted = oracle.suffix_sort(texts[name], k, stages=True)
            cache[(name, k)] = (sa, lms_sorted[1:])
        return cache[(name, k)]
    return get


@pytest.fixture(scope="module")
def lms_lists(texts, oracle):
    return {name: oracle.get_lms(S)[0][:-1].astype(np.int64) for name, S in texts.items()}


def _pairs_and_stretch_straddlers(S, lms, depth):
    """Tied segments of exactly two among the far LMS suffixes (p + depth <= n; all of them at depth 0) sorted on their first
    20 bases, and how many of those have their first member in the last slot of a 512-item stretch of the sorted list."""
    far = lms[lms + depth <= S.size] if depth else lms
    padded = np.concatenate([S, np.zeros(ROUND0_BASES, np.uint8)]).astype(np.uint64)  # past the end reads as 'A'
    key = np.zeros(far.size, np.uint64)
    for t in range(ROUND0_BASES):
        key = (key << np.uint64(2)) | padded[far + t]
    key.sort()
    m = key.size
    head = np.ones(m + 2, bool)  # items past the end count as heads
    head[1:m] = key[1:] != key[:-1]
    first = np.nonzero(head[:m] & ~head[1:m + 1] & head[2:m + 2])[0]
    return m, first.size, int(np.sum(first % STRETCH == STRETCH - 1))


@pytest.mark.parametrize("k,algo", MODES)
@pytest.mark.parametrize("name", sorted(PAIRS_K256))
def test_pair_records_equal_the_survivor_stream_and_the_oracle(name, k, algo, texts, refs, lms_lists, monkeypatch):
    import kiss_amd
    S = texts[name]
    want_sa, want_sorted = refs(name, k)
    for hook in ("KISS_HIP_NO_PAIR_RECORDS", "KISS_HIP_NO_FC0_ONEPASS"):
        monkeypatch.delenv(hook, raising=False)
    # sized to the text: on the copies the tied items exceed the default tied-segment reservation
    c = kiss_amd.Context(max_n=S.size, device=0, hooks=True)
    try:
        sa = c.suffix_sort(S, k, algo=algo)
        st = c.stats()
        assert np.array_equal(sa, want_sa), "suffix array, pair records"
        if k != K_UNBOUNDED:
            assert np.array_equal(c.stage_outputs()[1], want_sorted), "sorted LMS list, pair records"
        # the depth the LMS sort ran at: exact order by rank doubling (or after very deep ties) sorts to a bounded depth first
        depth = 125 * (st["refine_depth"] // 125 + 1) if st["refine_depth"] else st["depth"]
        m_far, pairs, straddlers = _pairs_and_stretch_straddlers(S, lms_lists[name], int(depth))
        print("%s k=%d algo=%d depth=%d: far %d, pairs %d, of which %d stay in the stream; pair_records %d"
              % (name, k, algo, depth, m_far, pairs, straddlers, st["pair_records"]))
        assert m_far >= 8 * 8192, "the one-pass form needs 8 tiles"
        assert straddlers > 0, "no pair on a stretch boundary"
        assert 0 < st["pair_records"] <= PAIRS_K256[name]
        assert st["pair_records"] == pairs - straddlers
        rounds = (st["lms_rounds"], st["sort_item_rounds"])
        for hook in ("KISS_HIP_NO_PAIR_RECORDS", "KISS_HIP_NO_FC0_ONEPASS"):
            monkeypatch.setenv(hook, "1")
            sa = c.suffix_sort(S, k, algo=algo)
            st = c.stats()
            monkeypatch.delenv(hook)
            assert st["pair_records"] == 0, hook
            assert np.array_equal(sa, want_sa), "suffix array, " + hook
            # the pairs count as items of the first refinement round either way
            assert (st["lms_rounds"], st["sort_item_rounds"]) == rounds, hook
    finally:
        c.close()
