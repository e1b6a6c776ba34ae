"""Small tied segments finished by one kernel (kiss_amd/csrc/lms_sort.hip: k_small_finish).

A refinement round of the LMS sort finishes every tied segment of up to 24 members on the spot.  k_small_finish does that
in one launch: a workgroup owns 256 items of the survivor stream plus a halo of 23 on either side, keeps the round's keys
in LDS and walks every key-tied pair once.  The result must be what the three-kernel form gives (k_gather_keys +
k_seg_adjacent + k_seg_finish: KISS_HIP_NO_SMALL_FUSED, hooks build), with the tied pairs in pair records or in the stream
(KISS_HIP_NO_FC0_ONEPASS), which is the oracle's.

The texts put small segments on every boundary the kernel has (wave, workgroup), at the threshold (24 members finish, 25
go to the big-segment path) and on both ranking paths (adjacent pairs in order; all pairs).  The test counts these on the
CPU from the far LMS suffixes -- the stream of the first refinement round, for the depth the sort ran at -- and asserts
that each text covers what it is meant to cover.  (tiny_triples has about 1 700 stream items and fewer than 8 tiles of
round-0 items, so its round 0 takes the count / scan / compact form; one_block_triples is the same with fewer than 256.)"""
import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

K_UNBOUNDED = 0xFFFFFFFF
MODES = [(32, 0), (256, 0), (K_UNBOUNDED, 0), (K_UNBOUNDED, 1)]  # (k, algo); algo 1 = PREFIX_DOUBLING
ROUND0_BASES = 20
STRETCH = 512    # items of one wave of k_fc0_onepass: a pair whose first member is a stretch's last item stays in the stream
ONEPASS_MIN = 8 * 8192
SMALL_SEG = 24
HOOKS = ("KISS_HIP_NO_SMALL_FUSED", "KISS_HIP_NO_FC0_ONEPASS")
# what each text must have in its first refinement round
COVERS = {
    "triples_exact": ("small", "cross64", "cross256"),
    "mixed_small": ("small", "cross64", "cross256", "exactly24", "more24", "unordered"),
    "short_arrays": ("small", "cross64", "cross256", "unordered"),
    "genome_like": ("small", "cross64", "cross256", "more24", "unordered"),
    "tiny_triples": ("small",),
    "one_block_triples": ("small",),
}


def _mutated(rng, block, rate):
    c = block.copy()
    if rate:
        hit = rng.random(c.size) < rate
        c[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    return c


def _copies(rng, block, c, rate):
    """c copies of a random block, each mutated at `rate`, each followed by 997 random bases"""
    b = rng.integers(0, 4, block, dtype=np.uint8)
    parts = []
    for _ in range(c):
        parts += [_mutated(rng, b, rate), rng.integers(0, 4, 997, dtype=np.uint8)]
    return np.concatenate(parts)


def _short_arrays(rng, count):
    """`count` tandem arrays of 12 x a random 171-base unit at 0.5 % mutations, each followed by 500 random bases"""
    parts = []
    for _ in range(count):
        unit = rng.integers(0, 4, 171, dtype=np.uint8)
        parts += [_mutated(rng, np.tile(unit, 12), 0.005), rng.integers(0, 4, 500, dtype=np.uint8)]
    return np.concatenate(parts)


def _texts():
    rng = np.random.default_rng(11)
    t = {}
    t["triples_exact"] = _copies(rng, 90_000, 3, 0)
    t["mixed_small"] = np.concatenate([_copies(rng, 20_000, 3, .01), _copies(rng, 12_000, 5, .02), _copies(rng, 4_000, 24, .01),
                                       _copies(rng, 4_000, 25, .01), _copies(rng, 8_000, 9, .10)])
    t["short_arrays"] = _short_arrays(rng, 200)
    t["genome_like"] = gen.genome_like(1_000_000, 31)
    t["tiny_triples"] = _copies(rng, 2_000, 3, 0)
    t["one_block_triples"] = _copies(rng, 250, 3, 0)
    return t


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


def _keys(S, p, start, bases):
    padded = np.concatenate([S, np.zeros(start + bases, np.uint8)]).astype(np.uint64)  # past the end reads as 'A'
    key = np.zeros(p.size, np.uint64)
    for t in range(start, start + bases):
        key = (key << np.uint64(2)) | padded[p + t]
    return key


def _first_round_stream(S, lms, depth):
    """The survivor stream of the first refinement round, computed on the CPU: the far LMS suffixes (p + depth <= n; all of
    them at depth 0) in the order of their first 20 bases then position, without the singletons and without the pairs that
    leave as pair records.  Counts over its tied segments."""
    far = lms[lms + depth <= S.size] if depth else lms
    k20 = _keys(S, far, 0, ROUND0_BASES)
    order = np.argsort(k20, kind="stable")
    k20, p = k20[order], far[order]
    m = p.size
    head = np.ones(m, bool)
    head[1:] = k20[1:] != k20[:-1]
    start = np.nonzero(head)[0]
    length = np.diff(np.append(start, m))
    stays = (length >= 3) | ((length == 2) & ((start % STRETCH == STRETCH - 1) | (m < ONEPASS_MIN)))
    keep = np.repeat(stays, length)
    p, length = p[keep], length[stays]
    sstart = np.cumsum(length) - length  # first member's index in the stream
    send = sstart + length - 1           # last member's
    small = (length >= 3) & (length <= SMALL_SEG)
    # the round's key: the next 32 bases (the depth is at least 125, so none is masked)
    k32 = _keys(S, p, ROUND0_BASES, 32)
    sid = np.repeat(np.arange(length.size), length)
    same = sid[1:] == sid[:-1]
    down = np.zeros(length.size, bool)   # some neighbour pair of the segment has its keys in descending order
    down[sid[1:][same & (k32[1:] < k32[:-1])]] = True
    srt = np.lexsort((k32, sid))
    tie = np.zeros(length.size, bool)    # two members share the key
    tie[sid[srt][1:][(sid[srt][1:] == sid[srt][:-1]) & (k32[srt][1:] == k32[srt][:-1])]] = True
    return {
        "items": int(p.size),
        "small": int(small.sum()),
        "cross64": int(np.sum(small & (sstart // 64 != send // 64))),
        "cross256": int(np.sum(small & (sstart // 256 != send // 256))),
        "exactly24": int(np.sum(length == SMALL_SEG)),
        "more24": int(np.sum(length > SMALL_SEG)),
        "unordered": int(np.sum(small & tie & down)),
    }


@pytest.mark.parametrize("k,algo", MODES)
@pytest.mark.parametrize("name", sorted(COVERS))
def test_small_finish_equals_the_three_kernel_form_and_the_oracle(name, k, algo, texts, refs, lms_lists, monkeypatch):
    import kiss_amd
    S = texts[name]
    want_sa, want_sorted = refs(name, k)
    for hook in HOOKS:
        monkeypatch.delenv(hook, raising=False)
    c = kiss_amd.Context(max_n=S.size, device=0, hooks=True)
    try:
        c.set_profiling(True)
        seen = {}
        for hooks in ((), HOOKS[:1], HOOKS[1:], HOOKS):
            for hook in hooks:
                monkeypatch.setenv(hook, "1")
            sa = c.suffix_sort(S, k, algo=algo)
            st = c.stats()
            for hook in hooks:
                monkeypatch.delenv(hook)
            what = " + ".join(hooks) or "default"
            assert np.array_equal(sa, want_sa), "suffix array, " + what
            if k != K_UNBOUNDED:
                assert np.array_equal(c.stage_outputs()[1], want_sorted), "sorted LMS list, " + what
            seen[hooks] = st
            # which path ran: with a pivot round ahead (bounded depth) the fused kernel needs no key in memory
            gathers = st["kernels"]["keygather"]["launches"]
            if k != K_UNBOUNDED and "KISS_HIP_NO_SMALL_FUSED" not in hooks:
                assert gathers == 0, what
            if "KISS_HIP_NO_SMALL_FUSED" in hooks:
                assert gathers > 0, what
        st = seen[()]
        rounds = (st["lms_rounds"], st["sort_item_rounds"])
        for hooks, other in seen.items():
            assert (other["lms_rounds"], other["sort_item_rounds"]) == rounds, hooks
        # the depth the LMS sort ran at: exact order by rank doubling (or after very deep ties) sorts to a bounded depth first
        depth = 125 * (st["refine_depth"] // 125 + 1) if st["refine_depth"] else st["depth"]
        got = _first_round_stream(S, lms_lists[name], int(depth))
        print("%s k=%d algo=%d depth=%d: %s" % (name, k, algo, depth, got))
        for what in COVERS[name]:
            assert got[what] > 0, (what, got)
        if name == "one_block_triples":
            assert got["items"] < 256, got
    finally:
        c.close()
