"""Cases and host reference for the segment-carrying radix sort (kiss_radix_sort with seg_bits > 0, radix.hip), shared by
tests/test_radix_seg_gpu.py (the device runs) and tests/test_radix_seg_cases.py (CPU: can the cases catch an error?).

A case is (count, key_lo_bit, seg_bits, segment distribution, key distribution, flags).  The sort orders tuples
(key64, seg32, pos32) by seg first and then by key >> shift0, shift0 = key_lo_bit & ~7; equal tuples keep their input order.
The key bits below shift0 are random payload: they travel with their item and never influence the order.

Contract of the callers (bits_for(number of segments), lms_sort.hip / flag_compact.hip; group ids < 256 at 8 bits,
stages.hip): every segment value is below 2^seg_bits.  The generator keeps to it; with seg_bits == 0 the column is all 0.
"""
import collections
import functools

import numpy as np

TILE = 16384
SMALL_COUNTS = [0, 1, 2, 63, 64, 65]
EDGE_COUNTS = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1]  # every bit pair meets every one of these
ODD_COUNT = 3 * TILE + 4097
BIG_COUNT = 64 * TILE + 1  # two RX_CHUNK column-sum chunks on the tile-histogram path
COUNTS = SMALL_COUNTS + EDGE_COUNTS + [ODD_COUNT, BIG_COUNT]

# (key_lo_bit, seg_bits) -> passes: 1 1 2 2 3 4 | 2 4 5 6 7 5 12 8.  (32, 15) is here for the six passes that no pair of the
# callers' shapes gives: with it every number of LDS histogram copies of k_radix_hist_all occurs (16, 12, 10, 9, 8, 5).
BIT_PAIRS = [(64, 1), (64, 8), (64, 9), (64, 16), (64, 17), (64, 32), (56, 3), (46, 7), (40, 9), (32, 15), (24, 12), (24, 0),
             (0, 32), (0, 0)]
SEG_KINDS = ["equal", "split_edge", "split_off", "uniform", "geometric", "sorted", "reversed", "digit_pairs"]
KEY_KINDS = ["uniform", "constant", "few"]
# Two items have one order that is right and one that is wrong, so a case of two is built against ONE error each, the
# wrong order always being "nothing moved" (the reference is [1, 0]):
#   pair_seg   segments descending, keys ascending: a sort that ignored the segment column leaves them
#   pair_key   one segment, keys descending: a sort that ignored the key leaves them
#   pair_low   segments descending that differ in the lowest digit only: dropping that digit leaves them
#   pair_high  segments descending that differ above the lowest digit only: dropping those digits leaves them
PAIR_KINDS = ["pair_seg", "pair_key", "pair_low", "pair_high"]

Case = collections.namedtuple("Case", "count key_lo_bit seg_bits seg_kind key_kind flags")


def passes(key_lo_bit, seg_bits):
    return (64 - (key_lo_bit & ~7)) // 8 + (seg_bits + 7) // 8


def seg_kinds_for(key_lo_bit, seg_bits):
    """the segment distributions that make sense for a bit pair"""
    if seg_bits == 0:
        return ["zero"]  # the contract leaves nothing else
    kinds = ["equal", "split_edge", "split_off", "uniform", "geometric", "reversed"]
    if key_lo_bit < 64:
        kinds.append("sorted")  # (without key passes a sorted column is sorted input: nothing would move)
    if seg_bits > 8:
        kinds.append("digit_pairs")
    return kinds


def pair_kinds_for(key_lo_bit, seg_bits):
    kinds = ["pair_seg"] if seg_bits > 0 else []
    if key_lo_bit < 64:
        kinds.append("pair_key")
    if seg_bits > 8:
        kinds += ["pair_low", "pair_high"]
    return kinds


def _case(count, pair, i, flags=0):
    """the i-th choice of distributions for a bit pair: walks through the pair's segment kinds and the key kinds"""
    lo, sb = pair
    kinds = seg_kinds_for(lo, sb)
    p = BIT_PAIRS.index(pair)
    seg_kind = kinds[(i + p) % len(kinds)]
    key_kind = KEY_KINDS[(i + 2 * p) % 3]
    if seg_kind == "sorted" and key_kind == "constant":
        key_kind = "few"  # (sorted segments and one key: sorted input again)
    if seg_kind in ("equal", "zero") and key_kind == "constant" and lo < 64:
        key_kind = "few" if i % 2 == 0 else "uniform"  # (one segment and one key: nothing but stability would show)
    return Case(count, lo, sb, seg_kind, key_kind, flags)


def _build_cases():
    cases = []
    for p, pair in enumerate(BIT_PAIRS):
        # every tile-edge count and the odd three-tile count, and with them every distribution the pair allows
        for i, n in enumerate(EDGE_COUNTS + [ODD_COUNT] + EDGE_COUNTS[:3]):
            cases.append(_case(n, pair, i))
        # the small counts: two per pair, so that every small count meets at least four pairs
        for j in range(2):
            if SMALL_COUNTS[(2 * p + j) % 6] != 2:
                cases.append(_case(SMALL_COUNTS[(2 * p + j) % 6], pair, 3 + j))
        # two items: every bit pair, one case for every error the pair can show
        for kind in pair_kinds_for(*pair):
            cases.append(Case(2, pair[0], pair[1], kind, "pair", 0))
    for i, pair in enumerate([(64, 8), (40, 9), (0, 32), (24, 0), (64, 17)]):
        cases.append(_case(BIG_COUNT, pair, [3, 4, 3, 0, 7][i]))
    # first_pos (flags bit 0): counts 1 and 2, and some of every size class, with and without key passes
    for pair in [(64, 8), (40, 9), (24, 0), (0, 32)]:
        for i, n in enumerate([1, 65, TILE, TILE + 1, 2 * TILE + 1, ODD_COUNT]):
            cases.append(_case(n, pair, i + 3, flags=1))
        for kind in pair_kinds_for(*pair):
            cases.append(Case(2, pair[0], pair[1], kind, "pair", 1))
    cases.append(_case(0, (64, 9), 3, flags=1))
    cases.append(_case(BIG_COUNT, (24, 12), 3, flags=1))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CASES = _build_cases()


def case_id(c):
    return "%d-lo%d-sb%d-%s-%s-f%d" % c


def shift0_of(c):
    return c.key_lo_bit & ~7


def sorted_key_bits(keys, shift0):
    """key >> shift0 (numpy leaves a shift by 64 undefined: there are no sorted key bits then)"""
    return np.zeros(keys.size, dtype=np.uint64) if shift0 >= 64 else keys >> np.uint64(shift0)


def _segments(c, rng):
    n, sb = c.count, c.seg_bits
    if c.seg_kind == "zero" or n == 0:
        return np.zeros(n, dtype=np.uint32)
    top = (1 << sb) - 1  # the largest value the contract allows
    if c.seg_kind == "equal":
        return np.full(n, top - (top >> 2), dtype=np.uint32)
    if c.seg_kind in ("split_edge", "split_off"):
        # the larger value first, so that the whole first run moves behind the second one.  The run ends exactly at a
        # tile edge (in the middle of a count too small to have one), or one item off it
        cut = TILE * max(1, (n // TILE) // 2) if n > TILE else n // 2
        if c.seg_kind == "split_off":
            cut += 1 if (n // TILE) % 2 == 0 and cut + 1 < n else -1
        cut = max(cut, 0)
        i = np.arange(n)
        if sb <= 8:
            return np.where(i < cut, top, top >> 1).astype(np.uint32)
        # more than one segment digit: the upper digits split at that edge and the lowest digit in the middle of the
        # first run, so that there is a pair of segments that differs in the lower digit only and one that differs in
        # the upper digits only (two values could not show an error in either digit alone)
        hi = np.where(i < cut, top >> 8, (top >> 8) >> 1)
        lo = np.where(i < cut // 2, 0xC4, 0x21)
        return ((hi << 8) | lo).astype(np.uint32)
    if c.seg_kind == "geometric":
        # a few huge segments and many singletons
        huge = (np.array([1, 3, 5, 7], dtype=np.uint64) * np.uint64(top) // np.uint64(8)).astype(np.uint32)
        if sb > 8:
            huge[1] = huge[0] ^ np.uint32(0x5A)  # two of them differ in the lowest digit only (the others: above it)
        s = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
        which = np.minimum(rng.geometric(0.35, n) - 1, 5)  # 82 % in the four huge ones, 18 % on their own
        return np.where(which < 4, huge[np.minimum(which, 3)], s).astype(np.uint32)
    if c.seg_kind == "digit_pairs":
        # two values in the lowest digit times two values in the digits above it
        hi = np.array([(top >> 8) >> 1, top >> 8], dtype=np.uint32)[rng.integers(0, 2, n)]
        lo = np.array([0x21, 0xC4], dtype=np.uint32)[rng.integers(0, 2, n)]
        return ((hi << np.uint32(8)) | lo).astype(np.uint32)
    # uniform over the full range, about eight members per segment so that the keys matter inside a segment
    if sb <= 8:
        pool = rng.integers(0, top + 1, max(1, n // 8), dtype=np.uint64).astype(np.uint32)
    else:  # ... and four segments to every value of the upper digits, so that each digit decides between some of them
        upper = rng.integers(0, (top >> 8) + 1, max(2, n // 32), dtype=np.uint64)
        upper[0], upper[-1] = 0, top >> 8  # (a small pool still has two values)
        lower = rng.choice(256, 4, replace=False).astype(np.uint64)
        pool = ((upper[:, None] << np.uint64(8)) | lower[None, :]).reshape(-1).astype(np.uint32)
    s = pool[rng.integers(0, pool.size, n)]
    if c.seg_kind == "sorted":
        return np.sort(s)
    if c.seg_kind == "reversed":
        return np.sort(s)[::-1].copy()
    assert c.seg_kind == "uniform", c.seg_kind
    return s


def _pair(c):
    """the two items of a PAIR_KINDS case: (seg, sorted key bits)"""
    top, width = (1 << c.seg_bits) - 1, 64 - shift0_of(c)
    small, big = 0x2121212121212121 & ((1 << width) - 1), 0xC4C4C4C4C4C4C4C4 & ((1 << width) - 1)
    bits = [big, small] if c.seg_kind == "pair_key" else [small, big]  # (no sorted key bits: both 0)
    if c.seg_kind == "pair_key":
        seg = [top - (top >> 2)] * 2
    elif c.seg_kind == "pair_seg":
        seg = [top, top >> 1]  # (more than one digit: they differ in the top bit only, the lowest digit is 0xFF in both)
    elif c.seg_kind == "pair_low":
        seg = [((top >> 8) << 8) | 0xC4, ((top >> 8) << 8) | 0x21]
    else:
        assert c.seg_kind == "pair_high", c.seg_kind
        seg = [((top >> 8) << 8) | 0x5A, (((top >> 8) >> 1) << 8) | 0x5A]
    return np.array(seg, dtype=np.uint32), np.array(bits, dtype=np.uint64)


def _sorted_bits(c, rng):
    """the key bits [shift0, 64) as a number below 2^(64 - shift0)"""
    n, width = c.count, 64 - shift0_of(c)
    if width == 0:
        return np.zeros(n, dtype=np.uint64)
    if c.key_kind == "uniform":
        v = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
        return v >> np.uint64(64 - width)
    mask = np.uint64((1 << width) - 1)
    if c.key_kind == "constant":
        return np.full(n, np.uint64(0x5A17C3E9A1B2D4F6) & mask, dtype=np.uint64)
    assert c.key_kind == "few", c.key_kind
    # three values that differ in every digit: many exact duplicates of the whole (seg, key >> shift0) tuple
    vals = np.array([0xC4C4C4C4C4C4C4C4, 0x2121212121212121, 0x7E7E7E7E7E7E7E7E], dtype=np.uint64) & mask
    return vals[rng.integers(0, 3, n)]


@functools.lru_cache(maxsize=4)
def make_case(c):
    """-> (keys u64, seg u32, pos u32, order): the input columns and the permutation a stable sort applies (read-only)"""
    rng = np.random.default_rng([c.count, c.key_lo_bit, c.seg_bits, (["zero"] + SEG_KINDS + PAIR_KINDS).index(c.seg_kind),
                                 (KEY_KINDS + ["pair"]).index(c.key_kind)])
    n, shift0 = c.count, shift0_of(c)
    if c.seg_kind in PAIR_KINDS:
        assert n == 2 and c.key_kind == "pair"
        seg, bits = _pair(c)
    else:
        seg = _segments(c, rng)
        bits = _sorted_bits(c, rng)
    # equal whole tuples next to each other, across the first tile edge, and (where the distribution has no order of its
    # own to keep) far apart: what shows an unstable sort
    pairs = [(n // 3, n // 3 + 1), (TILE - 1, TILE)]
    if c.seg_kind in ("uniform", "geometric", "digit_pairs", "zero"):
        pairs.append((0, n - 1))
    for a, b in pairs:
        if n >= 4 and 0 <= a < b < n and not (c.seg_kind.startswith("split") and seg[a] != seg[b]):  # (the split stays where it is)
            seg[b], bits[b] = seg[a], bits[a]
    low = rng.integers(0, 1 << 63, n, dtype=np.uint64)  # payload below the sorted bits
    if shift0 == 0:
        keys = bits
    elif shift0 == 64:
        keys = low << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    else:
        keys = (bits << np.uint64(shift0)) | (low >> np.uint64(64 - shift0))
    pos = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)).astype(np.uint32)  # no two equal
    order = reference_order(keys, seg, shift0)
    for a in (keys, seg, pos, order):
        a.setflags(write=False)
    return keys, seg, pos, order


def reference_order(keys, seg, shift0):
    """stable: segment primary, then the key bits from shift0 up (np.lexsort sorts by its LAST key first)"""
    return np.lexsort((sorted_key_bits(keys, shift0), seg))
