"""(no GPU) The cases of tests/radix_seg_cases.py can catch the errors they are there for: a result that ignored the
segment column, the key, one of the segment digits, or the input order of equal tuples would differ from the reference.

Where a property can not hold it is not asked for, and only there:
* 0 or 1 item have one order.  Two items have two, which can not tell three sorts apart (if sorting by either half of
  the segment alone leaves them where they are, so does the full sort): a case of two is built against ONE of the errors,
  every bit pair gets a case for every error it can show, and each is held to its own error below.  (b), (c) and (e) as
  they stand start at 63 items, the next count there is;
* one segment value has no digit that could go wrong ((b) and (e): "more than one segment value");
* a constant key makes "by segment alone" THE order ((c): key kinds uniform and few)."""
import numpy as np
import pytest

from tests import radix_seg_cases as rs
from tests.radix_seg_cases import CASES, case_id

VISIBLE_FROM = 63


def _orders_differ(a, b):
    return not np.array_equal(a, b)


def test_the_listed_set_covers_what_it_has_to():
    assert len(CASES) == len(set(CASES))
    assert {c.count for c in CASES} == set(rs.COUNTS)
    assert {(c.key_lo_bit, c.seg_bits) for c in CASES} == set(rs.BIT_PAIRS)
    assert {c.seg_kind for c in CASES} == set(rs.SEG_KINDS) | {"zero"} | set(rs.PAIR_KINDS)
    assert {c.key_kind for c in CASES if c.key_lo_bit < 64} == set(rs.KEY_KINDS) | {"pair"}
    assert all((c.count == 2) == (c.seg_kind in rs.PAIR_KINDS) == (c.key_kind == "pair") for c in CASES)
    for pair in rs.BIT_PAIRS:  # every bit pair meets every tile-edge count, and every distribution it allows
        mine = [c for c in CASES if (c.key_lo_bit, c.seg_bits) == pair]
        assert set(rs.EDGE_COUNTS) | {rs.ODD_COUNT} <= {c.count for c in mine}, pair
        assert {c.seg_kind for c in mine} == set(rs.seg_kinds_for(*pair)) | set(rs.pair_kinds_for(*pair)), pair
        assert rs.pair_kinds_for(*pair), pair  # two items: a case for every error the pair can show
    # pass counts 1..8 and 12: every number of LDS histogram copies of k_radix_hist_all, min(16384 / (256 passes), 16)
    assert {rs.passes(c.key_lo_bit, c.seg_bits) for c in CASES} == {1, 2, 3, 4, 5, 6, 7, 8, 12}
    assert {min(64 // rs.passes(c.key_lo_bit, c.seg_bits), 16) for c in CASES} == {16, 12, 10, 9, 8, 5}
    assert all(rs.passes(c.key_lo_bit, c.seg_bits) <= 12 for c in CASES)  # RX_MAX_PASSES
    # first_pos: counts 1 and 2 (the count == 1 copy of kiss_radix_sort), single tile, several tiles, both dispatch sizes
    flagged = {c.count for c in CASES if c.flags}
    assert {0, 1, 2, rs.TILE, rs.TILE + 1, rs.BIG_COUNT} <= flagged
    # the shapes of the shipped callers: the stage partition (no key pass, 8 bits), the pivot round at k = 256
    assert {(64, 8), (40, 9)} <= {(c.key_lo_bit, c.seg_bits) for c in CASES if c.count == rs.BIG_COUNT}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_keeps_the_contract_and_can_catch_an_error(c):
    keys, seg, pos, order = rs.make_case(c)
    n, shift0 = c.count, rs.shift0_of(c)
    assert keys.dtype == np.uint64 and seg.dtype == np.uint32 and pos.dtype == np.uint32
    assert keys.size == seg.size == pos.size == order.size == n
    # the callers' contract: segment values below 2^seg_bits
    assert n == 0 or int(seg.max()) < (1 << c.seg_bits)
    assert np.unique(pos).size == n and not np.any(pos == 0xDEADBEEF)  # (the hook's poison value would be seen)
    bits = rs.sorted_key_bits(keys, shift0)
    if n <= 4096 or c.count == rs.ODD_COUNT:
        # (a) the reference is Python's sorted() on (seg, key >> shift0, index)
        want = sorted(range(n), key=lambda i: (int(seg[i]), int(bits[i]), i))
        assert order.tolist() == want
    else:  # the same statement without a Python loop: ascending tuples, ascending index inside equal ones
        s, b, o = seg[order].astype(np.int64), bits[order], order.astype(np.int64)
        up = (s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & ((b[1:] > b[:-1]) | ((b[1:] == b[:-1]) & (o[1:] > o[:-1]))))
        assert bool(np.all(up)) and np.array_equal(np.sort(order), np.arange(n))
    if shift0 > 0 and n >= VISIBLE_FROM:  # the payload below the sorted bits is there and is no order of its own
        low = keys & np.uint64((1 << shift0) - 1)
        assert np.unique(low).size > n // 2
    if n == 2:
        # the right order moves both items, and the one error the case is there for would leave them where they are
        assert order.tolist() == [1, 0]
        wrong = {"pair_seg": np.argsort(bits, kind="stable"), "pair_key": np.argsort(seg, kind="stable"),
                 "pair_low": np.lexsort((bits, seg >> np.uint32(8))), "pair_high": np.lexsort((bits, seg & np.uint32(255)))}
        assert wrong[c.seg_kind].tolist() == [0, 1]
        assert (c.seg_kind == "pair_key") == (seg[0] == seg[1]) and (shift0 == 64 or bits[0] != bits[1])
        if c.seg_kind == "pair_low":
            assert seg[0] >> 8 == seg[1] >> 8
        if c.seg_kind == "pair_high":
            assert seg[0] & 255 == seg[1] & 255
    if n < VISIBLE_FROM:
        return
    several = np.unique(seg).size > 1
    by_key = np.argsort(bits, kind="stable")
    by_seg = np.argsort(seg, kind="stable")
    if c.seg_bits > 0 and several:  # (b) a sort that ignored the segment column
        assert _orders_differ(by_key, order)
    if shift0 < 64 and c.key_kind != "constant":  # (c) a sort that ignored the key
        assert _orders_differ(by_seg, order)
    # (d) equal whole tuples: an unstable sort is visible in the payload and the positions
    tup = np.stack([seg[order].astype(np.uint64), bits[order]])
    same = np.all(tup[:, 1:] == tup[:, :-1], axis=0)
    assert bool(same.any())
    a, b = order[:-1][same], order[1:][same]
    assert bool(np.any((keys[a] != keys[b]) if shift0 > 0 else (pos[a] != pos[b])))
    if c.seg_bits > 8 and several:  # (e) a sort that dropped or misplaced one of the segment digits
        by_low = np.lexsort((bits, seg & np.uint32(255)))
        by_high = np.lexsort((bits, seg >> np.uint32(8)))
        assert _orders_differ(by_low, order)
        assert _orders_differ(by_high, order)
    if c.seg_kind in ("split_edge", "split_off") and n > rs.TILE:
        # the first run ends exactly at a tile edge / one item off it
        upper = seg >> np.uint32(8 if c.seg_bits > 8 else 0)
        run = int(np.count_nonzero(upper == upper[0]))
        assert np.all(upper[:run] == upper[0]) and np.all(upper[run:] != upper[0])
        assert (run % rs.TILE == 0) if c.seg_kind == "split_edge" else (run % rs.TILE in (1, rs.TILE - 1)), run
    if c.seg_kind == "digit_pairs":
        v = np.unique(seg)
        assert v.size == 4 and (v[0] ^ v[1]) < 256 and (v[0] ^ v[2]) >= 256 and (v[0] & 255) == (v[2] & 255)
    if c.seg_kind == "geometric" and c.seg_bits == 32:
        cnt = np.unique(seg, return_counts=True)[1]
        assert int(np.sort(cnt)[-4:].sum()) > n // 2 and int(np.count_nonzero(cnt == 1)) > n // 16
