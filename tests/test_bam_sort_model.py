"""tests/bam_sort_model.py, the coordinate sort of BAM records defined in Python (include/kiss_hip_bam_sort.h), held
against what it can be held against without a GPU: numpy's stable argsort over the (rk, pos + 1) pairs on 500 random record sets,
the properties of a stable sort of whole records, the BAD rules one by one, and two cases worked by hand."""
import struct

import numpy as np

from tests import bam_model as B
from tests import bam_sort_model as M


def random_set(rng):
    """(records, n_ref): few references and few positions, so that keys tie; sizes from the least one up"""
    n_ref = int(rng.choice([1, 2, 3, 255, 256, 70000]))
    count = int(rng.choice([0, 1, 2, 3, 17, 64, 120]))
    recs = []
    for _ in range(count):
        ref = int(rng.choice([-1, 0, n_ref - 1, int(rng.integers(0, n_ref))]))
        pos = -1 if ref == -1 and rng.random() < 0.7 else int(rng.choice([-1, 0, 1, 255, 256, 65535, 65536, (1 << 31) - 1, int(rng.integers(0, 5))]))
        recs.append(M.make_record(ref, pos, rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes()))
    return recs, n_ref


def test_the_model_on_500_random_sets():
    rng = np.random.default_rng(2024)
    ties = 0
    for k in range(500):
        recs, n_ref = random_set(rng)
        bam, ri = M.pack(recs)
        got = M.sort(bam, ri, n_ref)
        n = len(recs)
        heads = [struct.unpack_from("<iii", r) for r in recs]
        rk = np.array([n_ref if h[1] == -1 else h[1] for h in heads], np.int64)
        p1 = np.array([h[2] + 1 for h in heads], np.int64)
        want = np.lexsort((p1, rk)) if n else np.zeros(0, np.int64)  # (lexsort is stable: the last key is the primary one)
        assert np.array_equal(want, np.argsort(rk * (1 << 32) + p1, kind="stable"))
        order = got["order"].astype(np.int64)
        assert np.array_equal(order, want), k
        # the properties
        assert sorted(order.tolist()) == list(range(n))
        keys = [(int(rk[r]), int(p1[r])) for r in order]
        assert keys == sorted(keys)
        for s in range(1, n):
            if keys[s] == keys[s - 1]:
                ties += 1
                assert order[s - 1] < order[s], k
        out = got["bam"].tobytes()
        idx = got["rec_index"]
        assert int(idx[0]) == 0 and int(idx[-1]) == len(out) == len(bam)
        for s in range(n):
            assert out[int(idx[s]):int(idx[s + 1])] == recs[order[s]], (k, s)
        assert sorted(B.split_records(out)) == sorted(recs)
        assert got["report"] == dict(records=n, bam_bytes=len(bam), unplaced=int(np.count_nonzero(rk == n_ref)),
                                     longest=max(map(len, recs), default=0), bad=0, first_bad=0)
        fast = M.sort_fast(bam, ri, n_ref)
        assert all(np.array_equal(fast[x], got[x]) for x in ("bam", "rec_index", "order")) and fast["report"] == got["report"], k
    assert ties > 1000  # (the stability is looked at, not assumed)


def test_two_records_with_the_unplaced_one_first():
    a, b = M.make_record(-1, -1, b"unplaced"), M.make_record(0, 0, b"placed")
    bam, ri = M.pack([a, b])
    got = M.sort(bam, ri, 1)
    assert got["order"].tolist() == [1, 0] and got["bam"].tobytes() == b + a
    assert got["rec_index"].tolist() == [0, len(b), len(a) + len(b)]
    assert got["report"] == dict(records=2, bam_bytes=len(a) + len(b), unplaced=1, longest=44, bad=0, first_bad=0)
    assert M.key_of(bam.tobytes(), 0, 1) == (1, 0) and M.key_of(bam.tobytes(), len(a), 1) == (0, 1)


def test_an_unmapped_mate_placed_at_its_partner_stays_beside_it():
    """read order: pair X (mate 1 on ref 1 at 500, mate 2 unmapped and placed there), a read on ref 0, pair Y the other way round
    (the unmapped mate first) on ref 1 at 500 as well, an unplaced pair, a read on ref 1 at 499"""
    recs = [M.make_record(1, 500, b"X/1 mapped"), M.make_record(1, 500, b"X/2 unmapped, placed"), M.make_record(0, 9, b"Z"),
            M.make_record(1, 500, b"Y/1 unmapped, placed"), M.make_record(1, 500, b"Y/2 mapped"), M.make_record(-1, -1, b"U/1"),
            M.make_record(-1, -1, b"U/2"), M.make_record(1, 499, b"W")]
    bam, ri = M.pack(recs)
    got = M.sort(bam, ri, 2)
    assert got["order"].tolist() == [2, 7, 0, 1, 3, 4, 5, 6]
    assert got["report"]["unplaced"] == 2 and B.split_records(got["bam"].tobytes()) == [recs[r] for r in got["order"]]


def test_every_bad_kind():
    good = [M.make_record(0, 5, b"a"), M.make_record(1, 6, b"bc"), M.make_record(-1, -1), M.make_record(1, 0, b"d" * 20)]
    bam, ri = M.pack(good)
    assert M.bad_records(bam, ri, 2) == [] and "bam" in M.sort(bam, ri, 2)

    def bad_of(bam, ri, n_ref=2):
        rep = M.sort(bam, ri, n_ref)
        assert set(rep) == {"report"}
        return M.bad_records(bam, ri, n_ref), rep["report"]["bad"], rep["report"]["first_bad"]

    shifted = ri.copy()
    shifted[0] = 1
    assert bad_of(bam, shifted) == ([0], 1, 0)                       # rec_index[0] != 0 (and block_size no longer fits: one record)
    longer = np.concatenate((bam, np.zeros(3, np.uint8)))
    assert bad_of(longer, ri) == ([3], 1, 3)                         # rec_index[records] != bam_bytes
    assert bad_of(bam[:-1], ri) == ([3], 1, 3)                       # ... on the other side: the record reaches past the bytes
    flat = ri.copy()
    flat[2] = flat[1]
    assert bad_of(bam, flat)[0] == [1, 2]                            # an empty record, and its neighbour's block_size is off
    for r in range(4):
        for rec, n_ref in ((M.make_record(0, 0)[:35], 2), (M.make_record(0, 0, block_size=33), 2), (M.make_record(-2, 0), 2),
                           (M.make_record(2, 0), 2), (M.make_record(0, 0), 0), (M.make_record(0, -2), 2), (M.make_record(0, 0, block_size=-1), 2)):
            recs = list(good)
            recs[r] = rec
            b, i = M.pack(recs)
            if len(rec) == 35:
                b[int(i[r])] = 31                                    # (its block_size is right: only the size is wrong)
            assert bad_of(b, i, n_ref)[1:] == ((1, r) if n_ref else (4 if r == 2 else 3, 0)), (r, rec[:12])
    assert M.bad_records(*M.pack([M.make_record(0, (1 << 31) - 1), M.make_record(-1, 7)]), 1) == []  # a place is not asked of refID -1
