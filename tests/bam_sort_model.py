"""kiss_hip_bam_sort_* (include/kiss_hip_bam_sort.h) restated as plain loops: which records are BAD, the key of
a record, the stable order, the sorted bytes with their CSR and the counts of the report.  Nothing here is fast and nothing is
shared with the library; tests/test_bam_sort_model.py holds it against numpy's stable argsort and against cases worked by hand."""
import struct

import numpy as np

RECORD_MIN = 36


def make_record(ref, pos, body=b"", block_size=None):
    """a record that is valid in the sort's sense: block_size, refID, pos, then 24 + len(body) bytes the sort never looks at
    (block_size: what the field says, when it is to be wrong)"""
    rest = bytes((7 * i + 1) & 255 for i in range(24)) + bytes(body)
    size = 12 + len(rest)
    return struct.pack("<iii", size - 4 if block_size is None else block_size, ref, pos) + rest


def pack(records):
    """records (a list of bytes) -> (bam as uint8, rec_index as uint64)"""
    index = np.zeros(len(records) + 1, np.uint64)
    at = 0
    for r, rec in enumerate(records):
        at += len(rec)
        index[r + 1] = at
    return np.frombuffer(b"".join(records), np.uint8).copy(), index


def bad_records(bam, rec_index, n_ref):
    """the BAD records, ascending"""
    bam = bytes(bytearray(bam))
    ri = [int(x) for x in rec_index]
    records = len(ri) - 1
    bad = []
    for r in range(records):
        a, b = ri[r], ri[r + 1]
        wrong = (r == 0 and a != 0) or (r == records - 1 and b != len(bam)) or b <= a or b > len(bam) or b - a < RECORD_MIN
        if not wrong:
            block_size, ref, pos = struct.unpack_from("<iii", bam, a)
            wrong = block_size != b - a - 4 or ref < -1 or ref >= n_ref or pos < -1
        if wrong:
            bad.append(r)
    return bad


def key_of(bam, at, n_ref):
    """(rk, pos + 1) of the record at byte `at`"""
    _, ref, pos = struct.unpack_from("<iii", bam, at)
    return (n_ref if ref == -1 else ref, pos + 1)


def sort(bam, rec_index, n_ref):
    """-> dict(bam, rec_index, order, report) as the library gives them; with BAD input: dict(report) alone, bad and first_bad in it"""
    raw = bytes(bytearray(bam))
    ri = [int(x) for x in rec_index]
    records = len(ri) - 1
    report = dict(records=records, bam_bytes=len(raw), unplaced=0, longest=0, bad=0, first_bad=0)
    bad = bad_records(raw, ri, n_ref)
    if bad:
        report.update(bad=len(bad), first_bad=bad[0])
        return {"report": report}
    keys = [key_of(raw, ri[r], n_ref) for r in range(records)]
    # insertion into a list, from the left: record r goes behind every record whose key is not larger (stable)
    order = []
    for r in range(records):
        at = len(order)
        while at > 0 and keys[order[at - 1]] > keys[r]:
            at -= 1
        order.insert(at, r)
    out, index = [], [0]
    for r in order:
        out.append(raw[ri[r]:ri[r + 1]])
        index.append(index[-1] + ri[r + 1] - ri[r])
    report["unplaced"] = sum(1 for k in keys if k[0] == n_ref)
    report["longest"] = max((ri[r + 1] - ri[r] for r in range(records)), default=0)
    return {"bam": np.frombuffer(b"".join(out), np.uint8).copy(), "rec_index": np.array(index, np.uint64),
            "order": np.array(order, np.uint32), "report": report}


def sort_fast(bam, rec_index, n_ref):
    """the same result through numpy's stable sort, for the inputs of the GPU tests that are too long for the loops above (the
    two are held against each other in tests/test_bam_sort_model.py); BAD input is not looked for"""
    raw = np.ascontiguousarray(bam, dtype=np.uint8).ravel()
    ri = np.asarray(rec_index, np.uint64).astype(np.int64)
    records = ri.size - 1
    head = np.zeros((records, 12), np.uint8)
    for b in range(12):
        head[:, b] = raw[ri[:-1] + b]
    f = head.view("<i4")
    ref, pos = f[:, 1].astype(np.int64), f[:, 2].astype(np.int64)
    rk = np.where(ref == -1, n_ref, ref)
    key = rk * (1 << 32) + (pos + 1)
    order = np.argsort(key, kind="stable")
    size = np.diff(ri)
    index = np.zeros(records + 1, np.int64)
    np.cumsum(size[order], out=index[1:])
    out = np.zeros(raw.size, np.uint8)
    src = np.repeat(ri[:-1][order] - index[:-1], size[order]) + np.arange(raw.size, dtype=np.int64) if records else np.zeros(0, np.int64)
    out[:] = raw[src]
    report = dict(records=records, bam_bytes=int(raw.size), unplaced=int(np.count_nonzero(ref == -1)), longest=int(size.max()) if records else 0,
                  bad=0, first_bad=0)
    return {"bam": out, "rec_index": index.astype(np.uint64), "order": order.astype(np.uint32), "report": report}
