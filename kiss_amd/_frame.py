"""What the stages of the read-mapping pipeline (fm_chain, fm_align, fm_select, fm_pair, fm_rescue, fm_md, fm_insert, reads and
FMIndex) share on the Python side: parameters from keywords, records and read batches from what a caller hands in, addresses
for the library, the C interface's size-then-fill convention, and records back from device tensors.  Nothing here computes a
result; tests/test_py_entries_recording.py holds what the numpy entries hand to the library and give back.
"""
import numpy as np

from . import _lib

U32_MAX = 0xFFFFFFFF


def record_dtype(struct):
    """the numpy layout of a ctypes record struct whose fields are all u32"""
    return np.dtype([(k, np.uint32) for k, _ in struct._fields_])


def make_params(kind, defaults, given, limits=()):
    """defaults overridden by the keywords `given`, as a dict of ints: every key known, every value a u32 and at most its entry
    in limits.  The caller checks the rules of its own and builds its struct."""
    p = dict(defaults)
    for k, v in given.items():
        if k not in p:
            raise TypeError("unknown %s parameter %r (known: %s)" % (kind, k, ", ".join(sorted(p))))
        p[k] = int(v)
    if min(p.values()) < 0 or max(p.values()) > U32_MAX:
        raise ValueError("the %s parameters are u32" % kind)
    for k, top in dict(limits).items():
        if p[k] > top:
            raise ValueError("%s is at most %d" % (k, top))
    return p


def records(rows, dtype, what, columns=None, structured=None):
    """a structured array, or an (n, columns) integer array in the order of `columns` (default: every field of dtype) -> dtype
    array.  From a structured array the fields `structured` are taken (default: columns); what is not given is 0.  what: the
    message for integers that are no u32."""
    arr = np.asarray(rows)
    columns = columns or dtype.names
    if arr.dtype.names:
        out = np.zeros(arr.shape[0], dtype)
        for k in structured or columns:
            out[k] = arr[k]
        return out
    ints = np.asarray(arr, np.int64).reshape(-1, len(columns))
    if ints.size and (ints.min() < 0 or ints.max() > U32_MAX):
        raise ValueError(what)
    out = np.zeros(ints.shape[0], dtype)
    for j, k in enumerate(columns):
        out[k] = ints[:, j]
    return out


def read_batch(reads):
    """a list of uint8 arrays, or (concatenated, index) -> concatenated (u8), index (u64).  The caller checks the index: the
    stages differ in what they take"""
    if isinstance(reads, tuple):
        return np.ascontiguousarray(reads[0], dtype=np.uint8), np.ascontiguousarray(reads[1], dtype=np.uint64)
    arrs = [np.ascontiguousarray(r, dtype=np.uint8).ravel() for r in reads]
    index = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([a.size for a in arrs], out=index[1:])
    return (np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)), index


def read_list(reads):
    """the inverse: either form of a batch -> one uint8 array per read"""
    cat, index = read_batch(reads)
    return [cat[int(index[q]):int(index[q + 1])] for q in range(index.size - 1)]


def lengths_index(lengths):
    """Q read lengths -> the Q + 1 offsets (u64)"""
    lens = np.ascontiguousarray(lengths, dtype=np.uint64).ravel()
    index = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=index[1:])
    return index


def read_index(lengths_or_index):
    """the Q read lengths, or the tuple ("index", Q + 1 offsets) -> the offsets (u64)"""
    if isinstance(lengths_or_index, tuple):
        if lengths_or_index[0] != "index":
            raise ValueError('read_lengths_or_index is an array of lengths or ("index", offsets)')
        return np.ascontiguousarray(lengths_or_index[1], dtype=np.uint64).ravel()
    return lengths_index(lengths_or_index)


def addresses(*arrays):
    """-> the addresses of the arrays for the library (None stays None), and what has to live until its calls are over: the
    library takes no NULL for an array without entries, so such an array is handed over as one element of its dtype"""
    hold = [a if a is None or a.size else np.zeros(1, a.dtype) for a in arrays]
    return [None if a is None else a.ctypes.data for a in hold], hold


def sized(call, room, rep, *totals):
    """The C interface's size-then-fill convention.  room(*counts) -> the arguments of call for outputs of that many entries,
    without arguments: for none.  A call that has too little room returns KISS_HIP_E_INVALID and leaves the totals in the
    fields `totals` of the report; if the first of them is not 0 the outputs are made that large and the call is repeated.
    -> (status, the arguments of the last call)"""
    args = room()
    rc = call(*args)
    if rc == _lib.KISS_HIP_E_INVALID and getattr(rep, totals[0]):
        args = room(*[int(getattr(rep, k)) for k in totals])
        rc = call(*args)
    return rc, args


def record_view(tensor, n, dtype):
    """the first n rows of an (N, fields) int32 device tensor -> structured host array"""
    raw = np.ascontiguousarray(tensor[:n].cpu().numpy()).view(np.uint32).reshape(n, len(dtype.names))
    return raw.view(dtype).reshape(n)


def check_mates(Q):
    if Q % 2:
        raise ValueError("a batch of pairs has an even number of reads (2 p and 2 p + 1 are the mates of pair p), not %d" % Q)
