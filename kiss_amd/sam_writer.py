"""The alignment lines of the SAM output, written on the device (kiss_hip_fmi_sam_dev / _host; include/kiss_hip_sam.h has the
definition; kiss_amd.fm_sam.sam_header gives the lines in front of them).  sam_lines() takes numpy arrays -- records from
anywhere -- and runs the host entry; FMIndex.map(sam=True) and map_pairs(sam=True) keep everything on the device and run the
device entry (sam_lines_dev).  All arithmetic runs in libkiss_hip.so; there is no CPU path."""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, records, sized
from .fm_sam import _bytes
from .sorter import _check


def pack_names(names):
    """a list of str or bytes -> (the bytes one after the other, u8; where each starts, u64; its length, u32): the spans the
    library takes.  A (raw, name_off, name_len) triple, as parse_reads gives it, is handed through"""
    if isinstance(names, tuple) and len(names) == 3:
        return (np.ascontiguousarray(names[0], dtype=np.uint8).ravel(), np.ascontiguousarray(names[1], dtype=np.uint64).ravel(),
                np.ascontiguousarray(names[2], dtype=np.uint32).ravel())
    parts = [_bytes(x) for x in names]
    lens = np.array([len(x) for x in parts], np.uint32)
    off = np.zeros(len(parts), np.uint64)
    if len(parts) > 1:
        np.cumsum(lens[:-1], out=off[1:])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), off, lens


def name_index(names):
    """the R names of the records -> (their bytes, the R + 1 offsets)"""
    parts = [_bytes(x) for x in (names or [])]
    idx = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(x) for x in parts], out=idx[1:])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), idx


def sam_input(ptrs, Q, C, R, first_alns):
    """kiss_hip_sam_input from a dict of addresses (what is missing or None is NULL) and the counts"""
    unknown = set(ptrs) - set(_lib.SamInput.POINTERS)
    if unknown:
        raise TypeError("unknown array(s) of the SAM input: %s (known: %s)" % (", ".join(sorted(unknown)), ", ".join(_lib.SamInput.POINTERS)))
    s = _lib.SamInput()
    for k in _lib.SamInput.POINTERS:
        setattr(s, k, ptrs.get(k))
    s.Q, s.C, s.R, s.first_alns = int(Q), int(C), int(R), int(first_alns)
    return s


def sam_lines_dev(lib, ctx, device, Q, C, R=0, first_alns=0, want_line_index=True, stream=None, **tensors):
    """the device entry on torch tensors -> dict of torch tensors (d_sam, d_line_index, d_read_line) and the report; two calls, the
    first one sizes the bytes and the lines (the C interface's convention).  tensors: the arrays of kiss_hip_sam_input by their
    names (None: NULL).  stream: None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.SamReport()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    inp = sam_input({k: (None if t is None else t.data_ptr()) for k, t in tensors.items()}, Q, C, R, first_alns)
    d_rl = torch.zeros(Q + 1, dtype=torch.int64, device=dev)

    def call(d_sam, cap, d_li, lcap):
        return lib.kiss_hip_fmi_sam_dev(ctx._ctx, ctypes.byref(inp), vp(d_sam.data_ptr()), cap, vp(d_li.data_ptr()) if d_li is not None else None,
                                        lcap, vp(d_rl.data_ptr()), ctypes.byref(rep), vp(stream) if stream else None)

    def room(m=0, lines=0):
        return (torch.zeros(max(m, 1), dtype=torch.uint8, device=dev), m,
                torch.zeros(lines + 1, dtype=torch.int64, device=dev) if want_line_index else None, lines)

    rc, (d_sam, _, d_li, _) = sized(call, room, rep, "sam_bytes", "lines")
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        raise _lib.KissHipError(rc, "kiss_hip_fmi_sam_dev", "%d bad read(s), the first one read %d" % (rep.bad, rep.first_bad))
    _check(rc, "kiss_hip_fmi_sam_dev", ctx._ctx)
    return {"d_sam": d_sam, "d_line_index": d_li, "d_read_line": d_rl, "rep": rep, "keep": tensors}


def sam_arrays(out):
    """the tensors of sam_lines_dev as what map(sam=True) adds to its result"""
    total = int(out["rep"].sam_bytes)
    li = out["d_line_index"]
    return {"sam": out["d_sam"][:total].cpu().numpy().tobytes(), "sam_line_index": None if li is None else li.cpu().numpy().view(np.uint64),
            "sam_read_line": out["d_read_line"].cpu().numpy().view(np.uint64), "sam_report": out["rep"].as_dict()}


def default_names(Q, paired=False):
    """the names of reads that have none, as the command line prints them: the decimal read number, or the pair number for both
    mates"""
    return [str(q // 2 if paired else q).encode() for q in range(Q)]


def _host_input(reads, read_index, names, alns, cigar, cigar_index, hits, hit_index, qual=None, pairs=None, source=None, first_alns=0, md=None,
                md_index=None, ref_names=None, bounds=None):
    """the arrays of a batch, as sam_lines takes them, held against each other -> (kiss_hip_sam_input over host pointers, Q, what
    keeps the arrays alive)"""
    from .fm_align import ALN_DTYPE
    from .fm_pair import PAIR_DTYPE
    from .fm_select import HIT_DTYPE
    cat = np.ascontiguousarray(reads, dtype=np.uint8).ravel()
    ridx = np.ascontiguousarray(read_index, dtype=np.uint64).ravel()
    if ridx.size < 1:
        raise ValueError("the read index has Q + 1 entries")
    Q = ridx.size - 1
    ql = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8).ravel()
    raw, noff, nlen = pack_names(names)
    al = records(alns, ALN_DTYPE, "the fields of an alignment record are u32")
    C = al.size
    cig = np.ascontiguousarray(cigar, dtype=np.uint32).ravel()
    oidx = np.ascontiguousarray(cigar_index, dtype=np.uint64).ravel()
    ht = records(hits, HIT_DTYPE, "the fields of a hit are u32")
    hidx = np.ascontiguousarray(hit_index, dtype=np.uint64).ravel()
    pr = None if pairs is None else records(pairs, PAIR_DTYPE, "the fields of a pair are u32")
    src = None if source is None else np.ascontiguousarray(source, dtype=np.uint32).ravel()
    mdb = None if md is None else np.ascontiguousarray(md, dtype=np.uint8).ravel()
    midx = None if md is None else np.ascontiguousarray(md_index, dtype=np.uint64).ravel()
    rn, rnidx = name_index(ref_names)
    R = rnidx.size - 1
    bnd = np.ascontiguousarray(bounds if bounds is not None else [0], dtype=np.uint64).ravel()
    if noff.size != Q or nlen.size != Q or hidx.size != Q + 1 or oidx.size != C + 1:
        raise ValueError("names has Q entries, hit_index Q + 1, cigar_index C + 1")
    if R and bnd.size != R + 1:
        raise ValueError("bounds has R + 1 = %d entries" % (R + 1))
    if (ql is not None and ql.size < cat.size) or (pr is not None and pr.size != Q // 2) or (src is not None and src.size != C):
        raise ValueError("qual covers the reads, pairs has Q / 2 records, source C entries")
    up = bool(np.all(ridx[1:] >= ridx[:-1]) and np.all(hidx[1:] >= hidx[:-1]) and np.all(oidx[1:] >= oidx[:-1]))
    if up:  # (what decreases the library refuses; what points past an array it would read)
        H = int(hidx[-1])
        if int(ridx[-1]) > cat.size or H > ht.size or int(oidx[-1]) > cig.size or (Q and int((noff + nlen).max()) > raw.size):
            raise ValueError("an index points past its array")
        if midx is not None and (midx.size != H + 1 or (np.all(midx[1:] >= midx[:-1]) and int(midx[-1]) > mdb.size)):
            raise ValueError("md_index has H + 1 entries and points inside md")
    keys = ("reads", "qual", "names", "name_len", "alns", "cigar", "hits", "pairs", "source", "md", "ref_names")
    ptrs, hold = addresses(cat, ql, raw, nlen, al, cig, ht, pr, src, mdb, rn if R else None)
    p = dict(zip(keys, ptrs))
    # (the index arrays are never empty, but name_off is with Q = 0)
    (p["name_off"],), hold2 = addresses(noff)
    p.update(read_index=ridx.ctypes.data, cigar_index=oidx.ctypes.data, hit_index=hidx.ctypes.data,
             md_index=None if midx is None else midx.ctypes.data, ref_name_index=rnidx.ctypes.data if R else None,
             bounds=bnd.ctypes.data if R else None)
    inp = sam_input(p, Q, C, R, first_alns)
    return inp, Q, (hold, hold2, cat, ridx, ql, raw, noff, nlen, al, cig, oidx, ht, hidx, pr, src, mdb, midx, rn, rnidx, bnd)


def sam_lines(reads, read_index, names, alns, cigar, cigar_index, hits, hit_index, qual=None, pairs=None, source=None, first_alns=0, md=None,
              md_index=None, ref_names=None, bounds=None, device=0, hooks=None):
    """The alignment lines of a batch given as arrays (numpy in, numpy out), through the host entry.  The arrays are those of
    include/kiss_hip_sam.h: alns / hits / pairs the structured arrays of the calls or (n, 12) / (n, 8) / (n, 10) integer arrays in
    the order of their fields; names a list of str or bytes or the (raw, name_off, name_len) triple of parse_reads; ref_names a
    list of R names with bounds (R + 1), or None.  Returns dict(sam: the bytes as uint8, line_index, read_line, report).  A batch
    with a bad read (see the header) raises KissHipError; its report is the exception's `report`."""
    inp, Q, hold = _host_input(reads, read_index, names, alns, cigar, cigar_index, hits, hit_index, qual, pairs, source, first_alns, md, md_index,
                               ref_names, bounds)
    lib = _lib.load(hooks)
    rep = _lib.SamReport()
    rl = np.zeros(Q + 1, np.uint64)

    def call(sam, cap, li, lcap):
        return lib.kiss_hip_fmi_sam_host(ctypes.byref(inp), sam.ctypes.data, cap, li.ctypes.data, lcap, rl.ctypes.data, ctypes.byref(rep), int(device))

    rc, (sam, _, li, _) = sized(call, lambda m=0, lines=0: (np.zeros(max(m, 1), np.uint8), m, np.zeros(lines + 1, np.uint64), lines), rep,
                               "sam_bytes", "lines")
    del hold
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        err = _lib.KissHipError(rc, "kiss_hip_fmi_sam_host", "%d bad read(s), the first one read %d" % (rep.bad, rep.first_bad))
        err.report = rep.as_dict()
        raise err
    _check(rc, "kiss_hip_fmi_sam_host")
    return {"sam": sam[:int(rep.sam_bytes)], "line_index": li, "read_line": rl, "report": rep.as_dict()}
