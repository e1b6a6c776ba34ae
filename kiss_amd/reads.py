"""Files of reads parsed on the GPU: one read per line, or FASTQ (kiss_hip_reads_parse_* / kiss_hip_reads_interleave_*;
include/kiss_hip_reads.h has the definition, tests/reads_model.py restates it).

parse_reads() takes the bytes of a file, or its path, and returns host arrays: (reads, read_index) is what FMIndex.seeds / map /
map_pairs take as they are.  parse_reads_dev() and interleave_reads_dev() work on torch tensors that stay on the device, on the
current torch stream.  Every byte is looked at in libkiss_hip.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._frame import addresses
from .sorter import _check

FORMATS = {"auto": _lib.READS_AUTO, "lines": _lib.READS_LINES, "fastq": _lib.READS_FASTQ}
FORMAT_NAMES = {_lib.READS_LINES: "lines", _lib.READS_FASTQ: "fastq"}
BAD_KINDS = {1: "line 1 of the record does not start with '@'", 2: "line 3 of the record does not start with '+'",
             3: "sequence and quality string differ in length", 4: "the file ends inside the record"}


def _format(fmt):
    if fmt not in FORMATS:
        raise ValueError("format is one of %s, not %r" % (", ".join(sorted(FORMATS)), fmt))
    return FORMATS[fmt]


def _report(rep):
    d = rep.as_dict()
    d["format"] = FORMAT_NAMES[d["format"]]
    for k in ("first_empty", "first_bad"):
        if d[k] == _lib.READS_NONE:
            d[k] = None
    return d


def _refuse_bad(rc, rep, where):
    """the message of a call that met bad records; any other failure as every call reports it"""
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad_records:
        raise ValueError("%s: %d bad FASTQ records, the first is record %d: %s"
                         % (where, rep.bad_records, rep.first_bad, BAD_KINDS.get(rep.first_bad_kind, "?")))
    _check(rc, where)


def names_of(raw, name_off, name_len):
    """the names of the reads from their spans in the file's bytes; the decimal read number where the span is empty"""
    buf = bytes(raw)
    return [buf[int(o):int(o) + int(n)].decode("latin-1") if n else str(q) for q, (o, n) in enumerate(zip(name_off, name_len))]


def parse_reads(source, format="auto", want_qual=True, want_names=True, ctx=None, device=0, hooks=None):
    """The reads of a file.  source: bytes, or a path.  format: "auto" (FASTQ iff the first byte is '@'), "lines", "fastq".
    ctx: a Context whose device and scratch the parse uses (its max_n at least four times the file's bytes); None: the
    library's own one-shot context on `device`.
    Returns dict(reads: the base codes of all reads one after the other (uint8; 4: no base), read_index (Q + 1, uint64), qual
    (the quality bytes at the same offsets, or None: a lines file, or want_qual=False), names (list of str, the read number
    where the file gives none; None with want_names=False), report).  (reads, read_index) goes into FMIndex.seeds / map /
    map_pairs as it is.  Bad FASTQ records raise ValueError naming the first one."""
    fmt = _format(format)
    if isinstance(source, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(bytes(source), np.uint8)
    else:
        with open(os.fspath(source), "rb") as f:
            raw = np.frombuffer(f.read(), np.uint8)
    if ctx is not None:
        return _parse_on_ctx(raw, format, want_qual, want_names, ctx)
    lib = _lib.load(hooks)
    rep = _lib.ReadsReport()

    def call(codes, qual, bases_cap, index, noff, nlen, reads_cap):
        p, hold = addresses(raw, codes, qual, index, noff, nlen)
        return lib.kiss_hip_reads_parse_host(p[0], raw.size, fmt, p[1], p[2], bases_cap, p[3], p[4], p[5], reads_cap, ctypes.byref(rep),
                                             int(device))

    index = np.zeros(1, np.uint64)
    rc = call(np.zeros(0, np.uint8), None, 0, index, None, None, 0)  # size ...
    codes, qual, noff, nlen = np.zeros(0, np.uint8), None, None, None
    if rc == _lib.KISS_HIP_E_INVALID and not rep.bad_records and (rep.reads or rep.bases):  # ... then fill
        Q, B = int(rep.reads), int(rep.bases)
        codes, index = np.zeros(B, np.uint8), np.zeros(Q + 1, np.uint64)
        qual = np.zeros(B, np.uint8) if want_qual and rep.has_qual else None
        noff, nlen = (np.zeros(Q, np.uint64), np.zeros(Q, np.uint32)) if want_names else (None, None)
        rc = call(codes, qual, B, index, noff, nlen, Q)
    _refuse_bad(rc, rep, "kiss_hip_reads_parse_host")
    names = None
    if want_names:
        names = names_of(raw, noff, nlen) if noff is not None else []
    return {"reads": codes, "read_index": index, "qual": qual, "names": names, "report": _report(rep)}


def _parse_on_ctx(raw, format, want_qual, want_names, ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    d_raw = torch.from_numpy(raw.copy()).to(dev) if raw.size else torch.zeros(0, dtype=torch.uint8, device=dev)
    out = parse_reads_dev(d_raw, format, want_qual, want_names, ctx)
    names = None
    if want_names:
        names = names_of(raw, out["name_off"].cpu().numpy().view(np.uint64), out["name_len"].cpu().numpy().view(np.uint32))
    return {"reads": out["reads"].cpu().numpy(), "read_index": out["read_index"].cpu().numpy().view(np.uint64),
            "qual": out["qual"].cpu().numpy() if out["qual"] is not None else None, "names": names, "report": out["report"]}


def parse_reads_dev(d_raw, format="auto", want_qual=True, want_names=True, ctx=None):
    """The same on the device: d_raw is a uint8 torch tensor with the file's bytes, the work runs on the current torch stream
    with the scratch of `ctx` (a Context, required).  Returns dict(reads (uint8 tensor), read_index (int64 tensor, Q + 1), qual
    (uint8 tensor or None), name_off (int64) / name_len (int32): the spans of the names inside d_raw, or None, report)."""
    import torch
    if ctx is None:
        raise ValueError("parse_reads_dev needs a Context")
    fmt = _format(format)
    if d_raw.dtype != torch.uint8 or d_raw.dim() != 1 or not d_raw.is_contiguous():
        raise ValueError("d_raw is a contiguous one-dimensional uint8 tensor")
    lib, dev, vp = ctx._lib, d_raw.device, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    rep = _lib.ReadsReport()
    ptr = lambda t: vp(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731

    def call(codes, qual, bases_cap, index, noff, nlen, reads_cap):
        return lib.kiss_hip_reads_parse_dev(ctx._ctx, ptr(d_raw), d_raw.numel(), fmt, ptr(codes), ptr(qual), bases_cap, vp(index.data_ptr()),
                                            ptr(noff), ptr(nlen), reads_cap, ctypes.byref(rep), stream)

    index = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = call(None, None, 0, index, None, None, 0)  # size ...
    codes, qual, noff, nlen = torch.zeros(0, dtype=torch.uint8, device=dev), None, None, None
    if want_names:
        noff, nlen = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    if rc == _lib.KISS_HIP_E_INVALID and not rep.bad_records and (rep.reads or rep.bases):  # ... then fill
        Q, B = int(rep.reads), int(rep.bases)
        codes, index = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        qual = torch.zeros(B, dtype=torch.uint8, device=dev) if want_qual and rep.has_qual else None
        if want_names:  # (one entry more than there are reads: a pointer that is not NULL when Q is 0)
            noff, nlen = torch.zeros(Q + 1, dtype=torch.int64, device=dev), torch.zeros(Q + 1, dtype=torch.int32, device=dev)
        rc = call(codes, qual, B, index, noff, nlen, Q)
        if want_names:
            noff, nlen = noff[:Q], nlen[:Q]
    _refuse_bad(rc, rep, "kiss_hip_reads_parse_dev")
    return {"reads": codes, "read_index": index, "qual": qual, "name_off": noff, "name_len": nlen, "report": _report(rep)}


def _batch(x):
    """(reads, read_index, qual or None) of a result of parse_reads, or of a tuple"""
    if isinstance(x, dict):
        return x["reads"], x["read_index"], x.get("qual")
    return (tuple(x) + (None,))[:3]


def interleave_reads(a, b, device=0, hooks=None):
    """Two parsed batches (the dicts of parse_reads, or (reads, read_index[, qual]) tuples) of P reads each -> one batch of 2 P:
    read 2 p is read p of a, read 2 p + 1 read p of b, as FMIndex.map_pairs and kiss_hip_fmi_pair_* expect mates.  qual: of
    both or of neither.  Returns dict(reads, read_index, qual); names (if both are dicts with names) are interleaved too."""
    ca, ia, qa = _batch(a)
    cb, ib, qb = _batch(b)
    ca, cb = np.ascontiguousarray(ca, np.uint8), np.ascontiguousarray(cb, np.uint8)
    ia, ib = np.ascontiguousarray(ia, np.uint64).ravel(), np.ascontiguousarray(ib, np.uint64).ravel()
    if ia.size < 1 or ib.size < 1:
        raise ValueError("a read index has Q + 1 entries")
    if (qa is None) != (qb is None):
        raise ValueError("qualities of both batches, or of neither")
    Pa, Pb = ia.size - 1, ib.size - 1
    if Pa != Pb:
        raise ValueError("%d reads and %d reads: a pair has one of each" % (Pa, Pb))
    if int(ia[-1]) > ca.size or int(ib[-1]) > cb.size or (qa is not None and (len(qa) < int(ia[-1]) or len(qb) < int(ib[-1]))):
        raise ValueError("a read index points past its reads")
    lib = _lib.load(hooks)
    total = int(ia[-1]) + int(ib[-1])
    codes, index = np.zeros(total, np.uint8), np.zeros(Pa + Pb + 1, np.uint64)
    qual = None
    if qa is not None:
        qa, qb, qual = np.ascontiguousarray(qa, np.uint8), np.ascontiguousarray(qb, np.uint8), np.zeros(total, np.uint8)
    got = ctypes.c_uint64()
    p, hold = addresses(ca, ia, qa, cb, ib, qb, codes, index, qual)
    _check(lib.kiss_hip_reads_interleave_host(p[0], p[1], p[2], Pa, p[3], p[4], p[5], Pb, p[6], p[7], p[8], total, ctypes.byref(got),
                                              int(device)), "kiss_hip_reads_interleave_host")
    res = {"reads": codes, "read_index": index, "qual": qual}
    if isinstance(a, dict) and isinstance(b, dict) and a.get("names") is not None and b.get("names") is not None:
        res["names"] = [n for pair in zip(a["names"], b["names"]) for n in pair]
    return res


def interleave_reads_dev(a, b, ctx):
    """The same on device tensors (the dicts of parse_reads_dev, or tuples), on the current torch stream."""
    import torch
    ca, ia, qa = _batch(a)
    cb, ib, qb = _batch(b)
    if (qa is None) != (qb is None):
        raise ValueError("qualities of both batches, or of neither")
    Pa, Pb = ia.numel() - 1, ib.numel() - 1
    if Pa != Pb:
        raise ValueError("%d reads and %d reads: a pair has one of each" % (Pa, Pb))
    dev, vp = ia.device, ctypes.c_void_p
    total = ca.numel() + cb.numel()
    codes = torch.zeros(total, dtype=torch.uint8, device=dev)
    index = torch.zeros(Pa + Pb + 1, dtype=torch.int64, device=dev)
    qual = torch.zeros(total, dtype=torch.uint8, device=dev) if qa is not None else None
    keep = torch.zeros(1, dtype=torch.uint8, device=dev)  # (a pointer that is not NULL for an array without entries)
    ptr = lambda t: None if t is None else vp(t.data_ptr() if t.numel() else keep.data_ptr())  # noqa: E731
    got = ctypes.c_uint64()
    _check(ctx._lib.kiss_hip_reads_interleave_dev(ctx._ctx, ptr(ca), vp(ia.data_ptr()), ptr(qa), Pa, ptr(cb), vp(ib.data_ptr()), ptr(qb), Pb,
                                                  ptr(codes), vp(index.data_ptr()), ptr(qual), total, ctypes.byref(got),
                                                  vp(torch.cuda.current_stream(dev).cuda_stream)),
           "kiss_hip_reads_interleave_dev", ctx._ctx)
    return {"reads": codes[:got.value], "read_index": index, "qual": qual[:got.value] if qual is not None else None}
