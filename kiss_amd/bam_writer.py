"""BAM output written on the device (include/kiss_hip_bam.h has the definition): the alignment records of a batch
(kiss_hip_fmi_bam_dev / _host) from the arrays the SAM lines are written from, and the BGZF framing of any bytes in stored blocks
with the CRC-32 of every block computed on the device (kiss_hip_bgzf_dev / _host).  bam_records() and bgzf() take numpy arrays
and run the host entries; FMIndex.map(bam=True), map_pairs(bam=True) and map_file(bam=True) keep everything on the device
(bam_records_dev, then bgzf_dev, no round trip between them); write_bam() writes a whole file.  The blocks are stored unless
compression is asked for (bgzf_deflate / bgzf_deflate_dev, map(bam_compress=True), write_bam(compress=True): DEFLATE on the device,
include/kiss_hip_deflate.h); `samtools sort` and every other BAM reader take either kind as it is.  The records
come out in read order unless they are sorted: bam_sort / bam_sort_dev put unframed records into coordinate order on the device
(kiss_hip_bam_sort_host / _dev, include/kiss_hip_bam_sort.h), map(bam_sort=True) does so for a batch and
write_bam(sort=True) for a whole file, whose header then says SO:coordinate.  A sorted file gets its BAI index from bam_index /
bam_index_dev (kiss_hip_bai_host / _dev, include/kiss_hip_bai.h): write_bam(sort=True, bai=True) writes FILE.bai
beside the file, built on the device from the sorted records and the offsets of their blocks.  Duplicate templates get FLAG 0x400
from bam_markdup / bam_markdup_dev (kiss_hip_bam_markdup_host / _dev, include/kiss_hip_markdup.h) while the records
are still in the order they were written: map(bam_markdup=True) for a batch, write_bam(sort=True, markdup=True) for a whole file.
All arithmetic runs in libkiss_hip.so; there is no CPU path."""
import ctypes
import os
import struct

import numpy as np

from . import _lib
from ._frame import sized
from .fm_sam import _bytes, sam_header as _sam_header
from .sam_writer import _host_input, sam_input
from .sorter import _check

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


SORT_ORDERS = ("unsorted", "coordinate")


def sam_header(ref_names, bounds, version, sort_order="unsorted"):
    """kiss_amd.sam_header -- @HD, one @SQ per record, @PG, as bytes -- with the SO: word of the @HD line chosen: "coordinate" for
    records that bam_sort has put in order.  Only that word changes; the default is kiss_amd.sam_header byte for byte"""
    if sort_order not in SORT_ORDERS:
        raise ValueError("sort_order is one of %s" % ", ".join(SORT_ORDERS))
    text = _sam_header(ref_names, bounds, version)
    first, rest = text.split(b"\n", 1)
    assert first.endswith(b"\tSO:unsorted")
    return first[:-len(b"unsorted")] + sort_order.encode() + b"\n" + rest


def bam_header(ref_names, bounds, version, sort_order="unsorted"):
    """the BAM header, unframed: the magic, the text of sam_header (sort_order: its SO: word), and the records with their lengths
    bounds[r + 1] - bounds[r]"""
    text = sam_header(ref_names, bounds, version, sort_order)
    text = text if isinstance(text, bytes) else str(text).encode()
    names = [_bytes(x) for x in ref_names]
    b = np.ascontiguousarray(bounds, dtype=np.uint64).ravel()
    if b.size != len(names) + 1:
        raise ValueError("bounds has R + 1 = %d entries" % (len(names) + 1))
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(names))]
    for r, nm in enumerate(names):
        l_ref = int(b[r + 1]) - int(b[r])
        if l_ref < 0 or l_ref >= 1 << 31:
            raise ValueError("record %d has %d bases: a BAM header holds fewer than 2^31" % (r, l_ref))
        out += [struct.pack("<i", len(nm) + 1), nm, b"\0", struct.pack("<i", l_ref)]
    return b"".join(out)


def _refuse_bad(rc, rep, entry):
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        err = _lib.KissHipError(rc, entry, "%d bad read(s), the first one read %d" % (rep.bad, rep.first_bad))
        err.report = rep.as_dict()
        raise err


def bam_records(reads, read_index, names, alns, cigar, cigar_index, hits, hit_index, qual=None, pairs=None, source=None, first_alns=0, md=None,
                md_index=None, ref_names=None, bounds=None, device=0, hooks=None):
    """The BAM records of a batch given as arrays (numpy in, numpy out), through the host entry; the arguments are those of
    sam_writer.sam_lines, and ref_names with bounds is required.  Returns dict(bam: the records as uint8, rec_index, read_rec,
    report).  A batch with a bad read (see the header) raises KissHipError; its report is the exception's `report`."""
    inp, Q, hold = _host_input(reads, read_index, names, alns, cigar, cigar_index, hits, hit_index, qual, pairs, source, first_alns, md, md_index,
                               ref_names, bounds)
    lib = _lib.load(hooks)
    rep = _lib.BamReport()
    rr = np.zeros(Q + 1, np.uint64)

    def call(bam, cap, ri, rcap):
        return lib.kiss_hip_fmi_bam_host(ctypes.byref(inp), bam.ctypes.data, cap, ri.ctypes.data, rcap, rr.ctypes.data, ctypes.byref(rep), int(device))

    rc, (bam, _, ri, _) = sized(call, lambda m=0, recs=0: (np.zeros(max(m, 1), np.uint8), m, np.zeros(recs + 1, np.uint64), recs), rep,
                               "bam_bytes", "records")
    del hold
    _refuse_bad(rc, rep, "kiss_hip_fmi_bam_host")
    _check(rc, "kiss_hip_fmi_bam_host")
    return {"bam": bam[:int(rep.bam_bytes)], "rec_index": ri, "read_rec": rr, "report": rep.as_dict()}


def bam_records_dev(lib, ctx, device, Q, C, R, first_alns=0, want_rec_index=True, stream=None, **tensors):
    """the device entry on torch tensors -> dict of torch tensors (d_bam, d_rec_index, d_read_rec) and the report; two calls, the
    first one sizes the bytes and the records.  tensors: the arrays of kiss_hip_sam_input by their names (None: NULL).  stream:
    None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.BamReport()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    inp = sam_input({k: (None if t is None else t.data_ptr()) for k, t in tensors.items()}, Q, C, R, first_alns)
    d_rr = torch.zeros(Q + 1, dtype=torch.int64, device=dev)

    def call(d_bam, cap, d_ri, rcap):
        return lib.kiss_hip_fmi_bam_dev(ctx._ctx, ctypes.byref(inp), vp(d_bam.data_ptr()), cap, vp(d_ri.data_ptr()) if d_ri is not None else None,
                                        rcap, vp(d_rr.data_ptr()), ctypes.byref(rep), vp(stream) if stream else None)

    def room(m=0, recs=0):
        return (torch.zeros(max(m, 1), dtype=torch.uint8, device=dev), m,
                torch.zeros(recs + 1, dtype=torch.int64, device=dev) if want_rec_index else None, recs)

    rc, (d_bam, _, d_ri, _) = sized(call, room, rep, "bam_bytes", "records")
    _refuse_bad(rc, rep, "kiss_hip_fmi_bam_dev")
    _check(rc, "kiss_hip_fmi_bam_dev", ctx._ctx)
    return {"d_bam": d_bam, "d_rec_index": d_ri, "d_read_rec": d_rr, "rep": rep, "keep": tensors}


def _refuse_unsortable(rc, rep, entry):
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        err = _lib.KissHipError(rc, entry, "%d bad record(s), the first one record %d" % (rep.bad, rep.first_bad))
        err.report = rep.as_dict()
        raise err


def bam_sort(bam, rec_index, n_ref, device=0, hooks=None):
    """Unframed BAM records (bam: bytes or a uint8 array; rec_index: records + 1, the CSR over them, as bam_records gives both) in
    coordinate order -- reference, then position, the records without a place last, equal places in input order --, sorted on the
    device through the host entry.  n_ref: the references of the header.  Returns dict(bam: the sorted records as uint8, rec_index:
    their CSR, order: order[s] is the input index of the record in slot s, report).  Input that is not such records (see the
    header) raises KissHipError; its report is the exception's `report`."""
    raw = np.frombuffer(bam, np.uint8) if isinstance(bam, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bam, dtype=np.uint8).ravel()
    ri = np.ascontiguousarray(rec_index, dtype=np.uint64).ravel()
    if ri.size < 1:
        raise ValueError("rec_index has records + 1 entries")
    records = ri.size - 1
    out = np.zeros(max(raw.size, 1), np.uint8)
    out_index = np.zeros(records + 1, np.uint64)
    order = np.zeros(max(records, 1), np.uint32)
    rep = _lib.BamSortReport()
    rc = _lib.load(hooks).kiss_hip_bam_sort_host(raw.ctypes.data if raw.size else None, raw.size, ri.ctypes.data, records, int(n_ref), out.ctypes.data,
                                                raw.size, out_index.ctypes.data, order.ctypes.data, ctypes.byref(rep), int(device))
    _refuse_unsortable(rc, rep, "kiss_hip_bam_sort_host")
    _check(rc, "kiss_hip_bam_sort_host")
    return {"bam": out[:raw.size], "rec_index": out_index, "order": order[:records], "report": rep.as_dict()}


def bam_sort_dev(lib, ctx, device, d_bam, n, d_rec_index, records, n_ref, want_order=True, stream=None):
    """the device entry on torch tensors: the first n bytes of the uint8 tensor d_bam and the int64 tensor d_rec_index (records + 1)
    -> dict of d_bam (n sorted bytes), d_rec_index (records + 1), d_order (records, int32 holding u32; None without want_order) and
    rep.  ctx sorts the records in its work arrays: one made for max_n >= 3.3 * records holds them.  stream: None, the current
    stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    n, records = int(n), int(records)
    d_out = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_index = torch.zeros(records + 1, dtype=torch.int64, device=dev)
    d_order = torch.zeros(max(records, 1), dtype=torch.int32, device=dev) if want_order else None
    rep = _lib.BamSortReport()
    rc = lib.kiss_hip_bam_sort_dev(ctx._ctx, vp(d_bam.data_ptr()) if n else None, n, vp(d_rec_index.data_ptr()), records, int(n_ref),
                                   vp(d_out.data_ptr()), n, vp(d_index.data_ptr()), vp(d_order.data_ptr()) if want_order else None,
                                   ctypes.byref(rep), vp(stream) if stream else None)
    _refuse_unsortable(rc, rep, "kiss_hip_bam_sort_dev")
    _check(rc, "kiss_hip_bam_sort_dev", ctx._ctx)
    return {"d_bam": d_out[:n] if n else d_out, "d_rec_index": d_index, "d_order": d_order[:records] if want_order else None, "rep": rep}


def _refuse_unmarkable(rc, rep, entry):
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        err = _lib.KissHipError(rc, entry, "%d bad record(s), the first one record %d" % (rep.bad, rep.first_bad))
        err.report = rep.as_dict()
        raise err


def _min_qual(min_qual):
    q = int(min_qual)
    if not 0 <= q < 1 << 32:
        raise ValueError("min_qual is 0 .. 2^32 - 1 (above 255 no quality counts)")
    return q


def bam_markdup(bam, rec_index, n_ref, min_qual=15, device=0, hooks=None):
    """The duplicate templates of unframed BAM records marked with FLAG 0x400 on the device, through the host entry
    (kiss_hip_bam_markdup_host; include/kiss_hip_markdup.h has the definition).  bam, rec_index: as bam_records gives both, IN THAT
    ORDER -- the records of a read together, the mates of a pair adjacent -- and not sorted.  min_qual: a quality counts towards a
    template's score from here (15: Picard's SUM_OF_BASE_QUALITIES).  Returns dict(bam: the marked records as uint8, dup: one byte
    per record, 1 for a record of a duplicate template, report).  Input that is not such records raises KissHipError; its report
    is the exception's `report`."""
    raw = np.array(np.frombuffer(bam, np.uint8) if isinstance(bam, (bytes, bytearray, memoryview)) else np.asarray(bam, dtype=np.uint8).ravel())
    ri = np.ascontiguousarray(rec_index, dtype=np.uint64).ravel()
    if ri.size < 1:
        raise ValueError("rec_index has records + 1 entries")
    records = ri.size - 1
    dup = np.zeros(max(records, 1), np.uint8)
    rep = _lib.MarkdupReport()
    rc = _lib.load(hooks).kiss_hip_bam_markdup_host(raw.ctypes.data if raw.size else None, raw.size, ri.ctypes.data, records, int(n_ref),
                                                   _min_qual(min_qual), dup.ctypes.data, ctypes.byref(rep), int(device))
    _refuse_unmarkable(rc, rep, "kiss_hip_bam_markdup_host")
    _check(rc, "kiss_hip_bam_markdup_host")
    return {"bam": raw, "dup": dup[:records], "report": rep.as_dict()}


def bam_markdup_dev(lib, ctx, device, d_bam, n, d_rec_index, records, n_ref, min_qual=15, want_dup=True, stream=None):
    """the device entry on torch tensors: the first n bytes of the uint8 tensor d_bam are marked IN PLACE; d_rec_index: int64,
    records + 1 -> dict of d_dup (records, uint8; None without want_dup) and rep.  ctx sorts the items in its work arrays, as
    bam_sort_dev has it.  stream: None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    n, records = int(n), int(records)
    d_dup = torch.zeros(max(records, 1), dtype=torch.uint8, device=dev) if want_dup else None
    rep = _lib.MarkdupReport()
    rc = lib.kiss_hip_bam_markdup_dev(ctx._ctx, vp(d_bam.data_ptr()) if n else None, n, vp(d_rec_index.data_ptr()), records, int(n_ref),
                                      _min_qual(min_qual), vp(d_dup.data_ptr()) if want_dup else None, ctypes.byref(rep),
                                      vp(stream) if stream else None)
    _refuse_unmarkable(rc, rep, "kiss_hip_bam_markdup_dev")
    _check(rc, "kiss_hip_bam_markdup_dev", ctx._ctx)
    return {"d_dup": d_dup[:records] if want_dup else None, "rep": rep}


def markdup_options(markdup):
    """markdup=True | dict(min_qual=...) -> the keyword arguments of bam_markdup_dev; False or None -> None"""
    if markdup is None or markdup is False:
        return None
    if markdup is True:
        return {"min_qual": _lib.MARKDUP_MIN_QUAL_DEFAULT}
    opts = dict(markdup)
    unknown = sorted(set(opts) - {"min_qual"})
    if unknown:
        raise ValueError("markdup takes min_qual, not %s" % ", ".join(unknown))
    return {"min_qual": _min_qual(opts.get("min_qual", _lib.MARKDUP_MIN_QUAL_DEFAULT))}


def bam_marked(lib, ctx, device, out, n_ref, min_qual=15):
    """the tensors of bam_records_dev with the duplicates of the batch marked in place (map(bam_markdup=True)): the same dict with
    d_dup and markdup_rep added"""
    if out["d_rec_index"] is None:
        raise ValueError("bam_markdup needs the record index: bam_records_dev(want_rec_index=True)")
    got = bam_markdup_dev(lib, ctx, device, out["d_bam"], int(out["rep"].bam_bytes), out["d_rec_index"], int(out["rep"].records), n_ref, min_qual)
    return dict(out, d_dup=got["d_dup"], markdup_rep=got["rep"])


def _refuse_unindexable(rc, rep, entry):
    if rc == _lib.KISS_HIP_E_INVALID and rep.bad:
        err = _lib.KissHipError(rc, entry, "%d record(s) that an index cannot hold or that are out of order, the first one record %d" % (rep.bad, rep.first_bad))
        err.report = rep.as_dict()
        raise err


def bam_index(bam, rec_index, n_ref, block_bytes=65280, block_index=None, file_base=0, device=0, hooks=None):
    """The BAI index of unframed BAM records in coordinate order (bam, rec_index: as bam_sort gives both), built on the device
    through the host entry (kiss_hip_bai_host, include/kiss_hip_bai.h).  block_bytes: the payload bytes with which the records are
    framed; block_index: the compressed offset of every block as bgzf_deflate(want_index=True) gives it (None: stored blocks);
    file_base: the bytes of the file in front of the first record block, the framed header.  Returns dict(bai: the bytes of
    FILE.bai, report).  The chunks are not merged beyond runs of one bin, so the bytes are a valid index and need not be those of
    `samtools index`.  Records that are out of order or that BAI cannot hold (see the header) raise KissHipError; its report is the
    exception's `report`."""
    raw = np.frombuffer(bam, np.uint8) if isinstance(bam, (bytes, bytearray, memoryview)) else np.ascontiguousarray(bam, dtype=np.uint8).ravel()
    ri = np.ascontiguousarray(rec_index, dtype=np.uint64).ravel()
    if ri.size < 1:
        raise ValueError("rec_index has records + 1 entries")
    bb = _block_bytes(block_bytes)
    bi = None
    if block_index is not None:
        bi = np.ascontiguousarray(block_index, dtype=np.uint64).ravel()
        if bi.size != -(-raw.size // (bb or _lib.BGZF_BLOCK_DEFAULT)) + 1:
            raise ValueError("block_index has blocks + 1 entries")
    records = ri.size - 1
    lib = _lib.load(hooks)
    rep = _lib.BaiReport()

    def call(bai, cap):
        return lib.kiss_hip_bai_host(raw.ctypes.data if raw.size else None, raw.size, ri.ctypes.data, records, int(n_ref), bb,
                                     None if bi is None else bi.ctypes.data, int(file_base), None if bai is None else bai.ctypes.data, cap,
                                     ctypes.byref(rep), int(device))

    rc, (bai, _) = sized(call, lambda m=0: (np.zeros(m, np.uint8) if m else None, m), rep, "bai_bytes")
    _refuse_unindexable(rc, rep, "kiss_hip_bai_host")
    _check(rc, "kiss_hip_bai_host")
    return {"bai": bai[:int(rep.bai_bytes)].tobytes(), "report": rep.as_dict()}


def bam_index_dev(lib, ctx, device, d_bam, n, d_rec_index, records, n_ref, block_bytes, d_block_index, file_base, stream=None):
    """the device entry on torch tensors: the first n bytes of the uint8 tensor d_bam (sorted records), the int64 tensor d_rec_index
    (records + 1), d_block_index (int64, blocks + 1, or None for stored blocks) -> (a uint8 tensor of exactly the bytes of FILE.bai,
    the report); two calls, the first one sizes the bytes.  stream: None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    n, records, bb = int(n), int(records), _block_bytes(block_bytes)
    rep = _lib.BaiReport()

    def call(d_bai, cap):
        return lib.kiss_hip_bai_dev(ctx._ctx, vp(d_bam.data_ptr()) if n else None, n, vp(d_rec_index.data_ptr()), records, int(n_ref), bb,
                                    None if d_block_index is None else vp(d_block_index.data_ptr()), int(file_base),
                                    None if d_bai is None else vp(d_bai.data_ptr()), cap, ctypes.byref(rep), vp(stream) if stream else None)

    rc, (d_bai, _) = sized(call, lambda m=0: (torch.zeros(m, dtype=torch.uint8, device=dev) if m else None, m), rep, "bai_bytes")
    _refuse_unindexable(rc, rep, "kiss_hip_bai_dev")
    _check(rc, "kiss_hip_bai_dev", ctx._ctx)
    return d_bai[:int(rep.bai_bytes)], rep


def bam_sorted(lib, ctx, device, out, n_ref):
    """the tensors of bam_records_dev with the records sorted (map(bam_sort=True)): the same dict with d_bam and d_rec_index
    replaced, d_order and sort_rep added.  It asks bam_records_dev for the record index it may have left out."""
    if out["d_rec_index"] is None:
        raise ValueError("bam_sort needs the record index: bam_records_dev(want_rec_index=True)")
    got = bam_sort_dev(lib, ctx, device, out["d_bam"], int(out["rep"].bam_bytes), out["d_rec_index"], int(out["rep"].records), n_ref)
    return dict(out, d_bam=got["d_bam"], d_rec_index=got["d_rec_index"], d_order=got["d_order"], sort_rep=got["rep"])


def _sort_counts(rep):
    return dict(unplaced=int(rep.unplaced), ms_sort_total=float(rep.ms_total), ms_sort_key=float(rep.ms_key), ms_sort=float(rep.ms_sort),
                ms_sort_copy=float(rep.ms_copy))


def bam_unframed(out):
    """the tensors of bam_records_dev as they are, for a caller that frames them later (write_bam(sort=True)): bam_dev = (the uint8
    tensor of the records, bytes, the int64 tensor of the record index, records), on the device; bam_read_rec and bam_report as
    bam_arrays gives them"""
    rep = out["rep"]
    more = {}
    if out.get("markdup_rep") is not None:
        more = {"bam_dup": out["d_dup"].cpu().numpy(), "bam_markdup_report": out["markdup_rep"].as_dict()}
    return {"bam_dev": (out["d_bam"], int(rep.bam_bytes), out["d_rec_index"], int(rep.records)),
            "bam_read_rec": out["d_read_rec"].cpu().numpy().view(np.uint64), "bam_report": rep.as_dict(), **more}


def _block_bytes(block_bytes):
    bb = int(block_bytes)
    if not 0 <= bb <= _lib.BGZF_BLOCK_MAX:
        raise ValueError("block_bytes is 1 .. %d (0: %d)" % (_lib.BGZF_BLOCK_MAX, _lib.BGZF_BLOCK_DEFAULT))
    return bb


def bgzf_bytes(n, block_bytes=65280, eof=False):
    """the bytes bgzf() makes of n"""
    bb = _block_bytes(block_bytes) or _lib.BGZF_BLOCK_DEFAULT
    return n + _lib.BGZF_OVERHEAD * (-(-n // bb)) + (_lib.BGZF_EOF_BYTES if eof else 0)


def bgzf(data, block_bytes=65280, eof=False, device=0, hooks=None, want_report=False):
    """data (bytes or a uint8 array) cut into BGZF blocks of block_bytes payload bytes, stored, each with its CRC-32, through the host
    entry -> bytes (want_report: and the report); eof: the end-of-file block behind them"""
    raw = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).ravel()
    bb = _block_bytes(block_bytes)
    out = np.zeros(max(bgzf_bytes(raw.size, bb, eof), 1), np.uint8)
    rep = _lib.BgzfReport()
    rc = _lib.load(hooks).kiss_hip_bgzf_host(raw.ctypes.data if raw.size else None, raw.size, bb, int(bool(eof)), out.ctypes.data, out.size,
                                            ctypes.byref(rep), int(device))
    _check(rc, "kiss_hip_bgzf_host")
    got = out[:int(rep.out_bytes)].tobytes()
    return (got, rep.as_dict()) if want_report else got


def bgzf_dev(lib, ctx, device, d_data, n, block_bytes=65280, eof=False, stream=None):
    """the device entry: the first n bytes of the uint8 tensor d_data -> (a uint8 tensor of exactly the blocks, the report)"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    bb = _block_bytes(block_bytes)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    total = bgzf_bytes(int(n), bb, eof)
    d_out = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
    rep = _lib.BgzfReport()
    rc = lib.kiss_hip_bgzf_dev(ctx._ctx, vp(d_data.data_ptr()) if n else None, int(n), bb, int(bool(eof)), vp(d_out.data_ptr()), total,
                               ctypes.byref(rep), vp(stream) if stream else None)
    _check(rc, "kiss_hip_bgzf_dev", ctx._ctx)
    return d_out[:int(rep.out_bytes)], rep


def bgzf_deflate(data, block_bytes=65280, eof=False, device=0, hooks=None, want_report=False, want_index=False):
    """bgzf() with the blocks compressed on the device (DEFLATE; include/kiss_hip_deflate.h), through the host entry -> bytes
    (want_index: and block_index, blocks + 1 uint64 over those bytes; want_report: and the report, in that order)"""
    raw = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).ravel()
    bb = _block_bytes(block_bytes)
    out = np.zeros(max(bgzf_bytes(raw.size, bb, eof), 1), np.uint8)
    index = np.zeros(-(-raw.size // (bb or _lib.BGZF_BLOCK_DEFAULT)) + 1, np.uint64)
    rep = _lib.BgzfDeflateReport()
    rc = _lib.load(hooks).kiss_hip_bgzf_deflate_host(raw.ctypes.data if raw.size else None, raw.size, bb, int(bool(eof)), out.ctypes.data, out.size,
                                                    index.ctypes.data, index.size, ctypes.byref(rep), int(device))
    _check(rc, "kiss_hip_bgzf_deflate_host")
    got = (out[:int(rep.out_bytes)].tobytes(),) + ((index,) if want_index else ()) + ((rep.as_dict(),) if want_report else ())
    return got if len(got) > 1 else got[0]


def bgzf_deflate_dev(lib, ctx, device, d_data, n, block_bytes=65280, eof=False, stream=None):
    """the device entry: the first n bytes of the uint8 tensor d_data -> (a uint8 tensor of exactly the blocks, block_index as an
    int64 tensor of blocks + 1, the report)"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    bb = _block_bytes(block_bytes)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    bound = bgzf_bytes(int(n), bb, eof)
    blocks = -(-int(n) // (bb or _lib.BGZF_BLOCK_DEFAULT))
    d_out = torch.zeros(max(bound, 1), dtype=torch.uint8, device=dev)
    d_index = torch.zeros(blocks + 1, dtype=torch.int64, device=dev)
    rep = _lib.BgzfDeflateReport()
    rc = lib.kiss_hip_bgzf_deflate_dev(ctx._ctx, vp(d_data.data_ptr()) if n else None, int(n), bb, int(bool(eof)), vp(d_out.data_ptr()), bound,
                                       vp(d_index.data_ptr()), blocks + 1, ctypes.byref(rep), vp(stream) if stream else None)
    _check(rc, "kiss_hip_bgzf_deflate_dev", ctx._ctx)
    return d_out[:int(rep.out_bytes)], d_index, rep


def bam_arrays(lib, ctx, device, out, block_bytes=65280, compress=False):
    """the tensors of bam_records_dev framed on the device, as what map(bam=True) adds to its result; compress: the blocks are
    compressed (bam_block_index and the counts of the coding beside them); after bam_sorted: bam_order and the sort's counts; after
    bam_marked: bam_dup and bam_markdup_report"""
    total = int(out["rep"].bam_bytes)
    ri = out["d_rec_index"]
    rep = out["rep"].as_dict()
    more = {}
    if out.get("markdup_rep") is not None:
        more["bam_dup"] = out["d_dup"].cpu().numpy()
        more["bam_markdup_report"] = out["markdup_rep"].as_dict()
    if out.get("sort_rep") is not None:
        rep.update(_sort_counts(out["sort_rep"]))
        more["bam_order"] = out["d_order"].cpu().numpy().view(np.uint32)
    if compress:
        d_blocks, d_index, frep = bgzf_deflate_dev(lib, ctx, device, out["d_bam"], total, block_bytes)
        rep.update({k: int(getattr(frep, k)) for k in ("stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches", "match_bytes")})
        more["bam_block_index"] = d_index.cpu().numpy().view(np.uint64)
    else:
        d_blocks, frep = bgzf_dev(lib, ctx, device, out["d_bam"], total, block_bytes)
    rep.update(blocks=int(frep.blocks), out_bytes=int(frep.out_bytes), ms_frame=float(frep.ms_total))
    return {"bam": d_blocks.cpu().numpy().tobytes(), "bam_rec_index": None if ri is None else ri.cpu().numpy().view(np.uint64),
            "bam_read_rec": out["d_read_rec"].cpu().numpy().view(np.uint64), "bam_report": rep, **more}


def write_bam(path, index, reads1, text, reads2=None, ref_names=None, bounds=None, version=None, compress=False, sort=False, bai=None, markdup=None,
              **params):
    """A whole BAM file of the read file(s) mapped by `index` (batches.map_file, which has the other arguments): the framed header,
    the blocks of every batch, the end-of-file block.  path: a file name, or a binary file object.  compress: the header and the
    batches in compressed blocks (bgzf_deflate, map_file(bam_compress=True)).  -> the batches, records and bytes written.
    sort: the records of the WHOLE file in coordinate order and SO:coordinate in the header.  The unframed records and the record
    index of every batch then stay on the device; behind the last batch they are concatenated, sorted once (bam_sort_dev) and
    framed once, and only then is anything written to path.  Device memory: about twice the file's uncompressed record bytes (the
    records and their sorted copy; while the batches are concatenated, or the blocks framed, one of the two is held a second time)
    plus 12 bytes per record (the index and the permutation), beside the sort's work arrays.  When that memory is not there
    MemoryError names the bytes asked for and nothing has been written.  The result also carries sort_report.
    bai (with sort=True): the BAI index of the file, built on the device from the sorted records, their index and the offsets of
    the blocks (bam_index_dev; include/kiss_hip_bai.h) before anything is written.  True: written to str(path) + ".bai", which needs
    path to be a file name; a file name; or a binary file object.  The result then carries bai_bytes and bai_report.  The index is
    valid per the specification; its bytes need not be those of `samtools index`, which merges more chunks.
    markdup (with sort=True): True or dict(min_qual=15): the duplicate templates of the WHOLE file get FLAG 0x400 on the device
    (bam_markdup_dev; include/kiss_hip_markdup.h has the definition), on the concatenated records directly before they are sorted:
    the batches are cut at read or pair boundaries, so the records of a template are still together there.  Only bytes 18 - 19 of
    records change: the blocks of a stored file and the index are what they are without it.  The result then carries
    markdup_report.  Without sort=True it is a ValueError: the unsorted path does not hold the file on the device."""
    from .batches import map_file
    if ref_names is None or bounds is None:
        raise ValueError("a BAM file needs ref_names and bounds")
    named = isinstance(path, (str, bytes)) or hasattr(path, "__fspath__")
    if bai is False:
        bai = None
    if bai is not None and not sort:
        raise ValueError("write_bam(bai=...) indexes a sorted file: it goes with sort=True")
    mark = markdup_options(markdup)
    if mark is not None and not sort:
        raise ValueError("write_bam(markdup=...) marks the duplicates of the whole file, which only the sorted path holds on the device: it goes "
                         "with sort=True")
    if bai is True:
        if not named:
            raise ValueError("write_bam(bai=True) writes the index beside the file: path must be a file name (or give bai a name or a file object)")
        bai = os.fsdecode(path) + ".bai"
    if version is None:  # (@PG VN: the library's version number, as kiss_hip_version() gives it)
        version = str(_lib.load(index._hooks).kiss_hip_version())
    frame = bgzf_deflate if compress else bgzf
    head = frame(bam_header(ref_names, bounds, version, "coordinate" if sort else "unsorted"), device=index.device, hooks=index._hooks)
    if compress and not sort:
        params["bam_compress"] = True
    done = {"batches": 0, "records": 0, "bytes": len(head)}
    if sort:
        blocks, done["sort_report"], index_bytes = _sorted_file(index, len(ref_names), compress,
                                                                map_file(index, reads1, text, reads2, bam=True, _bam_unframed=True, ref_names=ref_names,
                                                                         bounds=bounds, **params), done, len(head) if bai is not None else None,
                                                                mark)
    f = open(path, "wb") if named else path
    try:
        f.write(head)
        if sort:
            f.write(blocks)
            done["bytes"] += len(blocks)
        else:
            for res in map_file(index, reads1, text, reads2, bam=True, ref_names=ref_names, bounds=bounds, **params):
                f.write(res["bam"])
                done["batches"] += 1
                done["records"] += int(res["bam_report"]["records"])
                done["bytes"] += len(res["bam"])
        f.write(BGZF_EOF)
        done["bytes"] += len(BGZF_EOF)
    finally:
        if f is not path:
            f.close()
    if bai is not None:  # (behind the file it indexes)
        if isinstance(bai, (str, bytes)) or hasattr(bai, "__fspath__"):
            with open(bai, "wb") as g:
                g.write(index_bytes)
        else:
            bai.write(index_bytes)
    return done


def _sorted_file(index, n_ref, compress, batches, done, file_base=None, mark=None):
    """write_bam(sort=True): the records of all `batches` (results of map_file(_bam_unframed=True)) sorted and framed on the device
    -> (the blocks as bytes, the sort's report, the bytes of the index or None); done: the counts so far; file_base: the bytes of the
    framed header when the index is wanted (done then gains bai_bytes and bai_report); mark: the keyword arguments of
    bam_markdup_dev when the duplicates are to be marked (done then gains markdup_report)"""
    import torch
    dev = torch.device("cuda", index.device)
    parts, total, records = [], 0, 0
    for res in batches:
        d_bam, n, d_ri, recs = res["bam_dev"]
        done["batches"] += 1
        if recs:
            parts.append((d_bam[:n], d_ri[1:recs + 1] + total))  # (the index of the batch rebased onto the bytes in front of it)
            total += n
            records += recs
    done["records"] = records
    asked = 2 * total + 12 * records + 8
    lib = _lib.load(index._hooks)
    try:
        d_all = torch.cat([p[0] for p in parts]) if parts else torch.zeros(1, dtype=torch.uint8, device=dev)
        d_index = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev)] + [p[1] for p in parts])
        del parts
        ctx = index._context_to_sort(index._context(1 << 20), records)
        if mark is not None:  # (in place, while the records are in the order they were written)
            done["markdup_report"] = bam_markdup_dev(lib, ctx, index.device, d_all, total, d_index, records, n_ref, want_dup=False, **mark)["rep"].as_dict()
        got = bam_sort_dev(lib, ctx, index.device, d_all, total, d_index, records, n_ref, want_order=False)
        del d_all, d_index
        d_block_index = None
        if compress:
            d_blocks, d_block_index, _ = bgzf_deflate_dev(lib, ctx, index.device, got["d_bam"], total)
        else:
            d_blocks, _ = bgzf_dev(lib, ctx, index.device, got["d_bam"], total)
        index_bytes = None
        if file_base is not None:
            d_bai, brep = bam_index_dev(lib, ctx, index.device, got["d_bam"], total, got["d_rec_index"], records, n_ref, 65280, d_block_index, file_base)
            index_bytes = d_bai.cpu().numpy().tobytes()
            done["bai_bytes"], done["bai_report"] = len(index_bytes), brep.as_dict()
    except torch.cuda.OutOfMemoryError:
        raise MemoryError("write_bam(sort=True): the device does not hold the %d bytes the sort asks for (%d record bytes twice, 12 bytes for "
                          "each of %d records)" % (asked, total, records)) from None
    except _lib.KissHipError as e:
        if e.status == _lib.KISS_HIP_E_NOMEM:
            raise MemoryError("write_bam(sort=True): the device does not hold the %d bytes the sort asks for" % asked) from None
        raise
    return d_blocks.cpu().numpy().tobytes(), dict(got["rep"].as_dict()), index_bytes
