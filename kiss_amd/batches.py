"""A read file of any size parsed and mapped in batches (kiss_hip_reads_parse_part_*; include/kiss_hip_reads_part.h has the
definition, tests/reads_part_model.py restates it).

parse_reads_part() / parse_reads_part_dev() parse the first whole records of a chunk of a read file and say where the next chunk
starts; read_batches() is the loop around them: a generator over the parsed batches of one file, or of the two files of mates;
map_file() runs FMIndex.map / map_pairs on every batch, with the index and the text staying on the device.  Every byte is looked at
in libkiss_hip.so; there is no CPU path.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._frame import addresses
from .reads import BAD_KINDS, _format, _report, interleave_reads_dev
from .sorter import _check


def _part_report(rep):
    d = _report(rep.parsed)
    d.update(records_complete=int(rep.records_complete), records=int(rep.records), bytes_used=int(rep.bytes_used))
    return d


def _refuse_bad_part(rc, rep, where, first_read):
    """_refuse_bad with the number of the record in the file: first_read records were consumed before this chunk"""
    if rc == _lib.KISS_HIP_E_INVALID and rep.parsed.bad_records:
        raise ValueError("%s: bad FASTQ records, the first is record %d: %s"
                         % (where, int(first_read) + rep.parsed.first_bad, BAD_KINDS.get(rep.parsed.first_bad_kind, "?")))
    _check(rc, where)


def _part_arguments(format, max_records):
    if int(max_records) < 0:
        raise ValueError("max_records is 0 (every whole record of the chunk) or a count")
    return _format(format), int(max_records)


def _numbered_names(raw, name_off, name_len, first_read=0):
    """names_of() for a chunk: a read without a name gets its number in the file, first_read + its number in the chunk"""
    buf = bytes(raw)
    return [buf[int(o):int(o) + int(n)].decode("latin-1") if n else str(first_read + q) for q, (o, n) in enumerate(zip(name_off, name_len))]


def parse_reads_part(chunk, format="auto", final=True, max_records=0, want_qual=True, want_names=True, first_read=0, device=0, hooks=None):
    """The first whole records of a chunk of a read file (bytes): what parse_reads returns for them, and in report
    records_complete (the whole records of the chunk), records (those parsed: at most max_records when that is not 0) and
    bytes_used (where the next chunk starts; 0 records and 0 bytes without `final`: the chunk is too short for one record).
    final: the chunk reaches the end of the file.  first_read: the records consumed before the chunk; default names and the
    record number of an error count from it.  format "auto" looks at the first byte of the chunk: resolve it on the first chunk
    (report["format"]) and name it afterwards."""
    fmt, max_records = _part_arguments(format, max_records)
    raw = np.frombuffer(bytes(chunk), np.uint8)
    lib = _lib.load(hooks)
    rep = _lib.ReadsPartReport()

    def call(codes, qual, bases_cap, index, noff, nlen, reads_cap):
        p, hold = addresses(raw, codes, qual, index, noff, nlen)
        return lib.kiss_hip_reads_parse_part_host(p[0], raw.size, fmt, 1 if final else 0, max_records, p[1], p[2], bases_cap, p[3], p[4], p[5],
                                                  reads_cap, ctypes.byref(rep), int(device))

    index = np.zeros(1, np.uint64)
    rc = call(np.zeros(0, np.uint8), None, 0, index, None, None, 0)  # size ...
    codes, qual, noff, nlen = np.zeros(0, np.uint8), None, None, None
    if rc == _lib.KISS_HIP_E_INVALID and not rep.parsed.bad_records and (rep.parsed.reads or rep.parsed.bases):  # ... then fill
        Q, B = int(rep.parsed.reads), int(rep.parsed.bases)
        codes, index = np.zeros(B, np.uint8), np.zeros(Q + 1, np.uint64)
        qual = np.zeros(B, np.uint8) if want_qual and rep.parsed.has_qual else None
        noff, nlen = (np.zeros(Q, np.uint64), np.zeros(Q, np.uint32)) if want_names else (None, None)
        rc = call(codes, qual, B, index, noff, nlen, Q)
    _refuse_bad_part(rc, rep, "kiss_hip_reads_parse_part_host", first_read)
    names = None
    if want_names:
        names = _numbered_names(raw, noff, nlen, int(first_read)) if noff is not None else []
    return {"reads": codes, "read_index": index, "qual": qual, "names": names, "report": _part_report(rep)}


def parse_reads_part_dev(d_chunk, format="auto", final=True, max_records=0, want_qual=True, want_names=True, ctx=None, first_read=0):
    """The same on the device: d_chunk is a contiguous uint8 torch tensor (at any address: a slice that starts where the last
    call's bytes_used ended is fine), the work runs on the current torch stream with the scratch of `ctx` (a Context,
    required).  Returns the tensors of parse_reads_dev (name_off / name_len: spans inside d_chunk) and the report of
    parse_reads_part."""
    import torch
    if ctx is None:
        raise ValueError("parse_reads_part_dev needs a Context")
    fmt, max_records = _part_arguments(format, max_records)
    if d_chunk.dtype != torch.uint8 or d_chunk.dim() != 1 or not d_chunk.is_contiguous():
        raise ValueError("d_chunk is a contiguous one-dimensional uint8 tensor")
    lib, dev, vp = ctx._lib, d_chunk.device, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    rep = _lib.ReadsPartReport()
    ptr = lambda t: vp(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731

    def call(codes, qual, bases_cap, index, noff, nlen, reads_cap):
        return lib.kiss_hip_reads_parse_part_dev(ctx._ctx, ptr(d_chunk), d_chunk.numel(), fmt, 1 if final else 0, max_records, ptr(codes),
                                                 ptr(qual), bases_cap, vp(index.data_ptr()), ptr(noff), ptr(nlen), reads_cap,
                                                 ctypes.byref(rep), stream)

    index = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = call(None, None, 0, index, None, None, 0)  # size ...
    codes, qual, noff, nlen = torch.zeros(0, dtype=torch.uint8, device=dev), None, None, None
    if want_names:
        noff, nlen = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    if rc == _lib.KISS_HIP_E_INVALID and not rep.parsed.bad_records and (rep.parsed.reads or rep.parsed.bases):  # ... then fill
        Q, B = int(rep.parsed.reads), int(rep.parsed.bases)
        codes, index = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        qual = torch.zeros(B, dtype=torch.uint8, device=dev) if want_qual and rep.parsed.has_qual else None
        if want_names:  # (one entry more than there are reads: a pointer that is not NULL when Q is 0)
            noff, nlen = torch.zeros(Q + 1, dtype=torch.int64, device=dev), torch.zeros(Q + 1, dtype=torch.int32, device=dev)
        rc = call(codes, qual, B, index, noff, nlen, Q)
        if want_names:
            noff, nlen = noff[:Q], nlen[:Q]
    _refuse_bad_part(rc, rep, "kiss_hip_reads_parse_part_dev", first_read)
    return {"reads": codes, "read_index": index, "qual": qual, "name_off": noff, "name_len": nlen, "report": _part_report(rep)}


def _strip_mate_suffix(name):
    """FASTQ mates: a name that ends in /1 or /2 loses those two bytes, as on the command line"""
    return name[:-2] if len(name) >= 2 and name[-2] == "/" and name[-1] in "12" else name


class _Feed:
    """One read file fed to the part call: the bytes read and not yet consumed, on the host (the names are cut from them) and on
    the device.  `final` is known before a chunk is cut: the file's size is."""

    def __init__(self, path, dev):
        import torch
        self.path = os.fspath(path)
        self.f = open(self.path, "rb")
        self.size = os.fstat(self.f.fileno()).st_size
        self.read_to, self.first, self.fmt, self.done = 0, 0, None, False
        self.host = b""
        self.d = torch.zeros(0, dtype=torch.uint8, device=dev)

    def fill(self, want):
        """at least `want` unconsumed bytes, or all that are left"""
        import torch
        if len(self.host) < want and self.read_to < self.size:
            more = self.f.read(want - len(self.host))
            self.read_to += len(more)
            if not more:  # (the file shrank)
                self.size = self.read_to
            else:
                self.host += more
                self.d = torch.cat([self.d, torch.from_numpy(np.frombuffer(more, np.uint8).copy()).to(self.d.device)])
        return self.read_to >= self.size

    def consume(self, used, records):
        self.host = self.host[used:]
        self.d = self.d[used:]  # (the part call takes any address)
        self.first += records

    def close(self):
        self.f.close()


def read_batches(path1, path2=None, batch_reads=100000, chunk_bytes=64 << 20, format="auto", want_qual=True, want_names=True, ctx=None,
                 device=0, hooks=None, on_device=False):
    """A generator over the parsed batches of a read file of any size: batch_reads records each (the last one what is left), cut
    at record boundaries on the device (parse_reads_part_dev), the file read chunk_bytes at a time with the unused tail carried in
    front of the next chunk; while a chunk holds fewer than batch_reads whole records and the file goes on, it is doubled.  The
    batches, concatenated, are parse_reads() of the file.
    path2: the file of the mates; each batch is then batch_reads PAIRS, interleaved on the device as map_pairs expects them
    (reads 2 p and 2 p + 1), FASTQ names stripped of /1 and /2; ValueError when one file runs out first.
    Yields dict(reads, read_index, qual, names, first_read (the number of the batch's first record, or pair, in the file),
    records, format): host arrays, or with on_device the tensors (reads, read_index, qual).  Names the file does not give are
    the file-wide record numbers.  ctx: a Context for the parse (max_n at least four times the longest chunk), or a function
    of a chunk's bytes that returns one (map_file() lends the index's own, which the stages may regrow between two
    batches); None: one is made and regrown as needed."""
    import torch
    from .sorter import Context
    _format(format)
    fmt = format
    batch_reads, chunk_bytes = int(batch_reads), int(chunk_bytes)
    if batch_reads < 1 or chunk_bytes < 1:
        raise ValueError("batch_reads and chunk_bytes are at least 1")
    dev = torch.device("cuda", ctx.device if isinstance(ctx, Context) else int(device))
    own = [None]

    def context(nbytes):
        if ctx is not None:
            return ctx(nbytes) if callable(ctx) else ctx
        need = max(4 * (nbytes + 2), 1 << 20)
        if own[0] is None or own[0].max_n < need:
            if own[0] is not None:
                own[0].close()
            own[0] = Context(max_n=need + need // 2, device=int(device), hooks=hooks)
        return own[0]

    def part(feed, final, max_records):
        out = parse_reads_part_dev(feed.d, feed.fmt or fmt, final, max_records, want_qual, want_names, context(feed.d.numel()), feed.first)
        feed.fmt = out["report"]["format"]  # (resolved on the first chunk)
        return out

    def names_of_part(feed, out, strip):
        if not want_names:
            return None
        names = _numbered_names(feed.host, out["name_off"].cpu().numpy().view(np.uint64), out["name_len"].cpu().numpy().view(np.uint32), feed.first)
        return [_strip_mate_suffix(n) for n in names] if strip else names

    def batch(out, names, first, records):
        res = {"reads": out["reads"], "read_index": out["read_index"], "qual": out["qual"]}
        if not on_device:
            res = {"reads": out["reads"].cpu().numpy(), "read_index": out["read_index"].cpu().numpy().view(np.uint64),
                   "qual": out["qual"].cpu().numpy() if out["qual"] is not None else None}
        res.update(names=names, first_read=first, records=records, format=feeds[0].fmt)
        return res

    feeds = [_Feed(p, dev) for p in ([path1] if path2 is None else [path1, path2])]
    want = [chunk_bytes] * len(feeds)
    try:
        while not all(f.done for f in feeds):
            # size: the whole records either file has ready, up to batch_reads
            outs, finals = [], []
            for i, f in enumerate(feeds):
                while True:
                    final = f.fill(want[i])
                    out = part(f, final, batch_reads)
                    if final or out["report"]["records"] == batch_reads:
                        break
                    want[i] = 2 * max(want[i], len(f.host))  # fewer than batch_reads whole records: a longer chunk
                outs.append(out)
                finals.append(final)
            K = min(o["report"]["records"] for o in outs)
            if len(feeds) == 2:
                for f, o, final in zip(feeds, outs, finals):
                    if K == 0 and final and o["report"]["records_complete"] == 0 and max(x["report"]["records"] for x in outs):
                        raise ValueError("%s runs out after %d reads (all of them), before its mate file: a pair has one of each"
                                         % (f.path, f.first))
                if feeds[0].fmt != feeds[1].fmt:
                    raise ValueError("%s and %s differ in format (one is FASTQ, one has a read per line): name it with format="
                                     % (feeds[0].path, feeds[1].path))
                # fill: K records of both
                outs = [o if o["report"]["records"] == K else part(f, final, K) for f, o, final in zip(feeds, outs, finals)]
            first = feeds[0].first
            names = [names_of_part(f, o, len(feeds) == 2 and f.fmt == "fastq") for f, o in zip(feeds, outs)]
            for i, (f, o, final) in enumerate(zip(feeds, outs, finals)):
                rep = o["report"]
                f.consume(rep["bytes_used"], rep["records"])
                f.done = final and rep["records"] == rep["records_complete"]
                want[i] = chunk_bytes
            if K == 0:
                continue  # (blank lines at the end of the file)
            if len(feeds) == 1:
                yield batch(outs[0], names[0], first, K)
            else:
                both = interleave_reads_dev(outs[0], outs[1], context(0))
                yield batch(both, [n for pair in zip(*names) for n in pair] if want_names else None, first, K)
    finally:
        for f in feeds:
            f.close()
        if own[0] is not None:
            own[0].close()


def map_file(index, reads1, text, reads2=None, batch_reads=100000, chunk_bytes=64 << 20, format="auto", **params):
    """A generator over the batches of a read file mapped by `index`, an FMIndex: reads1 is the path of a FASTQ file or of one
    with a read per line, cut into batches of batch_reads records on the device (read_batches, which has chunk_bytes and
    format); every batch goes through index.map(), or with reads2 -- the path of the mates' file; batch_reads then counts
    pairs -- through what index.map_pairs() runs, with `params`, the arguments of either.  The index and the text stay on
    the device across the batches.
    Yields what map() / map_pairs() returns for the batch (read, hit and pair numbers count inside the batch) plus names
    (one per read, file-wide numbers where the file gives none), qual (the quality bytes at the offsets of the reads, or
    None) and first_read (the number of the batch's first read, or pair, in the file).  Apart from the insert size, every
    stage treats a read or a pair on its own: the mappings do not depend on how the file was cut.
    insert="auto" (or True, or a dict) with reads2: the insert size is estimated ONCE, from batch 0.  The three values it
    used -- the estimate, or the caller's or default values when batch 0 had too few samples -- serve every later batch,
    whose result carries insert = dict(applied, ins_min, ins_max, ins_mean, from_batch=0), without report and histogram.
    sam=True (with ref_names where bounds is given): every batch also carries its alignment lines (sam, sam_line_index,
    sam_read_line, sam_report, as map(sam=True) gives them), with the names and the qualities of the parsed chunk -- FASTQ mate
    names without their /1 and /2 --; the lines of the batches, one after the other, are the lines of the file.
    bam=True (with ref_names and bounds; it may stand beside sam=True): every batch also carries bam, the BGZF blocks of its BAM
    records (bam_rec_index, bam_read_rec, bam_report, as map(bam=True) gives them); the blocks of the batches, one after the other
    behind the framed header and in front of the end-of-file block, are the file (kiss_amd.bam_writer.write_bam does that).
    bam_compress=True (with bam=True): the blocks are compressed on the device, as map(bam_compress=True) does it.
    bam_sort=True is a ValueError: batches sorted one by one do not concatenate into a sorted file.  A sorted file is written by
    kiss_amd.bam_writer.write_bam(sort=True), which keeps the records of every batch on the device and sorts them once.
    bam_markdup=True is a ValueError for the same reason: duplicates are a property of the file, and
    kiss_amd.bam_writer.write_bam(sort=True, markdup=True) marks them once, on all its records.
    pileup=True (or a dict, or an (8, W) int32 device tensor to add to, as map(pileup=...) takes them): ONE tensor of counts,
    allocated once, to which every batch adds (kiss_hip_fmi_pileup_dev with accumulate): its size depends on the text and not on
    the file.  Every batch's result carries that tensor as pileup -- the sums up to and including the batch -- and
    pileup_report, the sums of the report's fields so far; behind the last batch they are those of the file."""
    if "names" in params or "qual" in params:
        raise ValueError("map_file takes names and qualities from the file")
    sam, bam, ref_names = bool(params.pop("sam", False)), bool(params.pop("bam", False)), params.pop("ref_names", None)
    if params.pop("bam_sort", False):
        raise ValueError("map_file(bam_sort=True): batches sorted one by one are not a sorted file; kiss_amd.bam_writer.write_bam(sort=True) "
                         "sorts the whole file")
    if params.pop("bam_markdup", False):
        raise ValueError("map_file(bam_markdup=True): duplicates marked batch by batch are not the duplicates of the file; "
                         "kiss_amd.bam_writer.write_bam(sort=True, markdup=True) marks the whole file")
    packed = {"bam_compress": True} if params.pop("bam_compress", False) else {}
    if packed and not bam:
        raise ValueError("bam_compress belongs to bam=True")
    if params.pop("_bam_unframed", False):  # (write_bam(sort=True): the records of every batch stay on the device, unframed)
        packed["_bam_unframed"] = True
    lines = lambda b: dict(sam=sam, bam=bam, names=b["names"], qual=b["qual"], ref_names=ref_names, **packed) if sam or bam else {}  # noqa: E731
    po = index._pileup_options({"pileup": params.pop("pileup", None)}, params.get("want_cigar", True))
    from .fm_pair import pair_params as make_pair_params
    from .fm_select import select_params as make_select_params
    d_text, n = index._text_dev(text)
    d_text = d_text[:n]
    paired = reads2 is not None
    if paired:
        keys = ("min_len", "max_len", "max_occ", "chain_params", "align_params", "select_params", "bounds", "want_cigar", "rescue",
                "want_md", "insert")
        p = {k: params.pop(k) for k in keys if k in params}
        index._md_needs_ops(p.get("want_md", False), p.get("want_cigar", True))
        sp = make_select_params(**(p.get("select_params") or {}))
        insert, pair_kw, ip = p.get("insert"), dict(params), None
        if insert is not None and insert is not False:
            from .fm_insert import insert_params as make_insert_params
            ip = make_insert_params(**({} if insert is True or insert == "auto" else dict(insert)))
        make_pair_params(**pair_kw)  # (a wrong argument is said before a file is opened)
    if po:
        import torch
        from .fm_pileup import add_reports, window
        lo, hi = window(n, po["lo"] or 0, po["hi"])
        dev = torch.device("cuda", index.device)
        if po["counts"] is None:
            po["counts"] = torch.zeros((8, hi - lo), dtype=torch.int32, device=dev)
        elif not isinstance(po["counts"], torch.Tensor):
            host = np.ascontiguousarray(po["counts"], dtype=np.uint32)
            po["counts"] = torch.from_numpy(host.view(np.int32)).to(dev)
        pileup_sums = {}
    carried = None
    lend = lambda nbytes: index._context(min(_lib.MAX_N, max(index.N, 4 * (nbytes + 2))))  # noqa: E731 (no second set of work arrays)
    for number, b in enumerate(read_batches(reads1, reads2, batch_reads, chunk_bytes, format, ctx=lend, device=index.device,
                                            hooks=index._hooks)):
        reads = (b["reads"], b["read_index"])
        if not paired:
            res = index.map(reads, d_text, **params, **lines(b),
                            **(dict(pileup=dict(po["params"], lo=po["lo"], hi=po["hi"], counts=po["counts"])) if po else {}))
        else:
            if carried is not None:
                pair_kw.update(ins_min=carried["ins_min"], ins_max=carried["ins_max"], ins_mean=carried["ins_mean"])
            res = index._map_pair_batch(reads, d_text, p.get("min_len", 19), p.get("max_len", 0), p.get("max_occ", 500),
                                        p.get("chain_params"), p.get("align_params"), sp, p.get("bounds"), p.get("want_cigar", True),
                                        p.get("rescue"), p.get("want_md", False), ip if carried is None else None,
                                        make_pair_params(**pair_kw),
                                        index._sam_options(lines(b),
                                                           p.get("want_cigar", True), p.get("bounds")), po)
            if ip is not None:
                if carried is None:
                    res["insert"]["from_batch"] = number
                    carried = {k: res["insert"][k] for k in ("applied", "ins_min", "ins_max", "ins_mean", "from_batch")}
                else:
                    res["insert"] = dict(carried)
        if po:
            res["pileup_report"] = dict(add_reports(pileup_sums, res["pileup_report"]))
        res.update(names=b["names"], qual=b["qual"], first_read=b["first_read"])
        yield res
