"""The definition of include/kiss_hip_reads.h restated as loops over lines: parse(raw, fmt) and interleave(a, b).

Both formats are line based.  A line is a maximal run of bytes between '\\n's; a last piece without '\\n' is a line if it is not
empty, an empty piece behind the last '\\n' is none; one trailing '\\r' is taken off a line.  Codes: A/a 0, C/c 1, G/g 2, T/t 3,
every other byte 4.

parse() returns a dict with every output array and every report field the definition gives:
  format ("lines" / "fastq": the one parsed), lines, reads, bases, no_base, empty_reads, first_empty (None: none), has_qual,
  bad_records, first_bad (None: none), first_bad_kind (0: none),
  codes (uint8), qual (uint8 or None), read_index (uint64, reads + 1), name_off (uint64) / name_len (uint32): the span of a
  read's name inside raw (name_off means something only where name_len > 0), names (the spans as str, the decimal read number
  where a span is empty).
With bad records only format, lines and the three bad_* fields are defined; the others are None.
"""
import numpy as np

CODES = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}
BAD_NO_AT, BAD_NO_PLUS, BAD_LENGTHS, BAD_TRUNCATED = 1, 2, 3, 4


def split_lines(raw):
    """[(beg, end)]: the lines of raw after the '\\r' strip, as spans"""
    raw = bytes(raw)
    spans, beg = [], 0
    while beg < len(raw):
        nl = raw.find(b"\n", beg)
        end = len(raw) if nl < 0 else nl
        stop = end - 1 if end > beg and raw[end - 1] == 0x0D else end
        spans.append((beg, stop))
        beg = end + 1
    return spans


def name_span(raw, beg, end):
    """the name of a header line [beg, end): behind its first byte up to the first space, tab or line end"""
    j = beg + 1
    while j < end and raw[j] not in (0x20, 0x09):
        j += 1
    return beg + 1, j - (beg + 1)


def _finish(raw, out, seqs, quals, spans):
    codes = [CODES.get(c, 4) for beg, end in seqs for c in raw[beg:end]]
    index = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([end - beg for beg, end in seqs], out=index[1:])
    out.update(reads=len(seqs), bases=len(codes), no_base=sum(1 for c in codes if c == 4), codes=np.array(codes, np.uint8), read_index=index,
               qual=None if quals is None else np.frombuffer(b"".join(raw[beg:end] for beg, end in quals), np.uint8).copy(),
               name_off=np.array([s[0] for s in spans], np.uint64), name_len=np.array([s[1] for s in spans], np.uint32),
               names=[raw[o:o + n].decode("latin-1") if n else str(q) for q, (o, n) in enumerate(spans)])
    return out


def parse(raw, fmt="auto"):
    raw = bytes(raw)
    assert fmt in ("auto", "lines", "fastq")
    if fmt == "auto":
        fmt = "fastq" if raw[:1] == b"@" else "lines"
    lines = split_lines(raw)
    out = dict(format=fmt, lines=len(lines), has_qual=int(fmt == "fastq"), empty_reads=0, first_empty=None, bad_records=0, first_bad=None,
               first_bad_kind=0)
    if fmt == "lines":
        seqs, spans = [], []
        for k, (beg, end) in enumerate(lines):
            if end == beg or raw[beg] == 0x3E:
                continue
            span = (0, 0)
            if k > 0:
                pb, pe = lines[k - 1]
                if pe > pb and raw[pb] == 0x3E:
                    span = name_span(raw, pb, pe)
            seqs.append((beg, end))
            spans.append(span)
        return _finish(raw, out, seqs, None, spans)
    kept = len(lines)
    while kept and lines[kept - 1][0] == lines[kept - 1][1]:
        kept -= 1
    seqs, quals, spans = [], [], []
    for r in range(-(-kept // 4)):
        rec = lines[4 * r:min(4 * r + 4, kept)]
        kind = 0
        if len(rec) < 4:
            kind = BAD_TRUNCATED
        elif rec[0][0] == rec[0][1] or raw[rec[0][0]] != 0x40:
            kind = BAD_NO_AT
        elif rec[2][0] == rec[2][1] or raw[rec[2][0]] != 0x2B:
            kind = BAD_NO_PLUS
        elif rec[1][1] - rec[1][0] != rec[3][1] - rec[3][0]:
            kind = BAD_LENGTHS
        if kind:
            out["bad_records"] += 1
            if out["first_bad"] is None:
                out["first_bad"], out["first_bad_kind"] = r, kind
            continue
        if rec[1][0] == rec[1][1]:
            out["empty_reads"] += 1
            if out["first_empty"] is None:
                out["first_empty"] = r
        seqs.append(rec[1])
        quals.append(rec[3])
        spans.append(name_span(raw, *rec[0]))
    if out["bad_records"]:
        out.update(reads=None, bases=None, no_base=None, empty_reads=None, first_empty=None, codes=None, qual=None, read_index=None,
                   name_off=None, name_len=None, names=None)
        return out
    return _finish(raw, out, seqs, quals, spans)


def interleave(a, b):
    """a, b: (codes, read_index, qual or None) of P reads each -> (codes, read_index, qual or None) of 2 P reads; None where
    the call refuses: different read counts, an index that decreases or does not start at 0, qualities of one batch only"""
    (ca, ia, qa), (cb, ib, qb) = a, b
    ia, ib = [int(x) for x in ia], [int(x) for x in ib]
    if len(ia) != len(ib) or (qa is None) != (qb is None) or ia[0] != 0 or ib[0] != 0:
        return None
    if any(y < x for idx in (ia, ib) for x, y in zip(idx, idx[1:])):
        return None
    codes, qual, index = [], [], [0]
    for p in range(len(ia) - 1):
        for c, idx, q in ((ca, ia, qa), (cb, ib, qb)):
            codes.extend(c[idx[p]:idx[p + 1]])
            if q is not None:
                qual.extend(q[idx[p]:idx[p + 1]])
            index.append(len(codes))
    return np.array(codes, np.uint8), np.array(index, np.uint64), None if qa is None else np.array(qual, np.uint8)
