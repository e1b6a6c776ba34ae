"""The definition of include/kiss_hip_reads_part.h restated over the lines of tests/reads_model.py: parse_part(raw, fmt, final,
max_records) parses the first whole records of a chunk of a read file and says how many bytes they took; batches() feeds a file
through it the way a caller does (the unused tail carried in front of the next chunk, `final` on the last one).

COMPLETE LINES.  final: the lines of the parse definition.  Not final: only lines ended by a '\\n' inside the chunk.
FASTQ.  kept = the complete lines up to the last one that is not empty after the strip (final or not: lines that are empty so far
are never consumed early).  records_complete = ceil(kept / 4) with final (a truncated last record counts, so that the parse
refuses it as kind 4), floor(kept / 4) without.  records = records_complete, or min(max_records, records_complete) when
max_records > 0.  final and records == records_complete: bytes_used = bytes and the prefix is parsed as parse() parses a file.
Otherwise bytes_used is the offset behind the '\\n' of line 4 records - 1 (0 when records is 0) and the prefix is parsed with
roles by line number and NO LINE DROPPED: an empty quality line that ends the prefix belongs to an empty read.
LINES.  A record is a read line.  bytes_used is the offset behind the '\\n' of read line number `records` (0 when records is 0);
final and records == records_complete: bytes_used = bytes.
AUTO looks at the first byte of the chunk.

parse_part() returns the dict of reads_model.parse for the prefix (first_bad relative to the chunk, name spans inside the chunk,
default names numbered inside the chunk) plus records_complete, records, bytes_used.
"""
from tests import reads_model as rm


def complete_lines(raw, final):
    """the spans of the complete lines of a chunk"""
    raw = bytes(raw)
    return rm.split_lines(raw if final else raw[:raw.rfind(b"\n") + 1])


def parse_part(raw, fmt="auto", final=True, max_records=0):
    raw = bytes(raw)
    assert fmt in ("auto", "lines", "fastq")
    if fmt == "auto":
        fmt = "fastq" if raw[:1] == b"@" else "lines"
    lines = complete_lines(raw, final)
    if fmt == "fastq":
        kept = len(lines)
        while kept and lines[kept - 1][0] == lines[kept - 1][1]:
            kept -= 1
        complete = -(-kept // 4) if final else kept // 4
        last_line = lambda records: 4 * records - 1  # noqa: E731
    else:
        read_lines = [k for k, (beg, end) in enumerate(lines) if end > beg and raw[beg] != 0x3E]
        complete = len(read_lines)
        last_line = lambda records: read_lines[records - 1]  # noqa: E731
    records = min(max_records, complete) if max_records > 0 else complete
    if final and records == complete:
        used = len(raw)
        out = rm.parse(raw, fmt)
    else:
        used = 0
        if records:
            used = raw.index(b"\n", lines[last_line(records)][0]) + 1
        # a sentinel record keeps the parse from dropping the empty lines that end the prefix; it is taken off again
        out = rm.parse(raw[:used] + b"@\nA\n+\nI\n", fmt) if fmt == "fastq" else rm.parse(raw[:used], fmt)
        if fmt == "fastq":
            out["lines"] -= 4
            if not out["bad_records"]:
                assert out["reads"] == records + 1
                out.update(reads=records, bases=out["bases"] - 1, codes=out["codes"][:-1], qual=out["qual"][:-1],
                           read_index=out["read_index"][:-1], name_off=out["name_off"][:-1], name_len=out["name_len"][:-1],
                           names=out["names"][:-1])
    out.update(records_complete=complete, records=records, bytes_used=used)
    return out


def batches(raw, chunk, max_records=0, fmt="auto", grow=lambda c: 2 * c):
    """The file fed chunk by chunk: [the dict of parse_part, plus first_read: the records consumed before].  The caller's loop:
    `chunk` bytes more behind the tail of the last call, `final` once the file's end is inside; a call that answers 0 records
    without `final` gets a longer chunk.  The format is resolved on the first chunk.  Stops behind the first batch with bad
    records."""
    raw = bytes(raw)
    out, pos, first, size = [], 0, 0, chunk
    while True:
        end = min(len(raw), pos + size)
        final = end == len(raw)
        got = parse_part(raw[pos:end], fmt, final, max_records)
        fmt = got["format"]
        if not final and got["records"] == 0:
            assert got["bytes_used"] == 0
            size = grow(size)
            continue
        got["first_read"] = first
        out.append(got)
        if got["bad_records"]:
            return out
        pos += got["bytes_used"]
        first += got["records"]
        size = chunk
        if final and got["records"] == got["records_complete"]:
            assert pos == len(raw)
            return out
