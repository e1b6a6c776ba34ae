"""The definition of the part call without a device (tests/reads_part_model.py; include/kiss_hip_reads_part.h) held against
tests/reads_model.py: the batches of a file, concatenated, are the parse of the whole file, however the file is cut.  Then hand
cases at the cut, the ABI of the new header and the arguments the Python wrappers refuse."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reads_model as rm
from tests import reads_part_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_fastq(rng):
    """a FASTQ file with CRLF, blank lines inside and at the end, empty reads, every bad kind, a cut in mid-record"""
    eol = b"\r\n" if rng.integers(4) == 0 else b"\n"
    lines = []
    for r in range(int(rng.integers(0, 30))):
        L = int(rng.integers(0, 3)) if rng.integers(4) == 0 else int(rng.integers(1, 40))
        seq = bytes(rng.choice(list(b"ACGTNacgt"), L).tolist())
        qual = bytes(rng.choice(list(b"@+I#5>"), L).tolist())
        lines += [b"@" + [b"r%d" % r, b"", b"r%d w" % r][r % 3], seq, b"+" + [b"", b"x"][r % 2], qual]
    if lines and rng.integers(3) == 0:  # one bad record, of any kind
        r, kind = int(rng.integers(len(lines) // 4)), int(rng.integers(1, 5))
        if kind == rm.BAD_NO_AT:
            lines[4 * r] = [b"", b"r"][int(rng.integers(2))]
        elif kind == rm.BAD_NO_PLUS:
            lines[4 * r + 2] = [b"", b"-"][int(rng.integers(2))]
        elif kind == rm.BAD_LENGTHS:
            lines[4 * r + 3] += b"I"
        else:
            lines.insert(4 * r + int(rng.integers(1, 4)), b"")  # a blank line inside shifts every role behind it
    if lines and rng.integers(5) == 0:
        lines = lines[:len(lines) - int(rng.integers(1, 4))]  # the file ends inside a record
    raw = b"".join(ln + eol for ln in lines)
    if raw and rng.integers(4) == 0:
        raw = raw[:-len(eol)]  # no last line end
        if rng.integers(2):
            return raw
    return raw + eol * int(rng.integers(0, 10))


def random_lines(rng):
    eol = b"\r\n" if rng.integers(4) == 0 else b"\n"
    lines = []
    for r in range(int(rng.integers(0, 40))):
        k = int(rng.integers(8))
        if k == 0:
            lines.append(b"")
        elif k <= 2:
            lines.append(b">" + [b"n%d" % r, b"", b"n%d more" % r][r % 3])
        else:
            lines.append(bytes(rng.choice(list(b"ACGTNacgt@+"), int(rng.integers(1, 40))).tolist()))
    raw = b"".join(ln + eol for ln in lines)
    if raw and rng.integers(4) == 0:
        return raw[:-len(eol)]
    return raw + eol * int(rng.integers(0, 10))


def check_property(raw, fmt, chunk, max_records):
    """the batches of raw, concatenated, against the parse of raw"""
    whole = rm.parse(raw, fmt)
    got = pm.batches(raw, chunk, max_records, fmt)
    where = (raw, fmt, chunk, max_records)
    for b in got[:-1]:
        assert not b["bad_records"], where
    last = got[-1]
    if whole["bad_records"]:
        assert last["bad_records"], where
        assert (last["first_bad"] + last["first_read"], last["first_bad_kind"]) == (whole["first_bad"], whole["first_bad_kind"]), where
        return 0
    assert not last["bad_records"], where
    assert sum(b["reads"] for b in got) == whole["reads"] and sum(b["empty_reads"] for b in got) == whole["empty_reads"], where
    assert all(b["records"] == b["reads"] and b["format"] == whole["format"] for b in got), where
    assert all(b["records"] <= max_records for b in got if max_records), where
    assert np.concatenate([b["codes"] for b in got]).tolist() == whole["codes"].tolist(), where
    index, pos, names = [0], 0, []
    for b in got:
        index += [int(x) + index[-1] for x in b["read_index"][1:]]
        chunk_bytes = raw[pos:]
        names += [chunk_bytes[int(o):int(o) + int(n)].decode("latin-1") if n else str(b["first_read"] + q)
                  for q, (o, n) in enumerate(zip(b["name_off"], b["name_len"]))]
        pos += b["bytes_used"]
    assert index == whole["read_index"].tolist() and names == whole["names"] and pos == len(raw), where
    if whole["qual"] is not None:
        assert np.concatenate([b["qual"] for b in got]).tolist() == whole["qual"].tolist(), where
    firsts = [b["first_read"] + b["first_empty"] for b in got if b["first_empty"] is not None]
    assert (firsts[0] if firsts else None) == whole["first_empty"], where
    return len(got)


@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_batches_are_the_parse_of_the_whole_file(fmt):
    rng = np.random.default_rng(20 if fmt == "fastq" else 21)
    bad = many = 0
    for i in range(500):
        raw = random_fastq(rng) if fmt == "fastq" else random_lines(rng)
        chunk = int(rng.integers(1, 30)) if i % 2 else int(rng.integers(1, 1001))
        max_records = int(rng.integers(0, 101)) if i % 3 else int(rng.integers(1, 4))
        n = check_property(raw, fmt, chunk, max_records)
        bad += n == 0
        many += n > 2
    assert many > 150 and (fmt == "lines" or bad > 50)


def test_auto_is_resolved_on_the_first_chunk():
    raw = b"@a\nAC\n+\n@I\n@b\nG\n+\n+\n"
    assert [b["format"] for b in pm.batches(raw, 11)] == ["fastq", "fastq"]
    assert check_property(raw, "auto", 11, 0) == 2
    assert pm.parse_part(b"", "auto", True)["format"] == "lines" and pm.parse_part(b">x\nAC\n", "auto", False)["format"] == "lines"


def part(raw, fmt, final, max_records=0):
    got = pm.parse_part(raw, fmt, final, max_records)
    return got["records_complete"], got["records"], got["bytes_used"], got["reads"]


def test_quality_lines_that_start_with_at_and_plus_at_the_cut():
    raw = b"@a\nAC\n+\n@I\n@b\nG\n+\n+\n@c\nT\n+\n@\n"
    for cut in range(len(raw)):  # a cut in front of any byte: whole records only, roles by line number
        rc, records, used, reads = part(raw[:cut], "fastq", False)
        assert rc == records == reads == (cut >= 11) + (cut >= 20) + (cut >= 29) and used == (0, 11, 20, 29)[records], cut
    assert part(raw, "fastq", False, 2) == (3, 2, 20, 2) and part(raw, "fastq", True, 2) == (3, 2, 20, 2)
    assert part(raw, "fastq", True, 3) == (3, 3, len(raw), 3) and part(raw, "fastq", True, 4) == (3, 3, len(raw), 3)
    assert pm.parse_part(raw, "fastq", False, 2)["qual"].tobytes() == b"@I+"


def test_empty_reads_and_blank_lines_at_the_cut():
    raw = b"@a\n\n+\n\n@b\nA\n+\nI\n"
    assert part(raw[:7], "fastq", False) == (0, 0, 0, 0)           # '@a', '', '+', '': the blank line is not consumed early
    assert part(raw[:9], "fastq", False) == (0, 0, 0, 0)           # (nor while the next line is not complete)
    assert part(raw[:10], "fastq", False) == (1, 1, 7, 1)          # '@b' is complete: the empty quality line belongs to read a
    got = pm.parse_part(raw, "fastq", True, 1)                     # no line dropped from a prefix that max_records cut
    assert (got["records"], got["bytes_used"], got["reads"], got["empty_reads"], got["first_empty"], got["lines"]) == (1, 7, 1, 1, 0, 4)
    got = pm.parse_part(raw[:7], "fastq", True)                    # the end of the file: the parse drops the line, kind 4
    assert (got["records_complete"], got["records"], got["bytes_used"], got["first_bad"], got["first_bad_kind"]) == (1, 1, 7, 0, rm.BAD_TRUNCATED)
    rec = b"@a\nAC\n+\nII\n"
    for blanks in (0, 1, 4, 5):
        raw = rec + b"\n" * blanks
        got = pm.parse_part(raw, "fastq", True)
        assert (got["records_complete"], got["records"], got["bytes_used"], got["reads"], got["lines"]) == (1, 1, len(raw), 1, 4 + blanks)
        assert part(raw, "fastq", False) == (1, 1, len(rec), 1)    # four or more blank lines are no record
        assert check_property(raw, "fastq", len(rec) + blanks // 2, 0) >= 1
    for final in (False, True):                                    # a chunk of blank lines only
        assert part(b"\n\r\n\n\n\n", "fastq", final) == (0, 0, 6 if final else 0, 0)
        assert part(b"\n\r\n\n\n\n", "lines", final) == (0, 0, 6 if final else 0, 0)
        for fmt in ("fastq", "lines", "auto"):                     # bytes == 0
            got = pm.parse_part(b"", fmt, final)
            assert (got["records_complete"], got["records"], got["bytes_used"], got["reads"], got["read_index"].tolist()) == (0, 0, 0, 0, [0])


def test_lines_format_at_the_cut():
    raw = b">x\nACGT\n>y\nGG\n>z\n"
    assert part(raw, "lines", False) == (2, 2, 14, 2)              # a '>' line last in the chunk stays with its read
    assert part(raw, "lines", True) == (2, 2, len(raw), 2)
    assert part(raw, "lines", True, 1) == (2, 1, 8, 1) and part(raw, "lines", False, 5) == (2, 2, 14, 2)
    assert part(raw[:13], "lines", False) == (1, 1, 8, 1) and part(raw[:13], "lines", True) == (2, 2, 13, 2)
    assert pm.parse_part(raw, "lines", False)["names"] == ["x", "y"]
    long = b">n\n" + b"ACGT" * 50 + b"\nAC\n"                     # a line longer than the chunk: 0 records, the caller reads on
    assert part(long[:64], "lines", False) == (0, 0, 0, 0) and part(long[:3], "lines", False) == (0, 0, 0, 0)
    assert check_property(long, "lines", 16, 0) == 1 and check_property(long, "lines", 16, 1) == 2
    fq = b"@n\n" + b"ACGT" * 50 + b"\n+\n" + b"IIII" * 50 + b"\n"
    assert part(fq[:100], "fastq", False) == (0, 0, 0, 0) and check_property(fq, "fastq", 7, 0) == 1


# ---- the ABI of include/kiss_hip_reads_part.h -------------------------------------------------------------------------------
def test_struct_sizes_and_exports(tmp_path):
    import kiss_amd
    from kiss_amd import _lib
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_reads_part.h"\nint main(void){printf("%zu %zu %zu %zu", '
                   'sizeof(kiss_hip_reads_part_report), offsetof(kiss_hip_reads_part_report, parsed), '
                   'offsetof(kiss_hip_reads_part_report, records_complete), offsetof(kiss_hip_reads_part_report, bytes_used));return 0;}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    size, at_parsed, at_complete, at_last = (int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split())
    assert ctypes.sizeof(_lib.ReadsPartReport) == size == ctypes.sizeof(_lib.ReadsReport) + 24
    assert _lib.ReadsPartReport.parsed.offset == at_parsed == 0  # new fields only follow the old ones
    assert _lib.ReadsPartReport.records_complete.offset == at_complete == 96 and _lib.ReadsPartReport.bytes_used.offset == at_last == size - 8
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kiss_hip_reads_part.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.READS_PART_EXPORTED_SYMBOLS) and len(syms) == 2
    for lib in (kiss_amd.load(False), kiss_amd.load(True)):
        for s in syms:
            assert hasattr(lib, s), "missing export " + s


def test_python_wrappers_refuse_bad_arguments_without_a_device(tmp_path):
    import kiss_amd
    with pytest.raises(ValueError):
        kiss_amd.batches.parse_reads_part(b"ACGT\n", format="fasta")
    with pytest.raises(ValueError):
        kiss_amd.batches.parse_reads_part(b"ACGT\n", max_records=-1)
    path = tmp_path / "r.txt"
    path.write_bytes(b"ACGT\n")
    for bad in (dict(batch_reads=0), dict(chunk_bytes=0), dict(format="fasta")):
        with pytest.raises(ValueError):
            next(kiss_amd.batches.read_batches(str(path), **bad))
