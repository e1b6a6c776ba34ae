"""The chunk reader of `kiss fmindex_query --batch-reads` without a device: kiss_amd/csrc/host/cli_batches.hpp compiled alone
(no libkiss_hip) into tests/cli_batches_check.cpp, which puts a plain host cut in the place of the part call, with
AddressSanitizer and UBSan.  The batches it prints are held against tests/reads_part_model.py and tests/reads_model.py: every
batch but the last has batch_reads records, they start at 0, batch_reads, 2 batch_reads ..., and concatenated they are the parse
of the whole file with file-wide default names, for chunk sizes 1, 7, 4096 and the file's size - 1, + 0, + 1.  A bad record, or a
read without bases, stops the reader in the batch it lies in, under its number in the file, behind the batches before it."""
import subprocess

import numpy as np
import pytest

from tests import reads_model as rm
from tests import reads_part_model as pm
from tests.test_cli_format import program
from tests.test_reads_part_model import random_fastq, random_lines


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return program(tmp_path_factory.mktemp("cli_batches"), "cli_batches_check")


def expected(raw, fmt, n):
    """(the reads of the batches that are printed: [(name, codes, qual)], what the error names or None)"""
    whole = rm.parse(raw, fmt)
    error = None
    if whole["bad_records"]:
        bad = whole["first_bad"]
        error = (bad // n, "record %d:" % bad)
        whole = pm.parse_part(raw, fmt, True, bad) if bad else None  # the records in front of it
    if whole is not None and whole["empty_reads"]:
        e = whole["first_empty"]
        if error is None or e // n < error[0]:
            error = (e // n, "read %d of" % e)
    Q = (whole["reads"] if whole is not None else 0) if error is None else error[0] * n
    reads = []
    for q in range(Q):
        beg, end = int(whole["read_index"][q]), int(whole["read_index"][q + 1])
        qual = "-" if whole["qual"] is None else "".join("%x." % c for c in whole["qual"][beg:end])
        reads.append((whole["names"][q], "".join(str(c) for c in whole["codes"][beg:end]), qual))
    return reads, error


def run_and_check(exe, path, raw, fmt, chunk, n):
    path.write_bytes(raw)
    r = subprocess.run([exe, str(path), fmt, str(chunk), str(n)], capture_output=True, text=True)
    reads, error = expected(raw, fmt, n)
    if error is None:
        assert r.returncode == 0 and r.stderr == "", (raw, fmt, chunk, n, r.stderr)
    else:
        assert r.returncode == 3 and error[1] in r.stderr, (raw, fmt, chunk, n, r.stderr)
    got, firsts, sizes = [], [], []
    for ln in r.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "batch" and len(f) == 4:
            firsts.append(int(f[1]))
            sizes.append(int(f[2]))
            assert f[3] == rm.parse(raw, fmt)["format"]
        else:
            got.append(tuple(f))
    assert got == reads, (raw, fmt, chunk, n)
    assert firsts == list(range(0, len(reads), n)), (raw, fmt, chunk, n, firsts)
    assert sizes == [min(n, len(reads) - a) for a in firsts]
    return len(firsts), error


@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_batches_of_random_files_at_every_chunk_size(exe, tmp_path, fmt):
    rng = np.random.default_rng(30 if fmt == "fastq" else 31)
    most, errors = 0, 0
    for i in range(30):
        raw = (random_fastq if fmt == "fastq" else random_lines)(rng)
        n = int(rng.choice([1, 3, 7, 1000]))
        for chunk in (1, 7, 4096, max(1, len(raw) - 1), max(1, len(raw)), len(raw) + 1):
            batches, error = run_and_check(exe, tmp_path / "reads", raw, fmt, chunk, n)
            most, errors = max(most, batches), errors + (error is not None)
    assert most > 3 and (errors > 0) == (fmt == "fastq")


def test_hand_cases(exe, tmp_path):
    p = tmp_path / "reads"
    fq = b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, b"ACGT"[:1 + i % 4], b"@+I>"[:1 + i % 4]) for i in range(9))
    for chunk in (1, 7, 4096, len(fq) - 1, len(fq), len(fq) + 1):
        for n in (1, 4, 9, 10):
            assert run_and_check(exe, p, fq, "auto", chunk, n) == (-(-9 // n), None)  # ('@' and '+' start quality lines)
        assert run_and_check(exe, p, fq + b"\n\r\n\n\n\n", "fastq", chunk, 3) == (3, None)  # five blank lines at the end are no record
        assert run_and_check(exe, p, fq[:-2], "fastq", chunk, 3)[1] == (2, "record 8:")  # no quality line, in the third batch
        assert run_and_check(exe, p, fq[:-4], "fastq", chunk, 3)[1] == (2, "record 8:")  # the file ends inside the record
        assert run_and_check(exe, p, fq.replace(b"@r4 x\nA\n+\n@\n", b"@r4 x\n\n+\n\n"), "fastq", chunk, 2)[1] == (2, "read 4 of")
        # lines: names from '>' lines, default names file-wide, a '>' line and blank lines last, no newline at the end
        ln = b">a\nACGT\n\nGG\r\n>b c\n>d\nT\nNNA\n>e\n\n"
        for tail in (b"", b"CC", b"CC\n>f"):
            for n in (1, 2, 5, 6):
                run_and_check(exe, p, ln + tail, "lines", chunk, n)
    assert [x[0] for x in expected(ln, "lines", 1)[0]] == ["a", "1", "d", "3"]
    long = b"@l\n" + b"ACGT" * 3000 + b"\n+\n" + b"I" * 12000 + b"\n@s\nA\n+\nI\n"  # a record longer than many chunks
    assert run_and_check(exe, p, long, "auto", 64, 1) == (2, None)
    assert run_and_check(exe, p, b"", "auto", 64, 1) == (0, None)
    assert run_and_check(exe, p, b"\n\n\n", "auto", 2, 1) == (0, None)
    assert subprocess.run([exe, str(tmp_path / "missing"), "auto", "64", "1"], capture_output=True).returncode == 3
