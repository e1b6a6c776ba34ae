"""The definition of the reads parser without a device (tests/reads_model.py; include/kiss_hip_reads.h).

The model in `lines` format is held against the project's own kiss_cli::read_file, compiled alone as tests/test_cli_format.py
compiles it (tests/cli_parse_check.cpp, with AddressSanitizer and UBSan): names and codes, read by read.  That ties the new
definition to what the command line did before the parser ran on the device.  The model in `fastq` format is held against
properties.  Then the ABI of the new header (struct sizes, exported symbols) and the host helpers of the FASTQ path of the command
line (tests/cli_reads_check.cpp, its own main, sanitizers on)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reads_model as rm
from tests.test_cli_format import program, sam
from tests.test_fasta_gpu import SMALL
from tests.test_lcp_model import FASTA_EDGE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = b"ACGTNacgt>@+ \t\r\n"


def random_files(count=200, seed=2024):
    rng = np.random.default_rng(seed)
    files = []
    for i in range(count):
        n = int(rng.integers(0, 60)) if i % 4 else int(rng.integers(60, 400))
        # newlines and headers often enough that every kind of neighbour occurs
        p = np.ones(len(ALPHABET))
        p[ALPHABET.index(b"\n")] = 4
        p[ALPHABET.index(b">")] = 2
        files.append(bytes(ALPHABET[j] for j in rng.choice(len(ALPHABET), n, p=p / p.sum())))
    return files


LINES_FILES = [t.encode() for t, _ in FASTA_EDGE_CASES] + list(SMALL) + random_files()


@pytest.fixture(scope="module")
def parse_check(tmp_path_factory):
    return program(tmp_path_factory.mktemp("reads_model"), "cli_parse_check")


def read_file_says(exe, path, raw):
    """kiss_cli::read_file on the bytes -> [(name bytes, codes)]"""
    with open(path, "wb") as o:
        o.write(raw)
    r = subprocess.run([exe, "reads", path], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", (raw, r.stderr)
    out = []
    for ln in r.stdout.split(b"\n")[:-1]:
        name, codes = ln.rsplit(b" ", 1)
        out.append((name, [int(c) for c in codes.decode()]))
    return out


def test_lines_format_is_read_file_bit_for_bit(parse_check, tmp_path):
    path = str(tmp_path / "reads.txt")
    reads = 0
    for raw in LINES_FILES:
        got = rm.parse(raw, "lines")
        want = read_file_says(parse_check, path, raw)
        assert got["reads"] == len(want), raw
        assert [n.encode("latin-1") for n in got["names"]] == [w[0] for w in want], raw
        for q, (_, codes) in enumerate(want):
            assert got["codes"][int(got["read_index"][q]):int(got["read_index"][q + 1])].tolist() == codes, (raw, q)
        assert got["qual"] is None and got["has_qual"] == 0 and got["bad_records"] == 0 and got["empty_reads"] == 0
        assert got["bases"] == sum(len(w[1]) for w in want) and got["no_base"] == sum(w[1].count(4) for w in want)
        reads += len(want)
    assert reads > 500 and len(LINES_FILES) >= 230


def test_lines_of_a_file():
    assert rm.split_lines(b"") == [] and rm.split_lines(b"\n") == [(0, 0)] and rm.split_lines(b"a") == [(0, 1)]
    assert rm.split_lines(b"ab\r\n\r\ncd\r") == [(0, 2), (4, 4), (6, 8)]  # (one '\r' goes, also from a last piece without '\n')
    assert rm.split_lines(b"a\r\r\nb\n\n") == [(0, 2), (4, 5), (6, 6)]     # (only one; an empty piece behind the last '\n' is no line)
    got = rm.parse(b"A\rC\r\n", "lines")
    assert got["codes"].tolist() == [0, 4, 1] and got["no_base"] == 1  # (a '\r' inside a line is no base)


def fastq_bytes(records, eol=b"\n", last_eol=True):
    out = b"".join(b"@" + n + eol + s + eol + b"+" + p + eol + q + eol for n, s, p, q in records)
    return out if last_eol or not out else out[:-len(eol)]


def random_records(rng, count, max_len=40):
    recs = []
    for r in range(count):
        L = int(rng.integers(0 if r % 7 == 3 else 1, max_len))
        seq = bytes(rng.choice(list(b"ACGTNacgtRY"), L).tolist())
        qual = bytes(rng.integers(33, 127, L).astype(np.uint8).tolist())
        name = [b"r%d" % r, b"r%d some words" % r, b"", b"r%d\ttab" % r, b" lead"][r % 5]
        recs.append((name, seq, [b"", b"again"][r % 2], qual))
    return recs


def check_round_trip(recs, raw, fmt="fastq"):
    got = rm.parse(raw, fmt)
    assert got["format"] == "fastq" and got["bad_records"] == 0 and got["first_bad"] is None and got["first_bad_kind"] == 0
    assert got["reads"] == len(recs) and got["has_qual"] == 1
    empties = [r for r, rec in enumerate(recs) if not rec[1]]
    assert got["empty_reads"] == len(empties) and got["first_empty"] == (empties[0] if empties else None)
    for r, (name, seq, _, qual) in enumerate(recs):
        lo, hi = int(got["read_index"][r]), int(got["read_index"][r + 1])
        assert got["codes"][lo:hi].tolist() == [rm.CODES.get(c, 4) for c in seq]
        assert got["qual"][lo:hi].tobytes() == qual
        word = re.split(rb"[ \t]", name)[0]
        assert got["names"][r] == (word.decode() if word else str(r))
        assert int(got["name_len"][r]) == len(word) and (not word or raw[int(got["name_off"][r]):][:len(word)] == word)
    assert got["bases"] == sum(len(rec[1]) for rec in recs) == int(got["read_index"][-1])
    return got


def test_fastq_round_trip_and_line_ends():
    rng = np.random.default_rng(7)
    for count in (0, 1, 2, 50):
        recs = random_records(rng, count)
        lines = check_round_trip(recs, fastq_bytes(recs))["lines"]
        assert lines == 4 * count
        check_round_trip(recs, fastq_bytes(recs, b"\r\n"))
        if count:
            check_round_trip(recs, fastq_bytes(recs, last_eol=False), "auto")           # no final newline
            check_round_trip(recs, fastq_bytes(recs, b"\r\n", last_eol=False))
            got = check_round_trip(recs, fastq_bytes(recs) + b"\n\n\r\n", "auto")       # trailing empty lines are dropped
            assert got["lines"] == 4 * count + 3
    # qualities that start with '@' and '+': roles come from the line number alone
    recs = [(b"a", b"ACGT", b"", b"@III"), (b"b", b"AC", b"", b"+@"), (b"c", b"G", b"", b"@"), (b"d", b"T", b"", b"+")]
    check_round_trip(recs, fastq_bytes(recs), "auto")
    # an empty read in the middle is kept: its sequence and quality lines are empty lines that are not at the end
    recs = [(b"a", b"AC", b"", b"II"), (b"e", b"", b"", b""), (b"b", b"G", b"", b"I")]
    assert check_round_trip(recs, fastq_bytes(recs))["first_empty"] == 1
    # auto: the first byte decides
    assert rm.parse(b">x\nAC\n", "auto")["format"] == "lines" and rm.parse(b"", "auto")["format"] == "lines"
    assert rm.parse(b"@x\nAC\n+\nII\n", "lines")["codes"].tolist() == [4, 4, 0, 1, 4, 4, 4]  # ('@x', 'AC', '+', 'II' as reads)


def test_fastq_bad_records():
    good = [(b"r%d" % r, b"ACGT", b"", b"IIII") for r in range(5)]
    lines = fastq_bytes(good).split(b"\n")[:-1]

    def parsed(edit):
        ls = list(lines)
        edit(ls)
        return rm.parse(b"\n".join(ls) + b"\n", "fastq")

    for r in (0, 2, 4):
        def no_at(ls):
            ls[4 * r] = b"r"

        def no_plus(ls):
            ls[4 * r + 2] = b""

        def lengths(ls):
            ls[4 * r + 3] = b"III"

        for edit, kind in ((no_at, rm.BAD_NO_AT), (no_plus, rm.BAD_NO_PLUS), (lengths, rm.BAD_LENGTHS)):
            got = parsed(edit)
            assert (got["bad_records"], got["first_bad"], got["first_bad_kind"]) == (1, r, kind)
            assert got["codes"] is None and got["reads"] is None

    def both(ls):  # the lowest kind that applies, at the smallest bad record
        ls[4 * 3] = b"x"
        ls[4 * 3 + 3] = b""
        ls[4 * 1 + 2] = b"-"
        ls[4 * 1 + 3] = b"II"

    got = parsed(both)
    assert (got["bad_records"], got["first_bad"], got["first_bad_kind"]) == (2, 1, rm.BAD_NO_PLUS)
    for cut in (1, 2, 3):  # a last record of fewer than four lines, whatever it holds
        got = rm.parse(b"\n".join(lines[:16 + cut]) + b"\n", "fastq")
        assert (got["bad_records"], got["first_bad"], got["first_bad_kind"]) == (1, 4, rm.BAD_TRUNCATED)
    # multi-line FASTQ is refused, not guessed at
    got = rm.parse(b"@a\nACGT\nACGT\n+\nIIIIIIII\n", "fastq")
    assert got["bad_records"] == 2 and (got["first_bad"], got["first_bad_kind"]) == (0, rm.BAD_NO_PLUS)


def test_interleave_model():
    a = (np.array([0, 1, 2, 3, 0], np.uint8), np.array([0, 2, 2, 5], np.uint64), np.arange(5, dtype=np.uint8))
    b = (np.array([3, 3, 1], np.uint8), np.array([0, 1, 3, 3], np.uint64), np.arange(10, 13, dtype=np.uint8))
    codes, index, qual = rm.interleave(a, b)
    assert codes.tolist() == [0, 1, 3, 3, 1, 2, 3, 0] and index.tolist() == [0, 2, 3, 3, 5, 8, 8] and qual.tolist() == [0, 1, 10, 11, 12, 2, 3, 4]
    assert rm.interleave(a[:2] + (None,), b[:2] + (None,))[2] is None
    assert rm.interleave(a, (b[0], b[1][:3], b[2])) is None and rm.interleave(a, b[:2] + (None,)) is None
    assert rm.interleave((a[0], np.array([0, 3, 2, 5], np.uint64), a[2]), b) is None


# ---- the ABI of include/kiss_hip_reads.h ------------------------------------------------------------------------------------
def test_struct_sizes_and_exports(tmp_path):
    import kiss_amd
    from kiss_amd import _lib
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kiss_hip_reads.h"\nint main(void){printf("%zu %zu %zu", '
                   'sizeof(kiss_hip_reads_report), offsetof(kiss_hip_reads_report, format), offsetof(kiss_hip_reads_report, ms_copy));'
                   'return 0;}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    size, at_format, at_last = (int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split())
    assert ctypes.sizeof(_lib.ReadsReport) == size == 96
    assert _lib.ReadsReport.format.offset == at_format == 64 and _lib.ReadsReport.ms_copy.offset == at_last == size - 4
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kiss_hip_reads.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(kiss_hip_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.READS_EXPORTED_SYMBOLS) and len(syms) == 4
    for lib in (kiss_amd.load(False), kiss_amd.load(True)):
        for s in syms:
            assert hasattr(lib, s), "missing export " + s
    assert (_lib.READS_AUTO, _lib.READS_LINES, _lib.READS_FASTQ) == tuple(
        int(re.search(r"#define KISS_HIP_READS_%s (\d+)" % k, text).group(1)) for k in ("AUTO", "LINES", "FASTQ"))


def test_python_wrappers_refuse_bad_arguments_without_a_device():
    import kiss_amd
    with pytest.raises(ValueError):
        kiss_amd.parse_reads(b"ACGT\n", format="fasta")
    a = (np.zeros(3, np.uint8), np.array([0, 3], np.uint64))
    with pytest.raises(ValueError):
        kiss_amd.interleave_reads(a, (np.zeros(0, np.uint8), np.array([0, 0, 0], np.uint64)))  # one read and two
    with pytest.raises(ValueError):
        kiss_amd.interleave_reads(a + (np.zeros(3, np.uint8),), a)  # qualities of one batch only


# ---- the host helpers of the command line -------------------------------------------------------------------------------------
def test_host_helpers_of_the_fastq_path(tmp_path):
    text = b"@first words\nACGT\n+\nIIII\n@\nAC\n+\n#!\n@pair/1\tx\nGG\n+\n;;\n"  # (the file of tests/cli_reads_check.cpp)
    spans = rm.parse(text, "fastq")
    assert list(zip(spans["name_off"].tolist(), spans["name_len"].tolist())) == [(1, 5), (26, 0), (36, 6)]
    r = subprocess.run([program(tmp_path, "cli_reads_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr

    def lines(q0, q1, q2):
        return [sam("r0", 0, "chr", 11, 60, "5M", "*", 0, 0, "ACGTA", q0, "NM:i:0", "AS:i:5", "XS:i:0"),
                sam("r1", 16, "chr", 11, 30, "5M", "*", 0, 0, "CGGTT", q1, "NM:i:0", "AS:i:5", "XS:i:0"),  # SEQ and QUAL reversed
                sam("r2", 4, "*", 0, 0, "*", "*", 0, 0, "TTN", q2)]                                        # unmapped: as read

    want = ["name first", "name 1", "name pair/1"] + ["strip [%s]" % n for n in ("pair", "pair", "pair/3", "", "x/", "1", "", "a/1", "r0")]
    want += lines("ABCDE", "!#$%&"[::-1], "@+>") + ["qual ABCDE EDCBA"] + lines("*", "*", "*") + ["qual * *"]
    assert r.stdout.split("\n") == want + [""]
