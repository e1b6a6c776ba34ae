"""`kiss fmindex_query --seeds reads.fastq [--mates mates.fastq] --chain --align --sam` on the three-record FASTA and the reads of
tests/test_cli_sam_gpu.py and tests/test_cli_pairs_gpu.py: the same reads written once as lines and once as FASTQ with random
qualities give the same SAM in every column but QUAL, which is the written string, reversed exactly on the FLAG 16 lines;
mates named x/1 and x/2 share one QNAME; a bad record, a read without bases and two files of different formats stop the command
with a message; --reads-format lines on a FASTQ file reads it as the command line always did."""
import os

import numpy as np
import pytest

from tests import test_cli_pairs_gpu, test_cli_sam_gpu
from tests.test_cli_seeds_gpu import run

pytestmark = pytest.mark.gpu


def write_fastq(path, reads, seed, suffix="", eol="\n"):
    """reads: [(name or None, letters)] -> the quality string of every read"""
    rng = np.random.default_rng(seed)
    quals = []
    with open(path, "w", newline="") as o:
        for name, letters in reads:
            # (any printable byte but '>': read as lines, a quality line that starts with it would be a header)
            quals.append("".join(chr(c) for c in rng.integers(33, 127, len(letters))).replace(">", "?"))
            o.write("@" + (name + suffix + " some words" if name else "") + eol + letters + eol + "+" + eol + quals[-1] + eol)
    return quals


def body(r):
    assert r.returncode == 0, r.stderr
    return [ln.split("\t") for ln in r.stdout.splitlines() if not ln.startswith("@")]


def check_qual(fastq_body, lines_body, quals_of_qname_and_mate):
    """every column but QUAL as from the lines file; QUAL the written string, reversed on the FLAG 16 lines"""
    assert len(fastq_body) == len(lines_body) > 0
    reversed_lines = 0
    for got, want in zip(fastq_body, lines_body):
        assert got[:10] == want[:10] and got[11:] == want[11:] and want[10] == "*"
        flag = int(got[1])
        written = quals_of_qname_and_mate(got[0], flag)
        assert got[10] == (written[::-1] if flag & 16 else written), got[:2]
        assert len(got[10]) == len(got[9])
        reversed_lines += bool(flag & 16)
    assert reversed_lines > 0 and any(int(x[1]) & 4 for x in fastq_body)


def test_fastq_reads_give_the_sam_of_the_same_reads_as_lines_with_their_qualities(tmp_path):
    _, _, fa, rf, reads = test_cli_sam_gpu.make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    fq = os.path.join(str(tmp_path), "reads.fastq")
    quals = write_fastq(fq, reads, 1)
    by_name = {(name if name else str(q)): quals[q] for q, (name, _) in enumerate(reads)}
    tail = ["--both-strands", "--chain", "--align", "--sam"]
    lines_body = body(run("fmindex_query", fa, "--seeds", rf, *tail))
    for extra in ([], ["--reads-format", "fastq"], ["--reads-format", "auto"]):
        check_qual(body(run("fmindex_query", fa, "--seeds", fq, *tail, *extra)), lines_body, lambda qname, flag: by_name[qname])
    # '\r\n' line ends, no final newline
    crlf = os.path.join(str(tmp_path), "crlf.fastq")
    write_fastq(crlf, reads, 1, eol="\r\n")
    with open(crlf, "rb") as i:
        data = i.read()
    with open(crlf, "wb") as o:
        o.write(data[:-2])
    check_qual(body(run("fmindex_query", fa, "--seeds", crlf, *tail)), lines_body, lambda qname, flag: by_name[qname])
    # the other exits of the pipeline do not depend on the format
    for upto in (["--chain"], ["--chain", "--align"], []):
        a, b = run("fmindex_query", fa, "--seeds", rf, *upto), run("fmindex_query", fa, "--seeds", fq, *upto)
        assert a.returncode == 0 and a.stdout == b.stdout and a.stdout

    # --reads-format lines on the FASTQ file: every line a read, as the command line read such a file before it knew FASTQ
    as_lines = body(run("fmindex_query", fa, "--seeds", fq, *tail, "--reads-format", "lines"))
    assert [x[0] for x in as_lines if not int(x[1]) & (256 | 2048)] == [str(k) for k in range(4 * len(reads))]  # (no name: none starts with '>')
    letters_of = lambda text: "".join(c.upper() if c in "ACGTacgt" else "N" for c in text)  # noqa: E731
    first = {x[0]: x for x in reversed(as_lines)}
    for q, (name, letters) in enumerate(reads):
        header = "@" + (name + " some words" if name else "")
        assert first[str(4 * q)][1:6] == ["4", "*", "0", "0", "*"] and first[str(4 * q)][9] == letters_of(header)  # the '@' line: no bases to speak of
        assert first[str(4 * q + 2)][1:6] == ["4", "*", "0", "0", "*"] and first[str(4 * q + 2)][9] == "N"          # the '+' line
        assert all(x[10] == "*" for x in as_lines)
    seq_lines = [x[1:] for x in as_lines if int(x[0]) % 4 == 1]
    assert seq_lines == [x[1:] for x in lines_body]  # the sequence lines map as they do from the lines file

    # what stops the command
    bad = os.path.join(str(tmp_path), "bad.fastq")
    with open(fq) as i:
        ls = i.read().split("\n")
    ls[4 * 3 + 3] = ls[4 * 3 + 3][:-1]  # record 3: one quality short
    with open(bad, "w") as o:
        o.write("\n".join(ls))
    r = run("fmindex_query", fa, "--seeds", bad, *tail)
    assert r.returncode != 0 and r.stdout == "" and "record 3" in r.stderr and "differ in length" in r.stderr
    ls[4 * 3 + 1] = ls[4 * 3 + 3] = ""  # record 3 without bases
    with open(bad, "w") as o:
        o.write("\n".join(ls))
    r = run("fmindex_query", fa, "--seeds", bad, *tail)
    assert r.returncode != 0 and r.stdout == "" and "read 3" in r.stderr and "no bases" in r.stderr
    r = run("fmindex_query", fa, "--seeds", fq, *tail, "--reads-format", "fasta")
    assert r.returncode != 0 and r.stdout == "" and "--reads-format is one of auto, lines, fastq" in r.stderr
    r = run("fmindex_query", fa, "-q", "ACGT", "--reads-format", "fastq")
    assert r.returncode != 0 and "--reads-format goes with --seeds" in r.stderr
    r = run("--help-reads")
    assert r.returncode == 1 and r.stdout == "" and "--reads-format" in r.stderr and "fastq" in r.stderr


def test_fastq_mates_share_one_qname_and_carry_their_qualities(tmp_path):
    _, _, fa, (rf1, rf2), pairs = test_cli_pairs_gpu.make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    mates = [[(p[0], p[1]) for p in pairs], [(p[2], p[3]) for p in pairs]]
    fq = [os.path.join(str(tmp_path), "reads_%d.fastq" % (m + 1)) for m in (0, 1)]
    # names that end in /1 and /2: "lonely/1" and "lonely/2" are in the inputs; every other named pair gets the suffix here
    quals = [write_fastq(fq[m], [(n, s) if n is None or "/" in n else (n + "/%d" % (m + 1), s) for n, s in mates[m]], 20 + m) for m in (0, 1)]
    qname = [(pairs[p][0] or str(p)).split("/")[0] for p in range(len(pairs))]
    assert "lonely" in qname and len(set(qname)) == len(qname)
    at = {name: p for p, name in enumerate(qname)}

    def written(name, flag):
        return quals[1 if flag & 128 else 0][at[name]]

    for extra in ([], ["--rescue"]):
        tail = ["--chain", "--align", "--sam", *extra]
        lines_body = body(run("fmindex_query", fa, "--seeds", rf1, "--mates", rf2, *tail))
        got = body(run("fmindex_query", fa, "--seeds", fq[0], "--mates", fq[1], *tail))
        for x in lines_body:  # from the lines files the names stay as they are: lonely/1 and lonely/2
            x[0] = x[0].split("/")[0]
        assert {x[0] for x in lines_body} == set(qname)
        check_qual(got, lines_body, written)
        for p, name in enumerate(qname):  # both mates carry one QNAME
            flags = [int(x[1]) for x in got if x[0] == name]
            assert any(f & 64 for f in flags) and any(f & 128 for f in flags)
    # one file FASTQ, one of lines: refused
    r = run("fmindex_query", fa, "--seeds", fq[0], "--mates", rf2, "--chain", "--align", "--sam")
    assert r.returncode != 0 and r.stdout == "" and "differ in format" in r.stderr
