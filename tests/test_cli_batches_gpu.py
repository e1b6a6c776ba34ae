"""`kiss fmindex_query --seeds READS [--mates READS2] --chain --align --sam --batch-reads N [--batch-chunk BYTES]` on the inputs of
tests/test_cli_sam_gpu.py and tests/test_cli_pairs_gpu.py: stdout is BYTE-EQUAL to the run without the option for N = 1, 3, the
read count and one more, with chunks of 64 bytes and of the default size, single-end, paired and with --rescue --md, from FASTQ
files and from lines files (whose reads without a name get their number in the file as QNAME).  A bad record in the third batch
is named by its number in the file behind the SAM lines of the first two; mate files of different lengths are refused;
--batch-reads goes with --sam; --ins-auto prints one [insert] line, from the first batch, and its SAM is that of the three values
given explicitly."""
import os

import pytest

from tests import test_cli_pairs_gpu, test_cli_sam_gpu
from tests.test_cli_fastq_gpu import write_fastq
from tests.test_cli_insert_gpu import LINE
from tests.test_cli_seeds_gpu import run

pytestmark = pytest.mark.gpu
TAIL = ["--chain", "--align", "--sam"]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """-> fasta, {"lines": [file], "fastq": [file]}, the read count"""
    tmp = tmp_path_factory.mktemp("single")
    _, _, fa, rf, reads = test_cli_sam_gpu.make_inputs(tmp)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    fq = os.path.join(str(tmp), "reads.fastq")
    write_fastq(fq, reads, 1)
    return fa, {"lines": [rf], "fastq": [fq]}, len(reads)


@pytest.fixture(scope="module")
def paired(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("paired")
    _, _, fa, files, pairs = test_cli_pairs_gpu.make_inputs(tmp)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    fq = [os.path.join(str(tmp), "reads_%d.fastq" % (m + 1)) for m in (0, 1)]
    for m in (0, 1):
        write_fastq(fq[m], [(p[2 * m], p[2 * m + 1]) for p in pairs], 20 + m)
    return fa, {"lines": files, "fastq": fq}, len(pairs)


def command(fa, files, *extra):
    return ["fmindex_query", fa, "--seeds", files[0]] + (["--mates", files[1]] if len(files) > 1 else ["--both-strands"]) + TAIL + list(extra)


@pytest.mark.parametrize("chunk", ([], ["--batch-chunk", "64"]))
@pytest.mark.parametrize("fmt", ("lines", "fastq"))
@pytest.mark.parametrize("mode", ("single", "paired", "rescue_md"))
def test_stdout_does_not_depend_on_the_batches(single, paired, mode, fmt, chunk):
    fa, files, Q = single if mode == "single" else paired
    extra = ["--rescue", "--md"] if mode == "rescue_md" else []
    whole = run(*command(fa, files[fmt], *extra))
    assert whole.returncode == 0 and whole.stdout.count("\n") > Q + 4, whole.stderr
    if fmt == "lines":  # reads without a name: their number in the file
        assert any(ln.split("\t")[0] == ("3" if mode == "single" else "4") for ln in whole.stdout.splitlines())
    for n in (1, 3, Q, Q + 1):
        r = run(*command(fa, files[fmt], *extra), "--batch-reads", str(n), *chunk)
        assert r.returncode == 0, r.stderr
        assert r.stdout == whole.stdout, (n, chunk)
        assert "[info] batches: %d, reads: %d," % (-(-Q // n), Q * (1 if mode == "single" else 2)) in r.stderr, r.stderr


def test_an_error_in_the_third_batch_comes_behind_the_lines_of_the_first_two(single, tmp_path):
    fa, files, Q = single
    with open(files["fastq"][0]) as i:
        ls = i.read().split("\n")
    whole = run(*command(fa, files["fastq"]))
    assert whole.returncode == 0
    bad = os.path.join(str(tmp_path), "bad.fastq")
    ls[4 * 7 + 3] = ls[4 * 7 + 3][:-1]  # record 7, in the third batch of 3: one quality short
    with open(bad, "w") as o:
        o.write("\n".join(ls))
    first_six = run(*command(fa, [bad]), "--batch-reads", "6")
    r = run(*command(fa, [bad]), "--batch-reads", "3", "--batch-chunk", "64")
    assert r.returncode != 0 and "record 7:" in r.stderr and "differ in length" in r.stderr
    assert first_six.returncode != 0 and "record 7:" in first_six.stderr
    assert r.stdout == first_six.stdout and r.stdout and whole.stdout.startswith(r.stdout)
    names = [ln.split("\t")[0] for ln in r.stdout.splitlines() if not ln.startswith("@")]
    assert set(names) == {"r0", "1", "r2/1", "3", "across", "junk"}
    ls[4 * 7 + 1] = ls[4 * 7 + 3] = ""  # read 7 without bases
    with open(bad, "w") as o:
        o.write("\n".join(ls))
    r = run(*command(fa, [bad]), "--batch-reads", "3")
    assert r.returncode != 0 and r.stdout == first_six.stdout and "read 7 of" in r.stderr and "no bases" in r.stderr


def test_mate_files_of_different_lengths_are_refused(paired, tmp_path):
    fa, files, P = paired
    for fmt in ("fastq", "lines"):
        with open(files[fmt][1]) as i:
            ls = i.read().split("\n")
        short = os.path.join(str(tmp_path), "short." + fmt)
        with open(short, "w") as o:
            o.write("\n".join(ls[:-5 if fmt == "fastq" else -3]) + "\n")  # the last mate is missing
        for n, order in ((3, [files[fmt][0], short]), (P if fmt == "lines" else P + 1, [short, files[fmt][0]])):
            r = run(*command(fa, order), "--batch-reads", str(n))
            assert r.returncode != 0 and "a pair has one of each" in r.stderr and short + " ends after %d reads" % (P - 1) in r.stderr, r.stderr
    r = run(*command(fa, [files["fastq"][0], files["lines"][1]]), "--batch-reads", "3")
    assert r.returncode != 0 and "differ in format" in r.stderr


def test_usage(single):
    fa, files, _ = single
    r = run("fmindex_query", fa, "--seeds", files["lines"][0], "--chain", "--align", "--batch-reads", "3")
    assert r.returncode != 0 and r.stdout == "" and "--batch-reads goes with --sam" in r.stderr
    r = run(*command(fa, files["lines"]), "--batch-chunk", "64")
    assert r.returncode != 0 and r.stdout == "" and "--batch-chunk goes with --batch-reads" in r.stderr
    r = run(*command(fa, files["lines"]), "--batch-reads", "3", "--batch-chunk", "0")
    assert r.returncode != 0 and r.stdout == "" and "--batch-chunk is in 1.." in r.stderr
    zero = run(*command(fa, files["lines"]), "--batch-reads", "0")  # 0: the whole file, as without the option
    assert zero.returncode == 0 and zero.stdout == run(*command(fa, files["lines"])).stdout and "[info] batches" not in zero.stderr
    h = run("--help-reads")
    assert h.returncode == 1 and h.stdout == ""
    for word in ("--batch-reads NUM (=0)", "--batch-chunk BYTES (=67108864)", "behind the SAM lines of the batches before it", "[insert]"):
        assert word in h.stderr
    assert "--batch-reads" not in run("-h").stderr


def test_ins_auto_is_estimated_once_from_the_first_batch(tmp_path):
    from tests.test_fm_insert_gpu import insert_truth_case
    S, m1, m2, _ = insert_truth_case()
    fa = os.path.join(str(tmp_path), "one.fa")
    with open(fa, "w") as o:
        letters = "".join("ACGT"[c] for c in S)
        o.write(">chr1\n" + "".join(letters[at:at + 61] + "\n" for at in range(0, len(letters), 61)))
    files = []
    for which, mates in enumerate((m1, m2)):
        files.append(os.path.join(str(tmp_path), "lib%d.txt" % (which + 1)))
        with open(files[-1], "w") as o:
            o.write("".join("".join("ACGT"[c] for c in r) + "\n" for r in mates))
    assert run("fmindex_build", "--exact", fa).returncode == 0
    auto = run(*command(fa, files), "--ins-auto", "--batch-reads", "100")
    assert auto.returncode == 0, auto.stderr
    found = LINE.findall(auto.stderr)
    assert len(found) == 1 and found[0][0] == "100" and found[0][-1] == "1", auto.stderr  # one line, of the 100 pairs of batch 0
    mean, ins_min, ins_max = found[0][6], found[0][8], found[0][9]
    given = run(*command(fa, files), "--ins-min", ins_min, "--ins-max", ins_max, "--ins-mean", mean)
    assert given.returncode == 0 and given.stdout == auto.stdout
    body = [ln.split("\t") for ln in auto.stdout.splitlines() if not ln.startswith("@")]
    assert len(body) == 400 and all(int(x[1]) & 2 for x in body)  # every pair proper, those of the second batch too
    few = run(*command(fa, files), "--ins-auto", "--batch-reads", "20")  # 20 pairs: below --ins-auto-min-pairs, the defaults serve
    assert few.returncode == 0 and few.stdout == run(*command(fa, files)).stdout
    found = LINE.findall(few.stderr)
    assert len(found) == 1 and found[0][0] == "20" and found[0][-1] == "0"
