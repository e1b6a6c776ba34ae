"""`kiss fmindex_query --seeds READS --chain --align --sam --bam FILE` on the three-record FASTA of tests/test_cli_sam_gpu.py:
gzip reads the file, it ends with the end-of-file block, its header is kiss_amd.bam_writer.bam_header, its records decoded by
tests/bam_model.py are the alignment lines of the same command without --bam, stdout has no SAM line, and `--bam -` gives the
same bytes on stdout.  Single end, paired, with --rescue --md, from FASTQ, and in batches of three."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import bam_model as B
from tests.test_cli_sam_gpu import RECORDS, make_inputs, revcomp_str
from tests.test_cli_seeds_gpu import KISS

pytestmark = pytest.mark.gpu


def kiss(*args):
    return subprocess.run([KISS] + list(args), capture_output=True)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_bam")
    S, bounds, fa, rf, reads = make_inputs(tmp)
    assert kiss("fmindex_build", "--exact", fa).returncode == 0
    rng = np.random.default_rng(8)
    letters = lambda p, L: "".join("ACGT"[c] for c in S[p:p + L])  # noqa: E731
    pairs = [(letters(p, 100), revcomp_str(letters(p + 150, 100))) for p in (200, 3000, 6500, 9000, 12000, 15000, 17000)]
    pairs.append((letters(4000, 100), "".join("ACGT"[c] for c in rng.integers(0, 4, 100))))  # a mate that maps nowhere
    files = {}
    for i in (0, 1):
        files["m%d.txt" % i] = "".join(">p%d words\n%s\n" % (p, pr[i]) for p, pr in enumerate(pairs))
        files["m%d.fq" % i] = "".join("@p%d/%d\n%s\n+\n%s\n" % (p, i + 1, pr[i], "".join(chr(33 + (7 * p + k) % 60) for k in range(100)))
                                      for p, pr in enumerate(pairs))
    for name, body in files.items():
        with open(os.path.join(str(tmp), name), "w") as o:
            o.write(body)
    at = lambda name: os.path.join(str(tmp), name)  # noqa: E731
    return {"fa": fa, "reads": rf, "bounds": bounds, "at": at, "tmp": str(tmp)}


VARIANTS = {
    "single": lambda x: ["--seeds", x["reads"], "--both-strands"],
    "paired": lambda x: ["--seeds", x["at"]("m0.txt"), "--mates", x["at"]("m1.txt")],
    "rescue, md": lambda x: ["--seeds", x["at"]("m0.txt"), "--mates", x["at"]("m1.txt"), "--rescue", "--md"],
    "fastq": lambda x: ["--seeds", x["at"]("m0.fq"), "--both-strands", "--md"],
    "batches of 3": lambda x: ["--seeds", x["at"]("m0.fq"), "--mates", x["at"]("m1.fq"), "--batch-reads", "3", "--ins-auto"],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bam_on_the_command_line(inputs, variant):
    import kiss_amd.bam_writer as W
    common = ["fmindex_query", inputs["fa"]] + VARIANTS[variant](inputs) + ["--chain", "--align", "--sam"]
    sam = kiss(*common)
    assert sam.returncode == 0, sam.stderr
    lines = sam.stdout.splitlines(keepends=True)
    header = b"".join(ln for ln in lines if ln.startswith(b"@"))
    body = [ln for ln in lines if not ln.startswith(b"@")]
    assert len(body) >= 8 and header.count(b"@SQ") == 3
    path = os.path.join(inputs["tmp"], "out.bam")
    r = kiss(*common, "--bam", path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"" and b"[info] bam: records: %d," % len(body) in r.stderr
    blob = open(path, "rb").read()
    assert blob.endswith(B.BGZF_EOF)
    raw = gzip.decompress(blob)
    version = header.rsplit(b"VN:", 1)[1].strip().decode()
    names = [name.encode() for name, _, _ in RECORDS]
    want_head = W.bam_header(names, inputs["bounds"], version)
    assert want_head[8:8 + len(header)] == header
    head, recs = B.skip_header(raw)
    assert head == want_head
    assert [B.bam_to_sam(x, names) for x in B.split_records(recs)] == body
    if variant == "rescue, md":
        assert b"MDZ" in recs and b"YTZCP\0" in recs
    if variant == "fastq":
        assert any(ln.split(b"\t")[10] != b"*" for ln in body)
    piped = kiss(*common, "--bam", "-")
    assert piped.returncode == 0 and gzip.decompress(piped.stdout) == raw and piped.stdout == blob


def test_bam_goes_with_sam_and_has_its_own_help(inputs):
    r = kiss("fmindex_query", inputs["fa"], "--seeds", inputs["reads"], "--chain", "--align", "--bam", os.path.join(inputs["tmp"], "no.bam"))
    assert r.returncode != 0 and r.stdout == b"" and b"--bam goes with --sam" in r.stderr
    assert not os.path.exists(os.path.join(inputs["tmp"], "no.bam"))
    h = kiss("--help-bam")
    assert b"--bam FILE" in h.stderr and b"samtools sort" in h.stderr
    assert b"--bam" not in kiss("-h").stderr and b"--bam" not in kiss("--help-sam").stderr
