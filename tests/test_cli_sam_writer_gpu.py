"""`kiss fmindex_query ... --sam --sam-writer device`: its stdout is byte for byte the stdout without the option (the host
writer), on the three-record FASTA of tests/test_cli_sam_gpu.py: single end and paired, --rescue --md, --ins-auto, FASTQ and
lines, --batch-reads 3; and the option is refused without --sam."""
import os

import numpy as np
import pytest

from tests.test_cli_sam_gpu import make_inputs, revcomp_str
from tests.test_cli_seeds_gpu import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam_writer")
    S, bounds, fa, rf, reads = make_inputs(tmp)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    rng = np.random.default_rng(8)
    letters = lambda a: "".join("ACGT"[c] for c in a)  # noqa: E731
    pairs = []
    for p in range(14):
        frag = int(rng.integers(250, 500))
        at = int(rng.integers(0, S.size - frag))
        a, b = S[at:at + 100].copy(), S[at + frag - 100:at + frag].copy()
        a[40] = (a[40] + 1) & 3
        one, two = letters(a), revcomp_str(letters(b))
        if p == 5:  # a mate without a seed: only the rescue finds it
            two = revcomp_str("".join("ACGT"[(c + (j % 10 == 5)) & 3] for j, c in enumerate(b)))
        if p == 9:
            two = letters(rng.integers(0, 4, 100))  # maps nowhere
        pairs.append((one, two) if p % 2 else (two, one))
    paths = {k: os.path.join(str(tmp), k) for k in ("m1.txt", "m2.txt", "m1.fq", "m2.fq", "single.fq")}
    for i, (txt, fq, tag) in enumerate((("m1.txt", "m1.fq", "/1"), ("m2.txt", "m2.fq", "/2"))):
        with open(paths[txt], "w") as o, open(paths[fq], "w") as q:
            for p, mates in enumerate(pairs):
                o.write((">pair%d words\n" % p if p % 4 else "\n") + mates[i] + "\n")
                qual = "".join(chr(c) for c in rng.integers(33, 127, len(mates[i])))
                q.write("@%s\n%s\n+\n%s\n" % ("" if p % 4 == 0 else "frag%d%s extra" % (p, tag), mates[i], qual))
    with open(paths["single.fq"], "w") as q:
        for k, (name, seq) in enumerate(reads):
            qual = "".join(chr(c) for c in rng.integers(33, 127, len(seq)))
            q.write("@%s\n%s\n+\n%s\n" % (name or "", seq, qual))
    return dict(fa=fa, rf=rf, **paths)


def both_writers(args):
    host, device, named = run(*args), run(*args, "--sam-writer", "device"), run(*args, "--sam-writer", "host")
    assert host.returncode == 0 and device.returncode == 0 and named.returncode == 0, (host.stderr, device.stderr)
    body = [ln for ln in host.stdout.splitlines() if not ln.startswith("@")]
    assert len(body) >= 10 and host.stdout.startswith("@HD")
    assert device.stdout == host.stdout == named.stdout
    return host.stdout


CASES = {
    "single end, lines": ("rf", None, ()),
    "single end, FASTQ, --md": ("single.fq", None, ("--md",)),
    "paired, lines": ("m1.txt", "m2.txt", ()),
    "paired, --rescue --md": ("m1.txt", "m2.txt", ("--rescue", "--md")),
    "paired, --ins-auto": ("m1.txt", "m2.txt", ("--ins-auto", "--ins-auto-min-pairs", "4")),
    "paired, FASTQ, --rescue --md": ("m1.fq", "m2.fq", ("--rescue", "--md")),
    "single end, --batch-reads 3": ("single.fq", None, ("--batch-reads", "3")),
    "paired, FASTQ, --batch-reads 3, --rescue --md": ("m1.fq", "m2.fq", ("--batch-reads", "3", "--rescue", "--md")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_device_writer_prints_the_bytes_of_the_host_writer(files, case):
    reads, mates, more = CASES[case]
    args = ["fmindex_query", files["fa"], "--seeds", files[reads], "--both-strands", "--chain", "--align", "--sam"]
    if mates:
        args += ["--mates", files[mates]]
    out = both_writers(args + list(more))
    assert ("MD:Z:" in out) == ("--md" in more)
    if "--rescue" in more:
        assert "YR:i:1" in out
    if case.endswith("FASTQ, --md"):
        assert "\t*\n" not in out  # (QUAL is the file's)


def test_the_option_is_refused_without_sam_and_with_another_writer(files):
    common = ["fmindex_query", files["fa"], "--seeds", files["rf"], "--both-strands", "--chain", "--align"]
    r = run(*common, "--sam-writer", "device")
    assert r.returncode != 0 and "--sam-writer goes with --sam" in r.stderr and r.stdout == ""
    r = run(*common, "--sam", "--sam-writer", "gpu")
    assert r.returncode != 0 and "--sam-writer is one of host, device" in r.stderr and r.stdout == ""
    r = run("--help-sam")
    assert "--sam-writer" in r.stderr and "EARLIER BATCHES" in r.stderr
