"""`kiss fmindex_query ... --sam --bam FILE --bam-compress` on the three-record FASTA of tests/test_cli_bam_gpu.py: the file, and
the bytes of `--bam -`, decompress to exactly what `--bam FILE` alone decompresses to, the file is strictly smaller, and
--bam-compress without --bam is refused with a message.  Single end, paired, with --rescue --md, and FASTQ in batches of three."""
import gzip
import os

import pytest

from tests import bam_model as B
from tests.test_cli_bam_gpu import VARIANTS, inputs, kiss  # noqa: F401  (inputs is the fixture)

pytestmark = pytest.mark.gpu

CASES = {k: VARIANTS[k] for k in ("single", "paired", "rescue, md", "batches of 3")}


@pytest.mark.parametrize("variant", sorted(CASES))
def test_bam_compress_on_the_command_line(inputs, variant):  # noqa: F811
    common = ["fmindex_query", inputs["fa"]] + CASES[variant](inputs) + ["--chain", "--align", "--sam"]
    stored, packed = os.path.join(inputs["tmp"], "stored.bam"), os.path.join(inputs["tmp"], "packed.bam")
    r = kiss(*common, "--bam", stored)
    assert r.returncode == 0, r.stderr
    r = kiss(*common, "--bam", packed, "--bam-compress")
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    blob, small = open(stored, "rb").read(), open(packed, "rb").read()
    raw = gzip.decompress(blob)
    assert small.endswith(B.BGZF_EOF) and gzip.decompress(small) == raw and len(small) < len(blob)
    assert b"[info] bam: records: %d, bytes: %d" % (len(B.split_records(B.skip_header(raw)[1])), len(small)) in r.stderr
    piped = kiss(*common, "--bam", "-", "--bam-compress")
    assert piped.returncode == 0 and piped.stdout == small


def test_bam_compress_goes_with_bam_and_is_in_the_help(inputs):  # noqa: F811
    no = os.path.join(inputs["tmp"], "no.bam")
    r = kiss("fmindex_query", inputs["fa"], "--seeds", inputs["reads"], "--both-strands", "--chain", "--align", "--sam", "--bam-compress")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-compress goes with --bam" in r.stderr and not os.path.exists(no)
    h = kiss("--help-bam")
    assert b"--bam-compress" in h.stderr and b"kiss_hip_bgzf_deflate_host" in h.stderr and b"--bam FILE" in h.stderr
