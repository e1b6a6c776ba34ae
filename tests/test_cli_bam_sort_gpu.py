"""`kiss fmindex_query ... --sam --bam FILE --bam-sort` on the inputs of tests/test_cli_bam_gpu.py: the file decodes to the header
with SO:coordinate and to tests/bam_sort_model.py's sort of the records of the same command without --bam-sort, with and without
--bam-compress; `--bam -` gives the same bytes on stdout; --bam-sort without --bam is refused with a message and no file; `kiss -h`
does not mention the option and `kiss --help-bam` does.  Single end, paired, with --rescue --md, FASTQ, and in batches of three."""
import gzip
import os

import pytest

from tests import bam_model as B
from tests import bam_sort_model as M
from tests.test_cli_bam_gpu import VARIANTS, inputs, kiss  # noqa: F401
from tests.test_cli_sam_gpu import RECORDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bam_sort_on_the_command_line(inputs, variant):  # noqa: F811
    import kiss_amd.bam_writer as W
    common = ["fmindex_query", inputs["fa"]] + VARIANTS[variant](inputs) + ["--chain", "--align", "--sam"]
    plain_path, path = os.path.join(inputs["tmp"], "plain.bam"), os.path.join(inputs["tmp"], "sorted.bam")
    r = kiss(*common, "--bam", plain_path)
    assert r.returncode == 0, r.stderr
    head, plain = B.skip_header(gzip.decompress(open(plain_path, "rb").read()))
    names = [name.encode() for name, _, _ in RECORDS]
    text = head[8:8 + int.from_bytes(head[4:8], "little")]
    version = text.rsplit(b"VN:", 1)[1].strip().decode()
    assert head == W.bam_header(names, inputs["bounds"], version)
    want_head = W.bam_header(names, inputs["bounds"], version, sort_order="coordinate")
    recs = B.split_records(plain)
    want = M.sort(*M.pack(recs), len(names))
    assert len(recs) >= 8 and want["order"].tolist() != list(range(len(recs)))  # (there is something to sort)
    for more in ([], ["--bam-compress"]):
        if os.path.exists(path):
            os.remove(path)
        r = kiss(*common, "--bam", path, "--bam-sort", *more)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b"" and b"[info] bam: records: %d," % len(recs) in r.stderr
        assert b"[info] bam sort: records: %d, unplaced: %d," % (len(recs), want["report"]["unplaced"]) in r.stderr
        blob = open(path, "rb").read()
        assert blob.endswith(B.BGZF_EOF)
        got_head, got = B.skip_header(gzip.decompress(blob))
        assert got_head == want_head and b"SO:coordinate" in got_head and got_head != head
        assert got == want["bam"].tobytes(), (variant, more)
        assert [B.bam_to_sam(x, names) for x in B.split_records(got)] == [B.bam_to_sam(recs[i], names) for i in want["order"]]
        piped = kiss(*common, "--bam", "-", "--bam-sort", *more)
        assert piped.returncode == 0 and piped.stdout == blob
    assert len(blob) < os.path.getsize(plain_path)  # (the compressed one)


def test_bam_sort_goes_with_bam_and_is_in_its_help_only(inputs):  # noqa: F811
    no = os.path.join(inputs["tmp"], "no.bam")
    r = kiss("fmindex_query", inputs["fa"], "--seeds", inputs["reads"], "--both-strands", "--chain", "--align", "--sam", "--bam-sort")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-sort goes with --bam" in r.stderr and not os.path.exists(no)
    h = kiss("--help-bam")
    assert b"--bam-sort" in h.stderr and b"kiss_hip_bam_sort_host" in h.stderr and b"--bam FILE" in h.stderr and b"samtools sort" in h.stderr
    assert b"--bam-sort" not in kiss("-h").stderr
