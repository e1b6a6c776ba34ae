"""`kiss fmindex_query ... --sam --bam FILE --bam-sort --bam-index` on the inputs of tests/test_cli_bam_gpu.py: FILE.bai is the
model's index (tests/bai_model.py) of the records and blocks found in FILE, a reader that goes through it finds what overlaps a
region, FILE and stdout are byte for byte those of the run without the option, with and without --bam-compress; the option is
refused with `--bam -` and without --bam-sort, with a message and nothing written; `kiss -h` does not mention it and
`kiss --help-bam` does.  Single end, paired, with --rescue --md, FASTQ, and in batches of three."""
import os

import pytest

from tests.test_cli_bam_gpu import VARIANTS, inputs, kiss  # noqa: F401
from tests.test_map_bam_index_gpu import check_index

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bam_index_on_the_command_line(inputs, variant):  # noqa: F811
    common = ["fmindex_query", inputs["fa"]] + VARIANTS[variant](inputs) + ["--chain", "--align", "--sam"]
    plain_path, path = os.path.join(inputs["tmp"], "sorted.bam"), os.path.join(inputs["tmp"], "indexed.bam")
    for more in ([], ["--bam-compress"]):
        for p in (plain_path, path, path + ".bai"):
            if os.path.exists(p):
                os.remove(p)
        plain = kiss(*common, "--bam", plain_path, "--bam-sort", *more)
        assert plain.returncode == 0 and not os.path.exists(plain_path + ".bai"), plain.stderr
        r = kiss(*common, "--bam", path, "--bam-sort", "--bam-index", *more)
        assert r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout == b""
        blob, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
        assert blob == open(plain_path, "rb").read(), (variant, more)
        recs = check_index(blob, bai, inputs["bounds"])
        assert len(recs) >= 8 and b"[info] bam index: bytes: %d," % len(bai) in r.stderr
        assert os.path.getmtime(path + ".bai") >= os.path.getmtime(path)


def test_bam_index_goes_with_a_sorted_file_and_is_in_the_bam_help_only(inputs):  # noqa: F811
    no = os.path.join(inputs["tmp"], "no.bam")
    common = ["fmindex_query", inputs["fa"], "--seeds", inputs["reads"], "--both-strands", "--chain", "--align", "--sam"]
    r = kiss(*common, "--bam", no, "--bam-index")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-index goes with --bam-sort" in r.stderr
    assert not os.path.exists(no) and not os.path.exists(no + ".bai")
    r = kiss(*common, "--bam", "-", "--bam-sort", "--bam-index")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-index" in r.stderr and b"--bam -" in r.stderr
    assert not os.path.exists("-.bai") and not os.path.exists(os.path.join(inputs["tmp"], "-.bai"))
    h = kiss("--help-bam")
    assert b"--bam-index" in h.stderr and b"kiss_hip_bai_host" in h.stderr and b"FILE.bai" in h.stderr
    assert b"--bam-index" not in kiss("-h").stderr
