"""What `kiss ... --bam-sort` keeps between the batches (kiss_amd/csrc/host/cli_bam_sort.hpp), compiled alone with AddressSanitizer
and UBSan (tests/cli_bam_sort_check.cpp): batches of 0, 1 and many records give the straightforward concatenation of their bytes
and the rebased index, and the header with SO:coordinate is kiss_amd.bam_writer.bam_header(sort_order="coordinate").  No GPU."""
import subprocess

import numpy as np
import pytest

import kiss_amd.bam_writer as W
from kiss_amd import sam_header
from tests.test_cli_format import program


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return program(tmp_path_factory.mktemp("cli_bam_sort_check"), "cli_bam_sort_check")


@pytest.mark.parametrize("batches", [[], [[]], [[36]], [[], [40], []], [[36, 37, 300], [], [1000], [41] * 50, [5000, 36]], [[36]] * 7],
                         ids=["no batch", "one empty batch", "one record", "empty batches around one record", "many", "seven batches of one"])
def test_the_kept_records_are_the_concatenation(exe, tmp_path, batches):
    rng = np.random.default_rng(len(batches))
    sizes = [s for b in batches for s in b]
    raw = rng.integers(0, 256, sum(sizes), dtype=np.uint8).tobytes()
    f = tmp_path / "bytes"
    f.write_bytes(raw)
    out = subprocess.check_output([exe, "records", str(f)] + [",".join(map(str, b)) or "-" for b in batches]).decode().split("\n")
    assert int(out[0]) == len(sizes)
    assert [int(x) for x in out[1].split()] == [0] + np.cumsum(sizes, dtype=np.int64).tolist()
    assert bytes.fromhex(out[2]) == raw


def test_an_index_that_does_not_cover_its_bytes_is_refused(exe, tmp_path):
    f = tmp_path / "bytes"
    f.write_bytes(b"x" * 10)
    r = subprocess.run([exe, "records", str(f), "36"], capture_output=True)
    assert r.returncode == 1 and not r.stdout  # (the check program's own answer: more bytes asked for than the file has)


def test_the_header_with_coordinate_order_is_bam_header(exe, tmp_path):
    for names, bounds in (([b"chrA", b"chrB", b"c"], [0, 100, 250, 251]), ([b"one record"], [0, (1 << 31) - 1])):
        text = tmp_path / "text"
        text.write_bytes(sam_header(names, bounds, "X"))  # (the lines as the command line has them: SO:unsorted)
        got = subprocess.check_output([exe, "header", str(text), str(len(names))] + [n.decode() for n in names] + [str(x) for x in bounds])
        assert got == W.bam_header(names, bounds, "X", sort_order="coordinate")
        assert got != W.bam_header(names, bounds, "X")
    text.write_bytes(b"@SQ\tSN:x\tLN:5\n")
    r = subprocess.run([exe, "header", str(text), "1", "x", "0", "5"], capture_output=True)
    assert r.returncode == 2 and b"@HD" in r.stderr and not r.stdout
