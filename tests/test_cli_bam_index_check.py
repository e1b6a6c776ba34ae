"""The host side of `kiss ... --bam-index` (kiss_amd/csrc/host/cli_bam_index.hpp), compiled alone with AddressSanitizer and UBSan
(tests/cli_bam_index_check.cpp): where FILE.bai goes, the refusal of an index for what goes to stdout, how many
blocks hold the records, and the block offsets that the framing call leaves, held against the framed bytes.  No GPU."""
import subprocess

import pytest

from tests.test_cli_format import program


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return program(tmp_path_factory.mktemp("cli_bam_index_check"), "cli_bam_index_check")


def run(exe, *words):
    r = subprocess.run([exe] + [str(w) for w in words], capture_output=True)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_the_path_of_the_index(exe):
    for name in ("pairs.bam", "dir/with.dots/x", "a b.bam", "x.bam.bam"):
        assert run(exe, "path", name) == (0, name + ".bai", "")


def test_the_index_of_what_goes_to_stdout_is_refused(exe):
    # (that --bam-index goes with --bam-sort, and --bam-sort with --bam, is the option table's: tests/test_cli_bam_index_gpu.py)
    for bam in ("pairs.bam", "dir/-", "-.bam", "--"):
        assert run(exe, "options", 1, bam) == (0, "ok", "")
    for bam in ("pairs.bam", "-"):                                                 # without the option nothing is asked
        assert run(exe, "options", 0, bam) == (0, "ok", "")
    rc, out, err = run(exe, "options", 1, "-")
    assert (rc, out) == (2, "") and "--bam-index" in err and "--bam -" in err and "FILE.bai" in err


def test_the_blocks_that_hold_the_records(exe):
    for n, bb in ((0, 65280), (1, 65280), (65280, 65280), (65281, 65280), (10 * 65280, 65280), (7, 1), (1 << 40, 65280), (100, 7)):
        assert run(exe, "blocks", n, bb) == (0, str(-(-n // bb)), "")
    assert run(exe, "blocks", 5, 0)[0] == 2


def test_the_block_offsets_the_framing_leaves(exe):
    assert run(exe, "frame") == (0, "stored\n", "")
    assert run(exe, "frame", 0, 65280, 0, 0) == (0, "1\n0 \n", "")                # no record: one entry
    assert run(exe, "frame", 3 * 65280 - 1, 65280, 900, 0, 300, 300, 900) == (0, "4\n0 300 300 900 \n", "")
    assert run(exe, "frame", 3 * 65280 + 1, 65280, 900, 0, 300, 600, 800, 900) == (0, "5\n0 300 600 800 900 \n", "")
    assert run(exe, "frame", 2 * 65280, 65280, 900, 0, 300, 600, 900)[0] == 1     # (the check program's own answer: no room for four)
    for words in ((100, 65280, 900, 0, 901), (100, 65280, 900, 1, 900), (130000, 65280, 900, 0, 500)):
        rc, out, err = run(exe, "frame", *words)                                   # the last entry is the framed bytes, the first is 0
        assert (rc, out) == (2, "") and "does not cover" in err, words
    rc, out, err = run(exe, "frame", 3 * 65280, 65280, 900, 0, 600, 300, 900)
    assert (rc, out) == (2, "") and "decreases" in err
