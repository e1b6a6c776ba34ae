"""`kiss suffix_sort ... --output-lcp FILE`: the LCP array of the exact suffix array, as the Python entry gives it."""
import os
import subprocess

import numpy as np
import pytest

from tests import gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")


def write_fasta(path, S):
    seq = "".join("ACGT"[int(c)] for c in S)
    with open(path, "w") as f:
        f.write(">chr1 lcp test\n")
        for i in range(0, len(seq), 80):
            f.write(seq[i:i + 80] + "\n")


@pytest.mark.parametrize("algo", ["PARALLEL_SORTING", "PREFIX_DOUBLING"])
def test_cli_output_lcp_equals_python(tmp_path, algo):
    import kiss_amd
    S = gen.genome_like(300_000, 21)
    fa, sa_f, lcp_f = str(tmp_path / "x.fa"), str(tmp_path / "sa"), str(tmp_path / "lcp")
    write_fasta(fa, S)
    r = subprocess.run([KISS, "suffix_sort", fa, "-k", "-1", "-s", algo, "--output-sa", sa_f, "--output-lcp", lcp_f],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "LCP array elapsed" in r.stderr
    SA, LCP = kiss_amd.lcp_array(S)
    assert np.array_equal(np.fromfile(sa_f, dtype="<u4"), SA)
    assert np.array_equal(np.fromfile(lcp_f, dtype="<u4"), LCP)


@pytest.mark.parametrize("text", [">h\n>AAAAAAAAAA\nAAAA\n", ">h\nAC>GTACGTAC\n", ">a\n>b\n>c\nAC\n", ">h\nACGT\n>h2\n>CC\nG"])
def test_cli_bounded_k_is_checked_against_the_parsed_length(tmp_path, text):
    # a second line that begins with '>' is sequence, and so is a '>' inside a line: k = n - 1 (n as the device parses the
    # file) is refused, k = n writes the LCP of the exact suffix array
    import kiss_amd
    fa, lcp_f = str(tmp_path / "x.fa"), str(tmp_path / "lcp")
    with open(fa, "w") as f:
        f.write(text)
    with kiss_amd.Context(max_n=1000) as ctx:
        S = ctx.read_sequence(fa)
    n = S.size
    r = subprocess.run([KISS, "suffix_sort", fa, "-k", str(n - 1), "--output-lcp", lcp_f], capture_output=True, text=True)
    assert r.returncode != 0 and "needs the exact suffix array" in r.stderr and not os.path.exists(lcp_f)
    assert "suffix sorting elapsed" not in r.stderr
    r = subprocess.run([KISS, "suffix_sort", fa, "-k", str(n), "--output-lcp", lcp_f], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(lcp_f, dtype="<u4"), kiss_amd.lcp_array(S)[1])


def test_cli_output_lcp_with_k_at_least_n(tmp_path):
    import kiss_amd
    S = gen.iid(5000, 22)
    fa, lcp_f = str(tmp_path / "x.fa"), str(tmp_path / "lcp")
    write_fasta(fa, S)
    r = subprocess.run([KISS, "suffix_sort", fa, "-k", "5000", "--output-lcp", lcp_f], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(lcp_f, dtype="<u4"), kiss_amd.lcp_array(S)[1])
    r = subprocess.run([KISS, "suffix_sort", fa, "-k", "4999", "--output-lcp", lcp_f + "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "needs the exact suffix array" in r.stderr and not os.path.exists(lcp_f + "2")
