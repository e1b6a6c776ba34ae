"""`kiss -g`: the three commands on a text over the byte alphabet (kiss_amd/csrc/host/kiss_cli.cpp), against the Python
entry points.  The file begins with '>' and holds '\\n' and 0x00: a FASTA rule or a stripped newline would change n."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import fm8_model as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")


def run(*args):
    return subprocess.run([KISS, *args], capture_output=True, text=True, errors="replace")


@pytest.fixture(scope="module")
def text_file(tmp_path_factory):
    body = m.english_like(20_000, 6).replace(b"search", b"se\x00rch") + bytes(range(256)) + b"\n>tail\nACGT\n"
    S = b">header line\nACGTNN\n" + body
    path = str(tmp_path_factory.mktemp("g") / "text.bin")
    with open(path, "wb") as f:
        f.write(S)
    return path, S


def test_suffix_sort_writes_the_exact_sa_and_lcp(text_file, tmp_path):
    import kiss_amd
    path, S = text_file
    sa_out, lcp_out = str(tmp_path / "sa.bin"), str(tmp_path / "lcp.bin")
    r = run("-g", "suffix_sort", path, "-k", "32", "-s", "PREFIX_DOUBLING", "--output-sa", sa_out, "--output-lcp", lcp_out)
    assert r.returncode == 0, r.stderr
    assert "n = %d, k = %d, suffix sorting elapsed" % (len(S), 2 ** 64 - 1) in r.stderr  # every byte of the file is text
    assert "ignored" in r.stderr
    sa, lcp = kiss_amd.lcp_array_bytes(S)
    assert np.array_equal(sa, kiss_amd.suffix_array_bytes(S))
    assert open(sa_out, "rb").read() == sa.astype("<u4").tobytes()
    assert open(lcp_out, "rb").read() == lcp.astype("<u4").tobytes()
    # the same file without -g is a FASTA file: another n
    r = run("suffix_sort", path, "-k", "-1")
    assert r.returncode == 0 and "n = %d," % len(S) not in r.stderr


@pytest.mark.parametrize("sa_intv", (4, 1, 9))
def test_build_and_query(text_file, tmp_path, sa_intv):
    from kiss_amd import FMIndexBytes
    path, S = text_file
    r = run("--generic", "fmindex_build", path, "--sa-intv", str(sa_intv))
    assert r.returncode == 0, r.stderr
    fm = FMIndexBytes.load(path + ".fmi8")  # the file the CLI wrote is the file the class reads
    assert (fm.N, fm.sa_intv) == (len(S) + 1, sa_intv)
    assert open(path + ".fmi8", "rb").read() == FMIndexBytes(sa_intv=sa_intv).build(S).to_bytes()
    for q, n_head in (("suffix array", 3), ("ACGT", 10), (">", 10), ("no such words", 10)):
        want = fm.locate(q.encode()).tolist()
        assert want == m.brute(S, q.encode())
        r = run("-g", "fmindex_query", path, "-q", q, "-n", str(n_head))
        assert r.returncode == 0, r.stderr
        assert "[info] query = %s found %d times" % (q, len(want)) in r.stderr
        got = [int(x) for x in re.findall(r"position is (\d+), content of substring is " + re.escape(q), r.stderr)]
        assert got == want[:n_head]
    # batch mode: u32 len, u32 count, raw bytes; a pattern holds 0x00 and '\n'
    L = 6
    pats = [S[p:p + L] for p in (0, 13, 5000, len(S) - L)] + [b"se\x00rch", b".\nthe ", b"\xff\xfe\xfd\xfc\xfb\xfa", b"zzzzzz"]
    pbin = str(tmp_path / "p.bin")
    with open(pbin, "wb") as f:
        f.write(struct.pack("<II", L, len(pats)) + b"".join(pats))
    res = fm.query_batch(pats)
    assert res["total_hits"] == sum(len(m.brute(S, P)) for P in pats)
    r = run("-g", "fmindex_query", path, "-b", pbin)
    assert r.returncode == 0, r.stderr
    assert "[info] query_len: %d, num_query: %d" % (L, len(pats)) in r.stderr
    assert "[info] number of matched locations: %d\n" % res["total_hits"] in r.stderr
    assert "[info] location checksum: %d\n" % res["checksum"] in r.stderr
    fm.close()


def test_rejected_options_and_missing_files(text_file, tmp_path):
    path, _ = text_file
    for extra, name in ((["--gpus", "2"], "--gpus"), (["--devices", "0,0"], "--devices"), (["--lookup-len", "2"], "--lookup-len"),
                        (["--exact"], "--exact"), (["--mismatches", "1"], "--mismatches")):
        for cmd in ("suffix_sort", "fmindex_build", "fmindex_query"):
            r = run("-g", cmd, path, *extra)
            assert r.returncode == 1 and name in r.stderr, (cmd, extra, r.stderr)
    r = run("-g", "suffix_sort", str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "cannot open" in r.stderr
    r = run("-g", "fmindex_query", str(tmp_path / "missing.bin"), "-q", "a")
    assert r.returncode == 1 and "cannot open" in r.stderr
    other = str(tmp_path / "noindex.bin")
    open(other, "wb").write(b"abc")
    r = run("-g", "fmindex_query", other, "-q", "a")
    assert r.returncode == 1 and "fmindex_build" in r.stderr
    open(other + ".fmi8", "wb").write(b"KISSFMI9 not an index")
    r = run("-g", "fmindex_query", other, "-q", "a")
    assert r.returncode == 1 and "magic" in r.stderr
    assert run("-g", "bogus", path).returncode == 1
