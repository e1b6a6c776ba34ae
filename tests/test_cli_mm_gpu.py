"""`kiss fmindex_build --exact` and `kiss fmindex_query --mismatches E` on a small FASTA, against the text itself
(tests/fm_mm_model.py)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import fm_mm_model as mm
from tests import gen
from tests.test_cli_gpu import write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")
NAMED_ERROR = "the positions need an index built with fmindex_build --exact"


def run(*args):
    return subprocess.run([KISS] + list(args), capture_output=True, text=True)


def text():
    S = gen.genome_like(60_000, 21)
    S[20_000:26_000] = np.tile(np.array([0, 2, 3], np.uint8), 2000)  # a tandem array: ties deeper than 32 bases
    return S


def single_query_matches(S, q, e, stderr, headn):
    c, p, m = mm.brute(S, q, e)
    qs = "".join("ACGT"[x] for x in q)
    head = re.search(r"query = %s found (\d+) times \(([^)]*)\)" % qs, stderr)
    if not head or int(head.group(1)) != int(c.sum()):
        return False
    classes = [int(x) for x in re.findall(r"(\d+) (?:exact|with)", head.group(2))]
    got = [(int(a), int(b)) for a, b in re.findall(r"position is (\d+), (\d+) mismatches", stderr)]
    return classes == c.tolist() and got == list(zip(p.tolist(), m.tolist()))[:headn]


def batch_file(path, pats):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", pats.shape[1], pats.shape[0]))
        f.write(bytes(ord("ACGT"[c]) for c in pats.reshape(-1)))


def test_exact_build_then_queries_with_one_mismatch(tmp_path):
    S = text()
    fa = str(tmp_path / "t.fa")
    write_fasta(fa, S)
    r = run("fmindex_build", "--exact", fa)
    assert r.returncode == 0, r.stderr
    exact_fmi = open(fa + ".fmi", "rb").read()
    for q in (S[1000:1020].copy(), S[21_000:21_030].copy(), S[40_000:40_012].copy()):
        q[5] = (q[5] + 1) & 3
        r = run("fmindex_query", fa, "--mismatches", "1", "-n", "7", "-q", "".join("ACGT"[x] for x in q))
        assert r.returncode == 0, r.stderr
        assert single_query_matches(S, q, 1, r.stderr, 7), r.stderr
    pats = mm.patterns_for(S, 300, 24, 1, 2) & 3
    pf = str(tmp_path / "p.bin")
    batch_file(pf, pats)
    r = run("fmindex_query", fa, "--mismatches", "1", "-b", pf)
    assert r.returncode == 0, r.stderr
    counts, pos, _, _ = mm.brute_batch(S, pats, 1)
    assert "matched locations with 0 mismatches: %d\n" % counts[:, 0].sum() in r.stderr
    assert "matched locations with 1 mismatches: %d\n" % counts[:, 1].sum() in r.stderr
    assert "number of matched locations: %d\n" % counts.sum() in r.stderr
    assert "location checksum: %d\n" % pos.sum() in r.stderr
    # --mismatches 0 on the exact index is the plain query
    a = run("fmindex_query", fa, "--mismatches", "0", "-b", pf)
    b = run("fmindex_query", fa, "-b", pf)
    pick = lambda s: [ln for ln in s.splitlines() if "number of matched" in ln or "checksum" in ln]  # noqa: E731
    assert a.returncode == 0 and b.returncode == 0 and pick(a.stderr) == pick(b.stderr)
    # the same queries on the default (k = 32) index: correct, or the named error -- nothing else
    r = run("fmindex_build", fa)
    assert r.returncode == 0, r.stderr
    assert len(open(fa + ".fmi", "rb").read()) == len(exact_fmi)  # the same layout
    for q in (S[1000:1020].copy(), S[21_000:21_030].copy()):
        q[5] = (q[5] + 1) & 3
        r = run("fmindex_query", fa, "--mismatches", "1", "-n", "7", "-q", "".join("ACGT"[x] for x in q))
        if r.returncode == 0:
            assert single_query_matches(S, q, 1, r.stderr, 7), r.stderr
        else:
            assert NAMED_ERROR in r.stderr
    assert run("fmindex_query", fa, "--mismatches", "4", "-q", "ACGT").returncode != 0
    assert "--exact" in run("-h").stderr and "--mismatches" in run("-h").stderr
