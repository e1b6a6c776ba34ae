"""`kiss fmindex_query --seeds READS` on a small FASTA built with `fmindex_build --exact`, against the text itself
(tests/fm_seed_model.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import fm_seed_model as sm
from tests import gen
from tests.test_cli_gpu import write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")
LETTERS = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


def run(*args):
    return subprocess.run([KISS] + list(args), capture_output=True, text=True)


def read_lines(S):
    """reads as the lines of the file: cut from the text, with substitutions, with N and other letters, lower case, short"""
    rng = np.random.default_rng(3)
    lines = []
    for L in (150, 64, 33, 250):
        p = int(rng.integers(0, S.size - L))
        s = "".join("ACGT"[c] for c in S[p:p + L])
        lines.append(s)
        lines.append(s[:L // 2] + "N" + s[L // 2 + 1:])
        lines.append(s[:L // 3].lower() + "R" + s[L // 3 + 1:-1] + "n")
        cut = S[p:p + L].copy()
        for _ in range(3):
            j = int(rng.integers(0, L))
            cut[j] = (cut[j] + 1) & 3
        rc = sm.revcomp(cut)
        lines.append("".join("ACGT"[c] for c in rc))
    lines += ["ACGTACGTACGTACGTACGTACGT", "NNNN", "A"]
    return lines


def expected(S, lines, both, min_len, max_len, max_occ):
    reads = [np.array([LETTERS.get(c, 4) for c in ln], np.uint8) for ln in lines]
    got = sm.Batch(S, reads, both, max_len).seeds(min_len, max_occ)
    out = []
    for v in range(len(got["seed_index"]) - 1):
        q, strand = (v // 2, "+-"[v & 1]) if both else (v, "+")
        for s in range(int(got["seed_index"][v]), int(got["seed_index"][v + 1])):
            pos = got["positions"][int(got["pos_index"][s]):int(got["pos_index"][s + 1])].tolist()
            out.append(" ".join(str(x) for x in [q, strand, int(got["start"][s]), int(got["len"][s]), int(got["count"][s])] + pos))
    return out


def test_seeds_on_the_command_line(tmp_path):
    S = gen.genome_like(60_000, 21)
    S[20_000:26_000] = np.tile(np.array([0, 2, 3], np.uint8), 2000)  # a tandem array: many occurrences
    fa = str(tmp_path / "t.fa")
    write_fasta(fa, S)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    lines = read_lines(S)
    rf = str(tmp_path / "reads.txt")
    with open(rf, "w") as o:
        o.write(">a header line\n" + "\n".join(lines[:5]) + "\n\n>another\n" + "\n".join(lines[5:]) + "\n")
    r = run("fmindex_query", fa, "--seeds", rf)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected(S, lines, False, 19, 0, 500)
    assert len(r.stdout.splitlines()) > len(lines) // 2
    r = run("fmindex_query", fa, "--seeds", rf, "--both-strands", "--min-seed-len", "12", "--max-seed-len", "40", "--max-occ", "5")
    assert r.returncode == 0, r.stderr
    want = expected(S, lines, True, 12, 40, 5)
    assert r.stdout.splitlines() == want
    assert any(ln.split()[1] == "-" for ln in want) and any(len(ln.split()) == 5 for ln in want)
    # another sampling interval
    assert run("fmindex_build", "--exact", "--sa-intv", "7", fa).returncode == 0
    r = run("fmindex_query", fa, "--sa-intv", "7", "--seeds", rf, "--min-seed-len", "1", "--max-occ", "0", "--both-strands")
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == expected(S, lines, True, 1, 0, 0)
    # refused combinations
    pf = str(tmp_path / "p.bin")
    open(pf, "wb").write(b"\x04\x00\x00\x00\x01\x00\x00\x00ACGT")
    for extra in (["-q", "ACGT"], ["-b", pf], ["--mismatches", "1"], ["-g"]):
        r = run("fmindex_query", fa, "--sa-intv", "7", "--seeds", rf, *extra)
        assert r.returncode != 0 and r.stdout == "", extra
    assert run("fmindex_query", fa, "--sa-intv", "7", "--max-occ", "5", "-q", "ACGT").returncode != 0  # goes with --seeds
    assert run("fmindex_query", fa, "--sa-intv", "7", "--seeds", rf, "--min-seed-len", "0").returncode != 0
    assert "--seeds" in run("-h").stderr and "--both-strands" in run("-h").stderr
    # the default (k = 32) index: the lines of the exact one, or the named error -- nothing else
    assert run("fmindex_build", fa).returncode == 0
    r = run("fmindex_query", fa, "--seeds", rf, "--max-seed-len", "32")
    if r.returncode == 0:
        assert r.stdout.splitlines() == expected(S, lines, False, 19, 32, 500)
    else:
        assert "the positions need an index built with fmindex_build --exact" in r.stderr
