"""`kiss fmindex_query --seeds READS --chain` on a small FASTA built with `fmindex_build --exact`, against the chain model run
on the seed model's seeds; the usage errors; and `--seeds` alone, byte for byte the lines of
tests/golden/cli_seeds_before_chain_*.txt.  Those files were written from tests/test_cli_seeds_gpu.expected, the statement
the binary before --chain is tested against; a recording of the binary of commit a0b0b58 on these inputs
(tests.test_cli_chain_gpu.make_inputs gives the files) is byte for byte the same, so they stand as they are."""
import os

import numpy as np

from tests import fm_chain_model as cm
from tests import fm_seed_model as sm
from tests import gen
from tests.test_cli_gpu import write_fasta
from tests.test_cli_seeds_gpu import LETTERS, read_lines, run

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED_ARGS = {"default": [], "both": ["--both-strands", "--min-seed-len", "12", "--max-seed-len", "40", "--max-occ", "5"]}


def make_inputs(tmp):
    """the text (with a tandem array: many occurrences), its FASTA and the reads file -> S, lines, fasta path, reads path"""
    S = gen.iid(40_000, 31)
    S[20_000:20_600] = np.tile(np.array([0, 2, 3], np.uint8), 200)
    fa = os.path.join(str(tmp), "t.fa")
    write_fasta(fa, S)
    lines = read_lines(S)
    # three reads made of three pieces of the text each, a few bases apart (the last one runs into the tandem array): chains
    # of more than one anchor
    for p in (1000, 30_000, 19_930):
        lines.append("".join("ACGT"[c] for c in np.concatenate([S[p:p + 40], S[p + 43:p + 90], [(S[p + 90] + 1) & 3], S[p + 91:p + 140]])))
    rf = os.path.join(str(tmp), "reads.txt")
    with open(rf, "w") as o:
        o.write(">a header line\n" + "\n".join(lines[:5]) + "\n\n>another\n" + "\n".join(lines[5:]) + "\n")
    return S, lines, fa, rf


def expected(S, lines, both, min_len, max_len, max_occ, **params):
    reads = [np.array([LETTERS.get(c, 4) for c in ln], np.uint8) for ln in lines]
    sd = sm.Batch(S, reads, both, max_len).seeds(min_len, max_occ)
    got = cm.chain(sd["start"], sd["len"], sd["seed_index"], sd["positions"], sd["pos_index"], **params)
    out = []
    for v in range(got["V"]):
        q, strand = (v // 2, "+-"[v & 1]) if both else (v, "+")
        for c in range(int(got["chain_index"][v]), int(got["chain_index"][v + 1])):
            out.append(" ".join(str(x) for x in [q, strand] + got["chains"][c].tolist()))
    return out


def test_chains_on_the_command_line(tmp_path):
    S, lines, fa, rf = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    r = run("fmindex_query", fa, "--seeds", rf, "--chain")
    assert r.returncode == 0, r.stderr
    want = expected(S, lines, False, 19, 0, 500)
    assert r.stdout.splitlines() == want
    assert len(want) >= 8 and any(int(ln.split()[3]) > 1 for ln in want)
    assert "chains: %d" % len(want) in r.stderr
    r = run("fmindex_query", fa, "--seeds", rf, "--both-strands", "--min-seed-len", "12", "--max-occ", "0", "--chain", "--max-gap", "100",
            "--band", "10", "--gap-cost", "7", "--max-lookback", "0", "--min-chain-score", "15")
    assert r.returncode == 0, r.stderr
    want = expected(S, lines, True, 12, 0, 0, max_gap=100, band=10, gap_cost=7, max_lookback=0, min_score=15)
    assert r.stdout.splitlines() == want
    assert any(ln.split()[1] == "-" for ln in want) and len(want) > 100  # (the tandem array)
    # the usage errors
    for opt in ("--max-gap", "--band", "--gap-cost", "--max-lookback", "--min-chain-score"):
        r = run("fmindex_query", fa, "--seeds", rf, opt, "3")
        assert r.returncode != 0 and r.stdout == "" and "goes with --chain" in r.stderr
    r = run("fmindex_query", fa, "--chain", "-q", "ACGT")
    assert r.returncode != 0 and r.stdout == "" and "--chain goes with --seeds" in r.stderr
    assert run("fmindex_query", fa, "--seeds", rf, "--chain", "--gap-cost", "65536").returncode != 0
    assert "--chain" in run("-h").stderr and "--min-chain-score" in run("-h").stderr


@pytest.mark.parametrize("which", sorted(SEED_ARGS))
def test_seeds_alone_print_what_they_printed_before(tmp_path, which):
    S, lines, fa, rf = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    r = run("fmindex_query", fa, "--seeds", rf, *SEED_ARGS[which])
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "cli_seeds_before_chain_%s.txt" % which), "rb") as g:
        assert r.stdout.encode() == g.read()
