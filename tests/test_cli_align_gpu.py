"""`kiss fmindex_query --seeds READS --chain --align` on a small FASTA built with `fmindex_build --exact`: every line against
tests/fm_align_model.py run on the chains that `--chain` alone prints for the same input (the chaining has its own tests),
and the usage errors."""
import numpy as np
import pytest

from tests import fm_align_model as am
from tests.test_cli_chain_gpu import make_inputs
from tests.test_cli_seeds_gpu import LETTERS, run

pytestmark = pytest.mark.gpu


def expected(S, lines, chain_lines, both, **params):
    """the --align lines the model gives for the chains of the --chain lines"""
    reads = [np.array([LETTERS.get(c, 4) for c in ln], np.uint8) for ln in lines]
    out = []
    for ln in chain_lines:
        q, strand, _, _, rbeg, rend, tbeg, tend = ln.split()
        R = am.virtual_read(reads[int(q)], strand == "-")
        rec, ops = am.align_rows(S, R, int(rbeg), int(rend), int(tbeg), int(tend), **params)
        cigar = "*"
        if ops:
            cigar = ("%dS" % rec["rbeg"] if rec["rbeg"] else "") + am.cigar_string(ops) + ("%dS" % (R.size - rec["rend"]) if R.size > rec["rend"] else "")
        out.append(" ".join(str(x) for x in (q, strand, rec["score"], rec["rbeg"], rec["rend"], rec["tbeg"], rec["tend"],
                                             rec["mismatches"] + rec["ins"] + rec["del"], cigar)))
    assert both or all(ln.split()[1] == "+" for ln in chain_lines)
    return out


def test_alignments_on_the_command_line(tmp_path):
    S, lines, fa, rf = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    chains = run("fmindex_query", fa, "--seeds", rf, "--chain")
    assert chains.returncode == 0, chains.stderr
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--align")
    assert r.returncode == 0, r.stderr
    want = expected(S, lines, chains.stdout.splitlines(), False)
    assert r.stdout.splitlines() == want
    assert len(want) >= 8 and any("D" in ln.split()[8] for ln in want) and any("S" in ln.split()[8] for ln in want)
    assert "chains: %d" % len(want) in r.stderr and "aligned: %d" % len(want) in r.stderr
    seed_args = ["--both-strands", "--min-seed-len", "12", "--max-occ", "5", "--chain", "--min-chain-score", "15"]
    chains = run("fmindex_query", fa, "--seeds", rf, *seed_args)
    assert chains.returncode == 0, chains.stderr
    r = run("fmindex_query", fa, "--seeds", rf, *seed_args, "--align", "--match", "2", "--mismatch", "3", "--gap-open", "4",
            "--gap-extend", "2", "--align-band", "5")
    assert r.returncode == 0, r.stderr
    want = expected(S, lines, chains.stdout.splitlines(), True, match=2, mismatch=3, gap_open=4, gap_extend=2, band=5)
    assert r.stdout.splitlines() == want
    assert any(ln.split()[1] == "-" for ln in want)
    # the usage errors
    for opt in ("--match", "--mismatch", "--gap-open", "--gap-extend", "--align-band"):
        r = run("fmindex_query", fa, "--seeds", rf, opt, "3")
        assert r.returncode != 0 and r.stdout == "" and "goes with --chain" in r.stderr
        r = run("fmindex_query", fa, "--seeds", rf, "--chain", opt, "3")
        assert r.returncode != 0 and r.stdout == "" and "goes with --align" in r.stderr
    r = run("fmindex_query", fa, "--seeds", rf, "--align")
    assert r.returncode != 0 and r.stdout == "" and "--align goes with --chain" in r.stderr
    assert run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--match", "0").returncode != 0
    assert run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--gap-open", "65536").returncode != 0
    assert "--align" in run("-h").stderr and "--align-band" in run("-h").stderr
