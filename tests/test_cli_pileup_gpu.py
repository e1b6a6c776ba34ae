"""`kiss fmindex_query --seeds READS --chain --align --sam --pileup FILE` on the three-record FASTA of the SAM tests: the file
against lines made from FMIndex.map(pileup=True, bounds=...) / map_pairs(...) on the same reads and parameters -- single-end,
paired and with --rescue --, the file with --batch-reads byte for byte the one without, stdout byte for byte what it is
without the option, and the parser's answers."""
import json
import os

import numpy as np
import pytest

from tests.test_cli_pileup import lines_of
from tests.test_cli_sam_gpu import RECORDS, make_inputs, revcomp_str
from tests.test_cli_seeds_gpu import LETTERS, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [r[0] for r in RECORDS]


def codes(letters):
    return np.array([LETTERS.get(c, 4) for c in letters], np.uint8)


def mate_files(tmp, S):
    """ten pairs cut from the text (fragments of 300 .. 500 bases, one or two substitutions a mate), one whose second mate is
    junk, and two whose second mate has a substitution every 12th base: only the rescue finds those"""
    rng = np.random.default_rng(77)
    letters = lambda a: "".join("ACGT"[c] for c in a)  # noqa: E731
    m1, m2 = [], []
    for p in range(13):
        frag = int(rng.integers(300, 501))
        at = int(rng.integers(0, 5500)) + (0, 6000, 11003)[p % 3]
        a, b = S[at:at + 100].copy(), S[at + frag - 100:at + frag].copy()
        a[int(rng.integers(20, 80))] ^= 1
        b[int(rng.integers(20, 80))] ^= 2
        if p >= 11:
            for j in range(5, 100, 12):
                b[j] = (b[j] + 1 + rng.integers(0, 3)) & 3
        x, y = letters(a), revcomp_str(letters(b))
        if p == 10:
            y = letters(rng.integers(0, 4, 100))
        m1.append(y if p % 2 else x)
        m2.append(x if p % 2 else y)
    paths = [os.path.join(str(tmp), k) for k in ("m1.txt", "m2.txt")]
    for path, mates in zip(paths, (m1, m2)):
        with open(path, "w") as o:
            for p, r in enumerate(mates):
                o.write(">pair%d\n%s\n" % (p, r))
    return paths, [codes(r) for r in m1], [codes(r) for r in m2]


def test_the_pileup_file_on_the_command_line(tmp_path):
    import kiss_amd
    import kiss_amd.fm_index as fm
    S, bounds, fa, rf, reads = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    out = os.path.join(str(tmp_path), "pile.tsv")

    def pileup_file(*args, only=()):
        """-> the lines of the file (only: the options that go with --pileup); checked: stdout is what it is without --pileup"""
        if os.path.exists(out):
            os.remove(out)
        plain, r = run(*args), run(*args, "--pileup", out, *only)
        assert plain.returncode == 0 and r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout and "[info] pileup:" in r.stderr and "[info] pileup:" not in plain.stderr
        with open(out) as f:
            return f.read().splitlines()

    arrs = [codes(letters) for _, letters in reads]
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    try:
        # single-end
        common = ["fmindex_query", fa, "--seeds", rf, "--both-strands", "--chain", "--align", "--sam"]
        res = f.map(arrs, S, both_strands=True, bounds=bounds, pileup=True)
        want = lines_of(res["pileup"], S, NAMES, bounds)
        got = pileup_file(*common)
        assert got == want and len(want) > 1000 and res["pileup_report"]["alt_columns"] > 10
        assert {ln.split("\t")[0] for ln in got} == set(NAMES) and any(ln.startswith("chrA\t6000\t") for ln in got)  # (the end of a record)
        assert pileup_file(*common, "--batch-reads", "3") == got
        assert pileup_file(*common, "--md", "--sam-writer", "device") == got
        res = f.map(arrs, S, both_strands=True, bounds=bounds, pileup=dict(min_mapq=30))
        assert pileup_file(*common, only=("--pileup-min-mapq", "30")) == lines_of(res["pileup"], S, NAMES, bounds)
        # paired, and with --rescue
        (p1, p2), m1, m2 = mate_files(tmp_path, S)
        paired = ["fmindex_query", fa, "--seeds", p1, "--mates", p2, "--chain", "--align", "--sam"]
        res = f.map_pairs(m1, m2, S, bounds=bounds, pileup=True)
        want = lines_of(res["pileup"], S, NAMES, bounds)
        assert pileup_file(*paired) == want and res["pair_report"]["proper"] >= 4
        assert pileup_file(*paired, "--batch-reads", "3") == want
        rescued = f.map_pairs(m1, m2, S, bounds=bounds, rescue=True, pileup=True)
        want_rescued = lines_of(rescued["pileup"], S, NAMES, bounds)
        assert rescued["rescue"]["rescued"] >= 1 and want_rescued != want
        assert pileup_file(*paired, "--rescue") == want_rescued == pileup_file(*paired, "--rescue", "--batch-reads", "4")
        proper = f.map_pairs(m1, m2, S, bounds=bounds, rescue=True, pileup=dict(proper_only=1))
        assert pileup_file(*paired, "--rescue", only=("--pileup-proper",)) == lines_of(proper["pileup"], S, NAMES, bounds) != want_rescued
    finally:
        f.close()


def test_what_the_parser_says(tmp_path):
    S, bounds, fa, rf, reads = make_inputs(tmp_path)
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--pileup", os.path.join(str(tmp_path), "x"))
    assert r.returncode != 0 and "--pileup goes with --sam" in r.stderr and not os.path.exists(os.path.join(str(tmp_path), "x"))
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--sam", "--pileup-min-mapq", "3")
    assert r.returncode != 0 and "--pileup-min-mapq goes with --pileup" in r.stderr
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--sam", "--pileup", os.path.join(str(tmp_path), "x"), "--pileup-proper")
    assert r.returncode != 0 and "--pileup-proper goes with --mates" in r.stderr
    with open(os.path.join(ROOT, "tests", "golden", "cli_parse_recording.json")) as g:
        usage = json.load(g)["-h"]
    r = run("-h")
    assert [r.returncode, r.stdout, r.stderr] == [1, "", usage]
    r = run("--help-pileup")
    assert r.returncode == 1 and r.stdout == ""
    for word in ("--pileup FILE", "--pileup-min-mapq NUM (=0)", "--pileup-proper", "COV + DEL", "32 bytes"):
        assert word in r.stderr, word
    # a file that cannot be opened is said before a read is mapped
    assert run("fmindex_build", "--exact", fa).returncode == 0
    r = run("fmindex_query", fa, "--seeds", rf, "--both-strands", "--chain", "--align", "--sam", "--pileup", os.path.join(str(tmp_path), "no/such/dir/x"))
    assert r.returncode != 0 and "cannot open" in r.stderr and r.stdout == ""
