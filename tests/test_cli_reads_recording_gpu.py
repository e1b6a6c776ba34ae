"""`kiss fmindex_query --seeds ...` against a recording: one command line per exit point of the read-mapping pipeline (seeds,
chains, alignments, SAM, paired SAM, paired SAM after --rescue) on the inputs of test_cli_chain_gpu, test_cli_sam_gpu,
test_cli_pairs_gpu and test_cli_rescue_gpu, and three command lines that fail.  stdout, the `[info] ` lines of stderr and the
exit status are compared byte for byte with tests/golden/cli_reads_recording.json, which `record()` below wrote from the binary
of commit a0b0b58 -- the last one whose command line was a chain of tail calls with two SAM writers -- and from no later one:
the file says what `kiss` printed before the pipeline was taken apart, so it is not made again from the code under test."""
import json
import os
import subprocess

import pytest

from tests import test_cli_chain_gpu, test_cli_pairs_gpu, test_cli_rescue_gpu, test_cli_sam_gpu
from tests.test_cli_seeds_gpu import KISS

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_reads_recording.json")
TMP_WORD = "TMP"  # stands for the temporary directory in what is compared
EXITS = (("seeds", []), ("seeds_both", ["--both-strands"]), ("chain", ["--chain"]), ("align", ["--chain", "--align"]),
         ("sam", ["--chain", "--align", "--sam", "--both-strands"]))


def command_lines(tmp):
    """writes the inputs under tmp -> ([fasta paths], {case: arguments})"""
    dirs = {k: os.path.join(str(tmp), k) for k in ("chain", "sam", "pairs", "rescue")}
    for d in dirs.values():
        os.mkdir(d)
    _, _, fa_c, rf_c = test_cli_chain_gpu.make_inputs(dirs["chain"])
    _, _, fa_s, rf_s, _ = test_cli_sam_gpu.make_inputs(dirs["sam"])
    _, _, fa_p, (p1, p2), pairs = test_cli_pairs_gpu.make_inputs(dirs["pairs"])
    _, _, fa_r, (r1, r2), _ = test_cli_rescue_gpu.make_inputs(dirs["rescue"])
    cases = {}
    for which, fa, rf, mates in (("chain", fa_c, rf_c, None), ("sam", fa_s, rf_s, None), ("pairs", fa_p, p1, [p2]),
                                 ("rescue", fa_r, r1, [r2, "--ins-max", "400"])):
        for name, opts in EXITS:
            cases[which + "-" + name] = ["fmindex_query", fa, "--seeds", rf] + opts
        if mates:
            cases[which + "-mates"] = cases[which + "-sam"] + ["--mates"] + mates
            cases[which + "-mates_rescue"] = cases[which + "-mates"] + ["--rescue"]
    short = os.path.join(dirs["pairs"], "short.txt")
    with open(short, "w") as o:
        o.write("\n".join(p[3] for p in pairs[:5]) + "\n")
    cases["fails-mates_without_sam"] = cases["pairs-align"] + ["--mates", p2]
    cases["fails-unequal_mate_files"] = cases["pairs-sam"] + ["--mates", short]
    cases["fails-no_reads_file"] = ["fmindex_query", fa_p, "--seeds", os.path.join(dirs["pairs"], "missing.txt"), "--chain"]
    return [fa_c, fa_s, fa_p, fa_r], cases


def run_case(kiss, args, tmp):
    """-> what is compared of one run; a run that fails also gives all of its stderr"""
    r = subprocess.run([kiss] + args, capture_output=True, text=True)
    assert r.returncode in (0, 1), (args, r.returncode, r.stderr)  # (anything else is a crash: nothing more is run)
    err = r.stderr.replace(str(tmp), TMP_WORD)
    got = {"status": r.returncode, "stdout": r.stdout.replace(str(tmp), TMP_WORD),
           "info": [ln for ln in err.splitlines() if ln.startswith("[info] ")]}
    if r.returncode != 0:
        got["stderr"] = err
    return got


def record(kiss, tmp):
    """every case with the binary `kiss` -> {case: {status, stdout, info[, stderr]}}"""
    fastas, cases = command_lines(tmp)
    for fa in fastas:
        assert subprocess.run([kiss, "fmindex_build", "--exact", fa]).returncode == 0
    return {case: run_case(kiss, args, tmp) for case, args in cases.items()}


with open(GOLDEN) as g:
    RECORDED = json.load(g)


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recording")
    fastas, cases = command_lines(tmp)
    for fa in fastas:
        assert subprocess.run([KISS, "fmindex_build", "--exact", fa]).returncode == 0
    return tmp, cases


def test_the_recording_has_every_case_and_no_other(indexed):
    assert sorted(RECORDED) == sorted(indexed[1]) and len(RECORDED) == 27
    assert all(RECORDED[c]["status"] == (1 if c.startswith("fails-") else 0) for c in RECORDED)
    assert all(RECORDED[c]["stdout"] == "" for c in RECORDED if c.startswith("fails-"))


@pytest.mark.parametrize("case", sorted(RECORDED))
def test_kiss_prints_what_it_printed(indexed, case):
    tmp, cases = indexed
    got = run_case(KISS, cases[case], tmp)
    assert got["status"] == RECORDED[case]["status"], got.get("stderr")
    assert got["stdout"] == RECORDED[case]["stdout"]
    assert got["info"] == RECORDED[case]["info"]
    assert got.get("stderr") == RECORDED[case].get("stderr")
