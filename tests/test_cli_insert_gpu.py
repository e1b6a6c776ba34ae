"""`kiss fmindex_query ... --mates READS2 --sam --ins-auto` on the three-record FASTA of the paired SAM tests, with and without
--rescue: every field of every line against FMIndex.map_pairs(insert=..., bounds=...) on the same reads, the line on stderr
against the report; a library of 1400 .. 1600 bases whose lines carry FLAG 0x2 only with the option; the usage errors; `kiss -h`
is what it was and the options are documented by `kiss --help-pairs`."""
import json
import os
import re

import numpy as np
import pytest

from tests import test_cli_pairs_gpu, test_cli_rescue_gpu
from tests.test_cli_pairs_gpu import expected_lines
from tests.test_cli_rescue_gpu import aln_of_lines
from tests.test_cli_seeds_gpu import LETTERS, ROOT, run

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^\[insert\] pairs=(\d+) samples=(\d+) used=(\d+) q25=(\d+) q50=(\d+) q75=(\d+) mean=(\d+) sd=(\d+) ins_min=(\d+) "
                  r"ins_max=(\d+) applied=([01])$", re.M)
LINE_KEYS = ("P", "samples", "used", "q25", "q50", "q75", "mean", "sd", "ins_min", "ins_max")


def arr(letters):
    return np.array([LETTERS.get(c, 4) for c in letters], np.uint8)


def index_of(S):
    import kiss_amd
    import kiss_amd.fm_index as fm
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    return fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)


def body_of(r):
    return [ln.split("\t") for ln in r.stdout.splitlines() if not ln.startswith("@")]


def insert_line(r, res):
    """the one line on stderr: its numbers are the report's"""
    found = LINE.findall(r.stderr)
    assert len(found) == 1, r.stderr
    rep = res["insert"]["report"]
    assert [int(x) for x in found[0]] == [rep[k] for k in LINE_KEYS] + [1 if res["insert"]["applied"] else 0], (found, rep)


@pytest.mark.parametrize("rescue", (False, True))
def test_sam_with_ins_auto_equals_map_pairs_field_by_field(tmp_path, rescue):
    S, bounds, fa, (rf1, rf2), pairs = (test_cli_rescue_gpu if rescue else test_cli_pairs_gpu).make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", rf1, "--chain", "--align", "--sam", "--mates", rf2] + (["--rescue"] if rescue else [])
    f = index_of(S)
    m1, m2 = [arr(p[1]) for p in pairs], [arr(p[3]) for p in pairs]
    applied = []
    # too few pairs for the defaults: the values given are the fallback; then an estimate from the few there are
    for given_opts, auto_opts, insert, given in (
            (["--ins-max", "400"], [], "auto", dict(ins_max=400)),
            (["--ins-mean", "9"], ["--ins-auto-min-pairs", "1", "--ins-auto-min-mapq", "1", "--ins-auto-max", "3000"],
             dict(min_samples=1, min_mapq=1, max_insert=3000), dict(ins_mean=9))):
        r = run(*common, *given_opts, "--ins-auto", *auto_opts)
        assert r.returncode == 0, r.stderr
        res = f.map_pairs(m1, m2, S, bounds=bounds, rescue=True if rescue else None, insert=insert, **given)
        want = expected_lines(res, pairs, bounds)
        if rescue:
            CA = res["first_pass"]["alignments"]
            from_window = [a is not None and int(res["aln_source"][a]) >= CA for a in aln_of_lines(res, len(pairs))]
            want = [ln + (["YR:i:1"] if w else []) for ln, w in zip(want, from_window)]
        assert body_of(r) == want
        insert_line(r, res)
        applied.append(res["insert"]["applied"])
        if not res["insert"]["applied"]:  # stdout changes only through the pairing
            plain = run(*common, *given_opts)
            assert plain.returncode == 0 and plain.stdout == r.stdout and "[insert]" not in plain.stderr
    f.close()
    assert applied == [False, True]


def test_a_library_of_1500_bases_is_paired_only_with_ins_auto(tmp_path):
    from tests.test_fm_insert_gpu import insert_truth_case
    S, m1, m2, truth = insert_truth_case()
    fa = os.path.join(str(tmp_path), "one.fa")
    with open(fa, "w") as o:
        letters = "".join("ACGT"[c] for c in S)
        o.write(">chr1\n" + "".join(letters[at:at + 61] + "\n" for at in range(0, len(letters), 61)))
    files = []
    for which, mates in enumerate((m1, m2)):
        files.append(os.path.join(str(tmp_path), "lib%d.txt" % (which + 1)))
        with open(files[-1], "w") as o:
            o.write("".join("".join("ACGT"[c] for c in r) + "\n" for r in mates))
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", files[0], "--chain", "--align", "--sam", "--mates", files[1]]
    plain, auto = run(*common), run(*common, "--ins-auto")
    assert plain.returncode == 0 and auto.returncode == 0, auto.stderr
    assert "[insert]" not in plain.stderr
    for r, flag in ((plain, 0), (auto, 2)):
        body = body_of(r)
        assert len(body) == 400 and all(int(x[1]) & 2 == flag for x in body), [x[:9] for x in body if int(x[1]) & 2 != flag][:3]
    tlen = [abs(int(x[8])) for x in body_of(auto)]
    assert tlen[0::2] == tlen[1::2] == [t[1] for t in truth]
    found = LINE.findall(auto.stderr)
    assert len(found) == 1 and found[0][:2] == ("200", "200") and found[0][-1] == "1" and 1480 <= int(found[0][6]) <= 1520
    # explicit values next to --ins-auto are only the fallback
    both = run(*common, "--ins-auto", "--ins-max", "500", "--ins-mean", "300")
    assert both.returncode == 0 and both.stdout == auto.stdout
    few = run(*common, "--ins-auto", "--ins-auto-min-pairs", "201", "--ins-max", "3000", "--ins-mean", "1500")
    fallback = run(*common, "--ins-max", "3000", "--ins-mean", "1500")
    assert few.returncode == 0 and few.stdout == fallback.stdout and LINE.findall(few.stderr)[0][-1] == "0"
    assert all(int(x[1]) & 2 for x in body_of(few))


def test_usage_errors_and_the_help_pages(tmp_path):
    _, _, fa, (rf1, rf2), _ = test_cli_pairs_gpu.make_inputs(tmp_path)
    common = ["fmindex_query", fa, "--seeds", rf1, "--chain", "--align", "--sam"]
    r = run(*common, "--ins-auto")
    assert r.returncode != 0 and r.stdout == "" and "--ins-auto goes with --mates" in r.stderr
    for opt in ("--ins-auto-min-mapq", "--ins-auto-max", "--ins-auto-min-pairs"):
        r = run(*common, "--mates", rf2, opt, "30")
        assert r.returncode != 0 and r.stdout == "" and opt + " goes with --ins-auto" in r.stderr
    for value in ("0", "65536"):
        r = run(*common, "--mates", rf2, "--ins-auto", "--ins-auto-max", value)
        assert r.returncode != 0 and r.stdout == "" and "--ins-auto-max is in 1..65535" in r.stderr
    with open(os.path.join(ROOT, "tests", "golden", "cli_parse_recording.json")) as g:
        usage = json.load(g)["-h"]
    h = run("-h")
    assert (h.returncode, h.stdout, h.stderr) == (1, "", usage) and "--ins-auto" not in usage
    r = run("--help-pairs")
    assert r.returncode == 1 and r.stdout == ""
    for word in ("--ins-auto ", "--ins-auto-min-mapq NUM (=20)", "--ins-auto-max NUM (=10000)", "--ins-auto-min-pairs NUM (=25)", "[insert] pairs="):
        assert word in r.stderr, word
