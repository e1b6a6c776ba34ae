"""`kiss fmindex_query --seeds READS1 --mates READS2 --chain --align --sam --rescue` on a three-record FASTA: every field of
every line against what FMIndex.map_pairs(rescue=True, bounds=...) implies on the same reads, YR:i:1 included; the mates that
were damaged on purpose come back; without --rescue the output is what it was; and the option rules."""
import os

import numpy as np
import pytest

from tests import gen
from tests.test_cli_pairs_gpu import expected_lines
from tests.test_cli_sam_gpu import RECORDS, revcomp_str
from tests.test_cli_seeds_gpu import LETTERS, run

pytestmark = pytest.mark.gpu


def make_inputs(tmp):
    """-> S, bounds, fasta path, the two read files, [(name1, letters1, name2, letters2)]"""
    S = gen.iid(sum(r[2] for r in RECORDS), 41)
    bounds = [0]
    fa = os.path.join(str(tmp), "three.fa")
    with open(fa, "w") as o:
        for name, desc, n in RECORDS:
            o.write(">" + name + (" " + desc if desc else "") + "\n")
            piece = "".join("ACGT"[c] for c in S[bounds[-1]:bounds[-1] + n])
            for at in range(0, n, 61):
                o.write(piece[at:at + 61] + "\n")
            bounds.append(bounds[-1] + n)
    rng = np.random.default_rng(8)

    def cut(p, damaged=False, L=100):
        R = S[p:p + L].copy()
        if damaged:  # a substitution every 12th base: no exact match of 19 bases, so no seed
            for j in range(5, L, 12):
                R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        return "".join("ACGT"[c] for c in R)

    junk = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    pairs = [("r0", cut(3000), "r0", revcomp_str(cut(3250, True))),                 # the reverse mate damaged, chrA
             ("r1", revcomp_str(cut(7300)), "r1", cut(7000, True)),                 # the forward mate damaged and second, chrB
             ("ok", cut(12000), "ok", revcomp_str(cut(12280))),                     # proper as it is
             ("edge", cut(5800), "edge", revcomp_str(cut(5890, True))),             # the window is clipped at the end of chrA
             ("over", cut(5950, False, 50) + cut(6000, False, 50), "over", junk(100)),  # an anchor across two records is no hit
             ("junk", cut(15000), "junk", junk(100))]                               # mate 2 maps nowhere, rescue or not
    files = []
    for which in (0, 1):
        path = os.path.join(str(tmp), "reads%d.txt" % (which + 1))
        with open(path, "w") as o:
            for pr in pairs:
                o.write(">" + pr[2 * which] + "\n" + pr[2 * which + 1] + "\n")
        files.append(path)
    return S, bounds, fa, files, pairs


def aln_of_lines(res, npairs):
    """the alignment behind every line of the body, in the order the command line writes them (None: an unmapped mate)"""
    hits, hidx = res["hits"], res["hit_index"]
    out = []
    for p in range(npairs):
        chosen = [int(res["pairs"][p]["hit1"]), int(res["pairs"][p]["hit2"])]
        for m in (0, 1):
            q = 2 * p + m
            if chosen[m] == 0xFFFFFFFF:
                out.append(None)
                continue
            for h in [chosen[m]] + [h for h in range(int(hidx[q]), int(hidx[q + 1])) if h != chosen[m]]:
                out.append(int(hits[h]["aln"]))
    return out


def test_rescued_sam_on_the_command_line(tmp_path):
    import kiss_amd
    import kiss_amd.fm_index as fm
    S, bounds, fa, (rf1, rf2), pairs = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", rf1, "--chain", "--align", "--sam", "--mates", rf2, "--ins-max", "400"]
    r = run(*common, "--rescue")
    assert r.returncode == 0, r.stderr
    body = [ln.split("\t") for ln in r.stdout.splitlines() if not ln.startswith("@")]

    arr = lambda letters: np.array([LETTERS.get(c, 4) for c in letters], np.uint8)  # noqa: E731
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    m1, m2 = [arr(p[1]) for p in pairs], [arr(p[3]) for p in pairs]
    res = f.map_pairs(m1, m2, S, bounds=bounds, ins_max=400, rescue=True)
    want = expected_lines(res, pairs, bounds)
    CA = res["first_pass"]["alignments"]
    from_window = [a is not None and int(res["aln_source"][a]) >= CA for a in aln_of_lines(res, len(pairs))]
    assert len(from_window) == len(want)
    want = [ln + (["YR:i:1"] if w else []) for ln, w in zip(want, from_window)]
    assert body == want

    by_name = {}
    for x in body:
        by_name.setdefault(x[0], []).append(x)
    # the damaged mates are back, proper, at their places, and say where they come from; their partners do not
    a, b = by_name["r0"]
    assert a[1:4] == ["99", "chrA", "3001"] and b[1:4] == ["147", "chrA", "3251"] and b[8] == "-350" and b[-1] == "YR:i:1" and "YR:i:1" not in a
    a, b = by_name["r1"]
    assert a[1:4] == ["83", "chrB", str(7300 - 6000 + 1)] and b[1:4] == ["163", "chrB", "1001"] and b[-1] == "YR:i:1" and "YR:i:1" not in a
    a, b = by_name["edge"]
    assert int(a[1]) & 2 and b[2:4] == ["chrA", "5891"] and b[-1] == "YR:i:1"
    assert all("YR:i:1" not in x for x in by_name["ok"]) and [int(x[1]) & 2 for x in by_name["ok"]] == [2, 2]
    assert [int(x[1]) & 4 for x in by_name["junk"]] == [0, 4]
    assert res["rescue"]["rescued"] == 3 and res["pair_report"]["proper"] == 4 and res["first_pass"]["pair_report"]["proper"] == 1
    assert "rescue: pairs planned: %d," % res["rescue"]["report"]["pairs_planned"] in r.stderr and "rescued: 3" in r.stderr
    assert "chains: %d," % res["rescue"]["report"]["chains"] in r.stderr and "proper: 4," in r.stderr

    # the parameters reach the calls
    r2 = run(*common, "--rescue", "--rescue-anchors", "1", "--rescue-min-anchor-score", "101", "--rescue-width", "64")
    assert r2.returncode == 0, r2.stderr
    res2 = f.map_pairs(m1, m2, S, bounds=bounds, ins_max=400, rescue=dict(max_anchors=1, min_anchor_score=101, max_width=64))
    body2 = [ln.split("\t") for ln in r2.stdout.splitlines() if not ln.startswith("@")]
    CA2 = res2["first_pass"]["alignments"]
    w2 = [a is not None and int(res2["aln_source"][a]) >= CA2 for a in aln_of_lines(res2, len(pairs))]
    assert body2 == [ln + (["YR:i:1"] if w else []) for ln, w in zip(expected_lines(res2, pairs, bounds), w2)]
    assert res2["rescue"]["report"]["anchors"] == 0 and "rescued: 0" in r2.stderr  # (no hit scores above 100)
    r3 = run(*common, "--rescue", "--rescue-width", "64")
    assert r3.returncode == 0 and "rescued: 3" in r3.stderr and "split: " in r3.stderr and "split: 0," not in r3.stderr

    # without --rescue the output is what it was
    plain = run(*common)
    assert plain.returncode == 0 and "YR:i:" not in plain.stdout and "rescue" not in plain.stderr
    res0 = f.map_pairs(m1, m2, S, bounds=bounds, ins_max=400)
    f.close()
    assert [ln.split("\t") for ln in plain.stdout.splitlines() if not ln.startswith("@")] == expected_lines(res0, pairs, bounds)
    assert res0["pair_report"]["proper"] == 1


def test_usage_errors_of_rescue(tmp_path):
    S, bounds, fa, (rf1, rf2), pairs = make_inputs(tmp_path)
    common = ["fmindex_query", fa, "--seeds", rf1, "--chain", "--align", "--sam"]
    r = run(*common, "--rescue")
    assert r.returncode != 0 and r.stdout == "" and "--rescue goes with --mates" in r.stderr
    for opt in ("--rescue-anchors", "--rescue-min-anchor-score", "--rescue-width"):
        r = run(*common, "--mates", rf2, opt, "3")
        assert r.returncode != 0 and r.stdout == "" and "goes with --rescue" in r.stderr
    for opt, v in (("--rescue-anchors", "0"), ("--rescue-width", "0"), ("--rescue-width", "1025")):
        r = run(*common, "--mates", rf2, "--rescue", opt, v)
        assert r.returncode != 0 and r.stdout == "" and "--rescue-width in 1..1024" in r.stderr
    assert "--rescue-width" in run("-h").stderr and "YR:i:1" in run("-h").stderr
