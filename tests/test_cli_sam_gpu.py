"""`kiss fmindex_query --seeds READS --chain --align --sam` on a three-record FASTA built with `fmindex_build --exact`: the
header, every alignment line against FMIndex.map(bounds=...) on the same reads and parameters, the record boundary, the
unmapped reads, and the output without --sam, which stays what it was."""
import os
import re

import numpy as np
import pytest

from tests import gen
from tests.test_cli_seeds_gpu import LETTERS, run

pytestmark = pytest.mark.gpu

RECORDS = (("chrA", "first record", 6000), ("chrB", "", 5003), ("chrC", "the\tlast", 7010))


def revcomp_str(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


def make_inputs(tmp):
    """-> S, bounds, fasta path, reads path, [(name, letters)]"""
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
    rng = np.random.default_rng(6)

    def cut(p, L, subs=2):
        R = S[p:p + L].copy()
        for j in rng.choice(np.arange(20, L - 20), subs, replace=False):  # (not where an end would rather be clipped)
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        return "".join("ACGT"[c] for c in R)

    reads = [("r0", cut(100, 150)), (None, revcomp_str(cut(6100, 150))), ("r2/1", cut(11003, 150)),      # 100 into B, the start of C
             (None, cut(5850, 150)),                                                                    # ends with chrA
             ("across", cut(5925, 150, 0)),                                                             # 75 bases of A, 75 of B
             ("junk", "".join("ACGT"[c] for c in rng.integers(0, 4, 120))),                             # maps nowhere
             (None, cut(12000, 70) + "N" + cut(12071, 79)),
             ("chimera", cut(3000, 80, 1) + revcomp_str(cut(15000, 90, 1))),                            # two heads
             ("clipped", "ACGTTGCA" * 3 + cut(8000, 100, 1)), (None, "NNNNNNNN")]
    rf = os.path.join(str(tmp), "reads.txt")
    with open(rf, "w") as o:
        for name, letters in reads:
            if name:
                o.write(">" + name + " some words\n")
            else:
                o.write("\n")
            o.write(letters + "\n")
    return S, bounds, fa, rf, reads


def cigar_len(cigar, ops):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in ops)


def test_sam_on_the_command_line(tmp_path):
    import kiss_amd
    import kiss_amd.fm_index as fm
    from kiss_amd.fm_align import cigar_string
    S, bounds, fa, rf, reads = make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", rf, "--both-strands", "--chain", "--align"]
    r = run(*common, "--sam")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    header = [ln for ln in lines if ln.startswith("@")]
    body = [ln for ln in lines if not ln.startswith("@")]
    assert header[0] == "@HD\tVN:1.6\tSO:unsorted"
    assert header[1:4] == ["@SQ\tSN:%s\tLN:%d" % (name, n) for name, _, n in RECORDS]
    assert len(header) == 5 and header[4].startswith("@PG\tID:kiss") and lines[:5] == header

    # the same reads through FMIndex.map
    arrs = [np.array([LETTERS.get(c, 4) for c in letters], np.uint8) for _, letters in reads]
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    res = f.map(arrs, S, both_strands=True, bounds=bounds)
    f.close()
    want = []
    for q, (name, letters) in enumerate(reads):
        qname = name if name else str(q)
        mine = res["hits"][int(res["hit_index"][q]):int(res["hit_index"][q + 1])]
        seq = "".join(c if c in "ACGT" else "N" for c in letters.upper())
        if len(mine) == 0:
            want.append("\t".join([qname, "4", "*", "0", "0", "*", "*", "0", "0", seq, "*"]))
        for h in mine:
            k = res["alignments"][int(h["aln"])]
            rev = bool(h["flags"] & 1)
            flag = (16 if rev else 0) | (256 if h["flags"] & 2 else 0) | (2048 if h["flags"] & 4 else 0)
            ops = res["cigar"][int(res["cigar_index"][h["aln"]]):int(res["cigar_index"][h["aln"] + 1])]
            L = len(letters)
            cigar = ("%dS" % k["rbeg"] if k["rbeg"] else "") + cigar_string(ops) + ("%dS" % (L - k["rend"]) if L > k["rend"] else "")
            fields = [qname, str(flag), RECORDS[int(h["ref"])][0], str(int(k["tbeg"]) - bounds[int(h["ref"])] + 1), str(int(h["mapq"])),
                      cigar, "*", "0", "0", revcomp_str(seq) if rev else seq, "*",
                      "NM:i:%d" % (int(k["mismatches"]) + int(k["ins"]) + int(k["del"])), "AS:i:%d" % int(h["score"])]
            if not h["flags"] & 2:
                fields.append("XS:i:%d" % int(h["sub"]))
            want.append("\t".join(fields))
    assert body == want
    by_name = {}
    for ln in body:
        by_name.setdefault(ln.split("\t")[0], []).append(ln.split("\t"))
    # every line has the eleven fields, and the CIGAR covers the SEQ
    for ln in body:
        f11 = ln.split("\t")
        assert len(f11) >= 11
        if f11[5] != "*":
            assert cigar_len(f11[5], "MIS") == len(f11[9])
    # where the reads were cut
    assert [x[1:4] for x in by_name["r0"]] == [["0", "chrA", "101"]] and by_name["r0"][0][4] == "60"
    assert [x[1:4] for x in by_name["1"]] == [["16", "chrB", "101"]]
    assert [x[1:4] for x in by_name["r2/1"]] == [["0", "chrC", "1"]]
    assert [x[1:4] for x in by_name["3"]] == [["0", "chrA", "5851"]]
    # no hit crosses a record boundary: the read cut across A | B aligns as one piece, which is spanning
    lengths = {name: n for name, _, n in RECORDS}
    for x in body:
        x = x.split("\t")
        if x[2] != "*":
            assert int(x[3]) - 1 + cigar_len(x[5], "MD") <= lengths[x[2]]
    assert [x[1:6] for x in by_name["across"]] == [["4", "*", "0", "0", "*"]]
    assert re.search(r"spanning: [1-9]", r.stderr)
    # the unmapped reads
    assert [x[1:6] for x in by_name["junk"]] == [["4", "*", "0", "0", "*"]] and by_name["junk"][0][9] == reads[5][1]
    assert [x[1:6] for x in by_name["9"]] == [["4", "*", "0", "0", "*"]] and by_name["9"][0][9] == "NNNNNNNN"
    # two heads on two strands, soft clips
    assert sorted(int(x[1]) for x in by_name["chimera"]) == [0, 2048 | 16] or sorted(int(x[1]) for x in by_name["chimera"]) == [16, 2048]
    assert re.match(r"2[0-4]S", by_name["clipped"][0][5]) and by_name["clipped"][0][2] == "chrB"
    assert "N" in by_name["6"][0][9]
    m = re.search(r"reads: (\d+), alignments: (\d+), candidates: (\d+), spanning: (\d+), redundant: (\d+), hits: (\d+), heads: (\d+), mapped: (\d+)",
                  r.stderr)
    rep = res["select_report"]
    assert m and [int(x) for x in m.groups()] == [rep[k] for k in ("Q", "alignments", "candidates", "spanning", "redundant", "hits",
                                                                  "heads", "mapped")]

    # the parameters reach the call
    r2 = run(*common, "--sam", "--min-map-score", "85", "--mapq-max", "33", "--mapq-coef", "40", "--max-hits", "1", "--overlap", "200")
    assert r2.returncode == 0, r2.stderr
    body2 = [ln.split("\t") for ln in r2.stdout.splitlines() if not ln.startswith("@")]
    assert len(body2) == len(reads) and [x[4] for x in body2 if x[0] == "r0"] == ["33"]
    assert [x[1] for x in body2 if x[0] == "chimera"] in (["0"], ["16"])

    # without --sam nothing changes: the nine columns of --align, from the model on the chains of --chain
    from tests.test_cli_align_gpu import expected
    chains = run(*common[:-1])
    plain = run(*common)
    assert chains.returncode == 0 and plain.returncode == 0, plain.stderr
    assert plain.stdout.splitlines() == expected(S, [letters for _, letters in reads], chains.stdout.splitlines(), True)
    assert "@HD" not in plain.stdout and "spanning" not in plain.stderr

    # the usage errors
    for opt in ("--min-map-score", "--overlap", "--mapq-coef", "--mapq-max", "--max-hits"):
        r = run(*common, opt, "3")
        assert r.returncode != 0 and r.stdout == "" and "goes with --sam" in r.stderr
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--sam")
    assert r.returncode != 0 and r.stdout == "" and "--sam goes with --align" in r.stderr
    assert run(*common, "--sam", "--overlap", "257").returncode != 0
    assert run(*common, "--sam", "--mapq-max", "256").returncode != 0
    assert "--sam" in run("-h").stderr and "--max-hits" in run("-h").stderr


def test_sam_of_a_plain_text_reference(tmp_path):
    """a file that does not begin with '>' is one record named after the file"""
    S = gen.iid(5000, 43)
    ref = os.path.join(str(tmp_path), "plain.txt")
    with open(ref, "w") as o:
        o.write("".join("ACGT"[c] for c in S[:2500]) + "\n" + "".join("ACGT"[c] for c in S[2500:]) + "\n")
    rf = os.path.join(str(tmp_path), "reads.txt")
    with open(rf, "w") as o:
        o.write("".join("ACGT"[c] for c in S[2450:2550]) + "\n")
    assert run("fmindex_build", "--exact", ref).returncode == 0
    r = run("fmindex_query", ref, "--seeds", rf, "--chain", "--align", "--sam")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[1] == "@SQ\tSN:plain.txt\tLN:5000" and len(lines) == 4
    assert lines[3].split("\t")[:6] == ["0", "0", "plain.txt", "2451", "60", "100M"]
