"""`kiss fmindex_query ... --sam --md` on the three-record FASTA of the SAM tests, single-end, paired, with --rescue and from FASTQ:
the output with --md is the output without it once MD:Z:... is taken off each line; the tag sits directly behind NM:i:; its
value is the one FMIndex.map / map_pairs(want_md=True, bounds=...) gives for that hit; unmapped lines carry none; --md without
--sam is refused; `kiss -h` is what it was and --md is documented by `kiss --help-sam`."""
import json
import os
import re

import numpy as np
import pytest

from tests import fm_md_model as mm
from tests import test_cli_pairs_gpu, test_cli_rescue_gpu, test_cli_sam_gpu
from tests.test_cli_sam_gpu import RECORDS
from tests.test_cli_seeds_gpu import LETTERS, ROOT, run

pytestmark = pytest.mark.gpu
MD_TAG = re.compile(r"\tMD:Z:([^\t]*)")


def arr(letters):
    return np.array([LETTERS.get(c, 4) for c in letters], np.uint8)


def index_of(S):
    import kiss_amd
    import kiss_amd.fm_index as fm
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    return fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)


def with_and_without(common):
    """-> the body lines with --md; checked: without the tags they are the lines without --md, header and all"""
    plain, tagged = run(*common), run(*common, "--md")
    assert plain.returncode == 0 and tagged.returncode == 0, tagged.stderr
    assert "MD:Z:" not in plain.stdout
    assert MD_TAG.sub("", tagged.stdout) == plain.stdout
    body = [ln for ln in tagged.stdout.splitlines() if not ln.startswith("@")]
    mapped = 0
    for ln in body:
        f = ln.split("\t")
        tags = [t[:5] for t in f[11:]]
        if int(f[1]) & 4:
            assert "MD:Z:" not in tags, ln
            continue
        mapped += 1
        assert tags[:3] == ["NM:i:", "MD:Z:", "AS:i:"] and tags.count("MD:Z:") == 1, ln  # directly behind NM:i:
        md = f[12][5:]
        assert mm.MD_RE.match(md), ln
        # numbers + letters = the text the CIGAR covers; NM = letters + inserted bases
        on_text = sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", f[5]) if op in "MD")
        toks = mm.parse_md(md)
        letters = sum(len(t.lstrip("^")) for t in toks if isinstance(t, str))
        assert sum(t for t in toks if isinstance(t, int)) + letters == on_text, ln
        inserted = sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", f[5]) if op == "I")
        assert int(f[11][5:]) == letters + inserted, ln
    assert mapped > 0
    return body


def keyed(body, paired):
    """(QNAME, mate, strand, RNAME, POS, CIGAR, MD) of every mapped line, sorted"""
    out = []
    for ln in body:
        f = ln.split("\t")
        if not int(f[1]) & 4:
            out.append((f[0], (int(f[1]) >> 6) & 3 if paired else 0, bool(int(f[1]) & 16), f[2], int(f[3]), f[5], f[12][5:]))
    return sorted(out)


def keyed_from(res, names, lengths, bounds, paired):
    """the same from the arrays of map / map_pairs(want_md=True)"""
    from kiss_amd import md_strings
    from kiss_amd.fm_align import cigar_string
    strings = md_strings(res["md"], res["md_index"])
    assert len(strings) == res["hits"].size
    out = []
    for q in range(len(names)):
        for h in range(int(res["hit_index"][q]), int(res["hit_index"][q + 1])):
            hit = res["hits"][h]
            k = res["alignments"][int(hit["aln"])]
            ops = res["cigar"][int(res["cigar_index"][hit["aln"]]):int(res["cigar_index"][hit["aln"] + 1])]
            L = lengths[q]
            cigar = ("%dS" % k["rbeg"] if k["rbeg"] else "") + cigar_string(ops) + ("%dS" % (L - k["rend"]) if L > k["rend"] else "")
            out.append((names[q], 1 + (q & 1) if paired else 0, bool(hit["flags"] & 1), RECORDS[int(hit["ref"])][0],
                        int(k["tbeg"]) - bounds[int(hit["ref"])] + 1, cigar, strings[h]))
    return sorted(out)


def test_md_single_end_lines_and_fastq(tmp_path):
    from tests.test_cli_fastq_gpu import write_fastq
    S, bounds, fa, rf, reads = test_cli_sam_gpu.make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", rf, "--both-strands", "--chain", "--align", "--sam"]
    body = with_and_without(common)
    f = index_of(S)
    res = f.map([arr(letters) for _, letters in reads], S, both_strands=True, bounds=bounds, want_md=True)
    f.close()
    names = [name if name else str(q) for q, (name, _) in enumerate(reads)]
    want = keyed_from(res, names, [len(letters) for _, letters in reads], bounds, False)
    assert keyed(body, False) == want and len(want) >= 8
    assert any(re.search(r"[ACGT]", k[-1]) for k in want) and any(k[2] for k in want)  # mismatches; a reverse strand
    # the same reads from FASTQ: the same tags, line by line
    fq = os.path.join(str(tmp_path), "reads.fastq")
    write_fastq(fq, reads, 1)
    fq_body = with_and_without(["fmindex_query", fa, "--seeds", fq, "--both-strands", "--chain", "--align", "--sam"])
    assert [MD_TAG.findall(ln) for ln in fq_body] == [MD_TAG.findall(ln) for ln in body]


@pytest.mark.parametrize("rescue", (False, True))
def test_md_paired_with_and_without_rescue(tmp_path, rescue):
    # (the pairs of the rescue test have mates without a seed: lines from a window, YR:i:1)
    S, bounds, fa, (rf1, rf2), pairs = (test_cli_rescue_gpu if rescue else test_cli_pairs_gpu).make_inputs(tmp_path)
    assert run("fmindex_build", "--exact", fa).returncode == 0
    common = ["fmindex_query", fa, "--seeds", rf1, "--chain", "--align", "--sam", "--mates", rf2, "--ins-max", "400"] + (["--rescue"] if rescue else [])
    body = with_and_without(common)
    f = index_of(S)
    res = f.map_pairs([arr(p[1]) for p in pairs], [arr(p[3]) for p in pairs], S, bounds=bounds, ins_max=400, rescue=True if rescue else None,
                      want_md=True)
    f.close()
    names = [(pr[2 * m] or str(p)) for p, pr in enumerate(pairs) for m in (0, 1)]
    lengths = [len(pr[2 * m + 1]) for pr in pairs for m in (0, 1)]
    want = keyed_from(res, names, lengths, bounds, True)
    assert keyed(body, True) == want and len(want) >= len(pairs)
    if rescue:
        assert any("YR:i:1" in ln and "MD:Z:" in ln for ln in body)


def test_md_goes_with_sam_and_the_help_pages(tmp_path):
    _, _, fa, rf, _ = test_cli_sam_gpu.make_inputs(tmp_path)
    r = run("fmindex_query", fa, "--seeds", rf, "--chain", "--align", "--md")
    assert r.returncode != 0 and r.stdout == "" and "--md goes with --sam" in r.stderr
    with open(os.path.join(ROOT, "tests", "golden", "cli_parse_recording.json")) as g:
        usage = json.load(g)["-h"]
    h = run("-h")
    assert (h.returncode, h.stdout, h.stderr) == (1, "", usage) and "--md" not in usage
    r = run("--help-sam")
    assert r.returncode == 1 and r.stdout == "" and "--md" in r.stderr and "MD:Z:" in r.stderr and "NM:i:" in r.stderr
