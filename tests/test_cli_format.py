"""What `kiss fmindex_query --seeds ...` prints and parses, without a device: kiss_amd/csrc/host/cli_format.hpp compiled alone
(no libkiss_hip) into two small programs, with AddressSanitizer and UBSan, and their output against lines written out here by
the rules of the header's comments.  tests/cli_format_check.cpp makes the State by hand; where a case coincides with one of
tests/golden/cli_reads_recording.json (a proper pair: 99 / 147, `=`, the signed TLEN, YS, YT; an unmapped mate at its partner's
place; both mates unmapped: 77 / 141; mates on two records: RNEXT by name, TLEN 0) the fields agree with it."""
import os
import subprocess


from tests.test_lcp_model import FASTA_EDGE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, R = "ACGTACGTAC", "GTACGTACGT"  # the reads of the pairs, and their reverse complement


def program(tmp, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", ROOT, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe


def sam(*fields):
    return "\t".join(str(f) for f in fields)


PLAIN = ["0 + 2 20 3 7 9 11", "1 - 1 19 600",  # --seeds: read strand start len count pos...
         "0 + 50 2 0 60 100 161"] + ["%d %s 0 0 0 0 0 0" % v for v in ((1, "-"), (2, "+"), (2, "+"), (2, "+"), (2, "-"))] + [  # --chain
         "0 + 12 0 12 10 22 0 12M", "1 - 6 2 12 120 129 2 2S5M1I4M3S", "2 + 7 3 10 40 47 0 3S7M", "2 + 6 0 6 140 146 0 6M4S",  # --align
         "2 + 5 0 7 200 208 1 4M1D3M3S", "2 - 0 0 0 0 0 0 *"]
HEADER = ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chrA\tLN:100", "@SQ\tSN:chrB\tLN:150", "@PG\tID:kiss\tPN:kiss\tVN:X"]


def single(a, b, at):
    """the lines of the four reads; a, b: the names of the records; at: where they start in the text"""
    return [sam("r0", 0, a, 11 - at[0], 60, "12M", "*", 0, 0, "ACGTACGTACGT", "*", "NM:i:0", "AS:i:12", "XS:i:0"),
            # reverse: 16, the SEQ reversed and complemented (N stays), clips on both sides, POS within the record, NM = 1 + 1
            sam("r1", 16, b, 121 - at[1], 37, "2S5M1I4M3S", "*", 0, 0, "GTACGTACGTNACGT", "*", "NM:i:2", "AS:i:6", "XS:i:3"),
            sam("r2", 0, a, 41 - at[0], 20, "3S7M", "*", 0, 0, "AACCGGTTAC", "*", "NM:i:0", "AS:i:7", "XS:i:6"),
            sam("r2", 256, b, 141 - at[1], 0, "6M4S", "*", 0, 0, "AACCGGTTAC", "*", "NM:i:0", "AS:i:6"),  # a secondary: no XS
            sam("r2", 2048 | 16, b, 201 - at[1], 11, "4M1D3M3S", "*", 0, 0, "GTAACCGGTT", "*", "NM:i:1", "AS:i:5", "XS:i:2"),
            sam("3", 4, "*", 0, 0, "*", "*", 0, 0, "ACGTACGTAN", "*")]


SINGLE = HEADER + single("chrA", "chrB", (0, 100)) + [HEADER[0], HEADER[3]] + single("*", "*", (0, 0))  # (the second time R == 0)
PAIRS = [  # proper: 1 + 2 + 32 + 64 and 1 + 2 + 16 + 128, the pair's MAPQ, TLEN with its sign, the mate's score
    sam("p0", 99, "chrA", 11, 40, "10M", "=", 51, 50, F, "*", "NM:i:0", "AS:i:10", "XS:i:0", "YS:i:10", "YT:Z:CP"),
    sam("p0", 147, "chrA", 51, 41, "10M", "=", 11, -50, R, "*", "NM:i:0", "AS:i:10", "XS:i:0", "YS:i:10", "YT:Z:CP"),
    # both start at the same base: mate 1 gets the positive TLEN
    sam("p1", 97, "chrA", 31, 12, "10M", "=", 31, 10, F, "*", "NM:i:0", "AS:i:10", "XS:i:1", "YS:i:10"),
    sam("p1", 145, "chrA", 31, 13, "10M", "=", 31, -10, R, "*", "NM:i:0", "AS:i:10", "XS:i:2", "YS:i:10"),
    # two records: RNEXT by name, TLEN 0
    sam("p2", 65, "chrA", 6, 60, "10M", "chrB", 101, 0, F, "*", "NM:i:0", "AS:i:10", "XS:i:0", "YS:i:10"),
    sam("p2", 129, "chrB", 101, 59, "10M", "chrA", 6, 0, F, "*", "NM:i:0", "AS:i:10", "XS:i:0", "YS:i:10"),
    # mate 2 does not map: mate 1 says so (8) and points at itself, mate 2 lies there (and says that mate 1 is reversed: 32)
    sam("p3", 1 | 8 | 16 | 64, "chrB", 11, 50, "10M", "=", 11, 0, R, "*", "NM:i:0", "AS:i:9", "XS:i:4"),
    sam("p3", 1 | 4 | 32 | 128, "chrB", 11, 0, "*", "=", 11, 0, F, "*"),
    sam("p4", 1 | 4 | 8 | 64, "*", 0, 0, "*", "*", 0, 0, F, "*"),
    sam("p4", 1 | 4 | 8 | 128, "*", 0, 0, "*", "*", 0, 0, F, "*"),
    # the pair chose the secondary of mate 1: written first, without 256 (and, not a head, without XS); the read's own primary
    # behind it is displaced: 256 and MAPQ 0, the mate fields, TLEN 0; mate 2 came from a rescue window: YR:i:1
    sam("p5", 99, "chrB", 61, 25, "10M", "=", 91, 40, F, "*", "NM:i:0", "AS:i:10", "YS:i:8", "YT:Z:CP"),
    sam("p5", 1 | 32 | 64 | 256, "chrA", 61, 0, "10M", "chrB", 91, 0, F, "*", "NM:i:0", "AS:i:10", "XS:i:10"),
    sam("p5", 147, "chrB", 91, 26, "10M", "=", 61, -40, R, "*", "NM:i:0", "AS:i:8", "XS:i:0", "YS:i:10", "YT:Z:CP", "YR:i:1")]


INFO = ["[info] reads: 4, seeds: 2, located seeds: 1, positions: 3", "[info] virtual reads: 8, anchors: 9, chains: 6, best score: 50",
        "[info] virtual reads: 8, chains: 6, aligned: 5, band too wide: 1, best score: 12"] + 2 * [
        "[info] reads: 4, alignments: 6, candidates: 5, spanning: 0, redundant: 0, hits: 5, heads: 4, mapped: 3, most candidates of a read: 3"] + [
        "[info] reads: 12, alignments: 10, candidates: 0, spanning: 0, redundant: 0, hits: 10, heads: 0, mapped: 0, most candidates of a read: 0",
        "[info] pairs: 6, eligible hits: 0, combinations: 0, concordant: 0, proper: 2, promoted: 1, lifted: 0, most combinations of a pair: 0",
        "[info] rescue: pairs planned: 4, anchors: 3, chains: 1, split: 0, empty: 0, bad input: 0, most chains of a pair: 1, rescued: 1"]


def test_lines_of_a_state_made_by_hand(tmp_path):
    r = subprocess.run([program(tmp_path, "cli_format_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n") == PLAIN + SINGLE + HEADER + PAIRS + [""]
    assert r.stderr.split("\n") == INFO + [""]


# the records of FASTA_EDGE_CASES, in its order (the last one is no FASTA file: one record named after the file)
RECORDS = [["h 0 15"], ["h 0 11"], ["a 0 2", "c 2 4"], ["a 0 2", "c 2 6"], ["h 0 4", "h2 4 8"], ["x.fa 0 10"]]
READS = (">first some words\r\nACGTN\r\n\r\nacgtRY\r\n>second\r\n\r\nGGCC\r\n>third\tx\r\nTTAA\r\n>\r\nA\r\n",
         ["first 01234", "1 012344", "2 2211", "third 3300", "4 0"])


def test_the_file_parsers(tmp_path):
    exe = program(tmp_path, "cli_parse_check")
    path = tmp_path / "x.fa"
    for (text, n), want in zip(FASTA_EDGE_CASES, RECORDS):
        path.write_bytes(text.encode())
        r = subprocess.run([exe, "records", str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.splitlines() == want, (text, r.stdout, r.stderr)
        assert int(want[-1].split()[2]) == n  # (the bases the device parser finds)
    path.write_bytes(b">only\n\n>h2 words\r\nAC\r\n")  # a record without bases is left out; '\r' is a base, and ends a name
    r = subprocess.run([exe, "records", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["h2 0 3"]
    path.write_bytes(READS[0].encode())
    r = subprocess.run([exe, "reads", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.splitlines() == READS[1], r.stdout
    r = subprocess.run([exe, "reads_unnamed", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["- " + ln.split()[1] for ln in READS[1]]
    assert subprocess.run([exe, "reads", str(tmp_path / "missing")], capture_output=True).returncode != 0
