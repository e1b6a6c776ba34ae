"""The pileup file of `kiss fmindex_query ... --pileup FILE` without a device: kiss_amd/csrc/host/cli_pileup.hpp compiled alone
(no libkiss_hip) into a small program (tests/cli_pileup_check.cpp), with AddressSanitizer and UBSan, and its lines against lines
written out here, by the rule of the header's comment, from the planes of tests/fm_pileup_model.py: three records, counts on
both sides of a record boundary, positions that have an insertion behind them and nothing else, a text byte that is no base,
a count that wrapped, and a text without records."""
import os
import struct
import subprocess

import numpy as np

from tests import fm_pileup_model as pm
from tests.test_cli_format import program

M, I, D = 0, 1, 2


def lines_of(planes, text, names, bounds):
    """one line per position with COV + DEL + INS > 0: RNAME POS REF COV A C G T N DEL INS"""
    full = pm.base_counts(planes, text)
    out = []
    for j in range(len(text)):
        cov, dele, ins = (int(planes[k][j]) for k in (pm.COV, pm.DEL, pm.INS))
        if cov + dele + ins == 0:
            continue
        r = max(k for k in range(len(bounds) - 1) if bounds[k] <= j) if names else 0
        out.append("\t".join([names[r] if names else "*", str(j - (bounds[r] if names else 0) + 1), "ACGTN"[min(int(text[j]), 4)], str(cov)]
                             + [str(int(x)) for x in full[:, j]] + [str(dele), str(ins)]))
    return out


def printed(exe, path, planes, text, names, bounds):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(text), len(names)))
        for name in names:
            f.write(struct.pack("<Q", len(name)) + name.encode())
        f.write(np.asarray(bounds, np.uint64).tobytes() + np.asarray(text, np.uint8).tobytes() + np.ascontiguousarray(planes, np.uint32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout.splitlines()


def the_planes():
    """a text of three records (10, 6 and 14 bases; one byte is no base) under six reads"""
    text = np.array([0, 1, 2, 3] * 7 + [0, 1], np.uint8)
    text[9] = 4
    reads = [np.array(r, np.uint8) for r in (
        [0, 1, 2, 3, 0, 1, 2, 3],              # 8M at 4: over the boundary 10
        [2, 3, 0, 0, 0, 1, 2, 3],              # 2M 2I 4M at 6: an insertion behind position 7; the text byte 9, no base, under two bases
        [3, 3, 1, 2, 3, 0],                    # 2I 4M at 16: an insertion behind 15, the last position of record 2, which nothing covers
        [0, 4, 2, 3, 2, 3],                    # 4M 2D 2M at 20: a no-base, a deletion
        [1, 1, 1],                             # 3M at 27, up to the end of the text, every base differs or not
        [0, 1, 3, 3])]                         # 2M 2I at 0 ... an insertion behind position 1
    recs = [(0, 8, 4, 12), (0, 8, 6, 12), (0, 6, 16, 20), (0, 6, 20, 28), (0, 3, 27, 30), (0, 4, 0, 2)]
    ops = [[(M, 8)], [(M, 2), (I, 2), (M, 4)], [(I, 2), (M, 4)], [(M, 4), (D, 2), (M, 2)], [(M, 3)], [(M, 2), (I, 2)]]
    alns = np.zeros((6, 12), np.uint32)
    alns[:, 2:6] = recs
    words = np.array([(ln << 4) | op for o in ops for op, ln in o], np.uint32)
    oidx = np.concatenate([[0], np.cumsum([len(o) for o in ops])])
    want = pm.pileup(text, reads, alns, np.arange(7), words, oidx)
    assert want["bad"] == 0 and want["counted"] == 6 and want["insertions"] == 3
    return text, want["counts"]


def test_the_lines_of_three_records(tmp_path):
    exe = program(tmp_path, "cli_pileup_check")
    text, planes = the_planes()
    names, bounds = ["chrA", "b", "third record"], [0, 10, 16, 30]
    want = lines_of(planes, text, names, bounds)
    got = printed(exe, tmp_path / "a.bin", planes, text, names, bounds)
    assert got == want
    by_pos = {(f[0], int(f[1])): f for f in (ln.split("\t") for ln in got)}
    assert by_pos[("chrA", 10)][3] == "2" and by_pos[("b", 1)][3] == "2"           # both sides of a boundary
    assert by_pos[("b", 6)] == ["b", "6", "T", "0", "0", "0", "0", "0", "0", "0", "1"]  # an insertion behind it and nothing else
    assert by_pos[("chrA", 10)][2] == "N" and sum(int(x) for x in by_pos[("chrA", 10)][4:9]) == 2  # (a byte that equals no base)
    assert ("b", 5) not in by_pos and ("chrA", 3) not in by_pos                   # nothing there: no line
    assert by_pos[("third record", 6)][8] == "1"                                  # the no-base of read 3
    assert by_pos[("third record", 9)][9] == "1" and by_pos[("third record", 9)][3] == "0"  # deleted, not covered
    assert by_pos[("third record", 14)][1] == "14" and len(got) == len(want) > 20
    # without records: '*' and the position in the text
    assert printed(exe, tmp_path / "b.bin", planes, text, [], [0]) == lines_of(planes, text, [], [0])
    # counts modulo 2^32, as the planes hold them
    big = planes.copy()
    big[pm.COV, 5] = 7
    big[pm.ALT_C, 5] = 0xFFFFFFFF
    assert printed(exe, tmp_path / "c.bin", big, text, names, bounds) == lines_of(big, text, names, bounds)
    # no position at all
    assert printed(exe, tmp_path / "d.bin", np.zeros((8, 0), np.uint32), [], [], [0]) == []
    assert printed(exe, tmp_path / "e.bin", np.zeros((8, 30), np.uint32), text, names, bounds) == []


def test_the_cli_documents_the_option_and_keeps_its_help():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kiss = os.path.join(root, "kiss_amd", "kiss")
    r = subprocess.run([kiss, "--help-pileup"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    for word in ("--pileup FILE", "--pileup-min-mapq", "--pileup-proper", "RNAME POS REF COV A C G T N DEL INS"):
        assert word in r.stderr, word
    assert "pileup" not in subprocess.run([kiss, "-h"], capture_output=True, text=True).stderr
    r = subprocess.run([kiss, "fmindex_query", "--seeds", "r", "--chain", "--align", "--pileup", "x", "missing/x.fa"], capture_output=True, text=True)
    assert r.returncode != 0 and "--pileup goes with --sam" in r.stderr
    r = subprocess.run([kiss, "fmindex_query", "--seeds", "r", "--chain", "--align", "--sam", "--pileup", "x", "--pileup-min-mapq", "256", "missing/x.fa"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--pileup-min-mapq is at most 255" in r.stderr
