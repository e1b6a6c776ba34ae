"""tests/fm_sam_model.py, the alignment lines of the SAM output defined in Python, held against the host writer: the line
functions of kiss_amd/csrc/host/cli_format.hpp, compiled alone with AddressSanitizer and UBSan into tests/cli_sam_check.cpp (as
tests/test_cli_format.py compiles its programs), print 500 random States byte for byte as the model does; the model also gives
the lines written out by hand in tests/test_cli_format.py for the two States of tests/cli_format_check.cpp, restated here as
arrays; and kiss_amd.sam_header gives the header lines of the same test.  No GPU needed."""
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import fm_sam_model as M
from tests.test_cli_format import HEADER, PAIRS, SINGLE, program

BATCHES = 500


def serialise(b):
    Q, C, H, R = len(b["read_index"]) - 1, len(b["alns"]), len(b["hits"]), len(b["ref_names"])
    u64 = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()  # noqa: E731
    u32 = lambda a: np.ascontiguousarray(a, np.int64).astype(np.uint32).tobytes()  # noqa: E731
    text = lambda s: struct.pack("<Q", len(s)) + bytes(s)  # noqa: E731
    out = [struct.pack("<9Q", b["pairs"] is not None, b["qual"] is not None, b["md"] is not None, b["source"] is not None, int(b["first_alns"]),
                       R, Q, C, H), u64(b["read_index"]), bytes(bytearray(b["reads"]))]
    if b["qual"] is not None:
        out.append(bytes(bytearray(b["qual"])))
    out += [text(n) for n in b["names"]]
    out += [u32(b["alns"]), u64(b["cigar_index"]), u32(b["cigar"]), u32(b["hits"]), u64(b["hit_index"])]
    if b["pairs"] is not None:
        out.append(u32(b["pairs"]))
    if b["source"] is not None:
        out.append(u32(b["source"]))
    if b["md"] is not None:
        out += [u64(b["md_index"]), bytes(bytearray(b["md"]))]
    out += [text(n) for n in b["ref_names"]]
    out.append(u64(b["bounds"]))
    return b"".join(out)


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(2024)
    return [M.random_batch(rng) for _ in range(BATCHES)]


def test_the_batches_cover_what_they_should(batches):
    kinds = {(b["pairs"] is not None, b["qual"] is not None, b["md"] is not None, len(b["ref_names"])) for b in batches}
    assert len(kinds) == 2 * 2 * 2 * 3
    assert any(b["source"] is not None for b in batches) and any(b["pairs"] is not None and b["source"] is None for b in batches)
    assert any(len(b["ref_names"]) == 3 and b["ref_names"][0] == b["ref_names"][2] for b in batches)
    flags, where, mates = set(), set(), set()
    for b in batches:
        flags |= {int(t[M.H_FLAGS]) for t in b["hits"]}
        for p, pr in enumerate(b["pairs"] if b["pairs"] is not None else []):
            mapped = []
            for i in (0, 1):
                hb, he, mine = int(b["hit_index"][2 * p + i]), int(b["hit_index"][2 * p + i + 1]), int(pr[i])
                mapped.append(mine != M.NONE)
                if mine != M.NONE and he - hb >= 3:
                    where.add("first" if mine == hb else "last" if mine == he - 1 else "middle")
            mates.add(tuple(mapped))
    assert flags == set(range(8)) and where == {"first", "middle", "last"}
    assert mates == {(True, True), (True, False), (False, True), (False, False)}
    assert not any(M.bad_reads(b) for b in batches)


def test_the_model_equals_the_host_writer_byte_for_byte(batches, tmp_path):
    exe = program(tmp_path, "cli_sam_check")
    path = tmp_path / "states.bin"
    path.write_bytes(struct.pack("<Q", len(batches)) + b"".join(serialise(b) for b in batches))
    r = subprocess.run([exe, str(path)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    out, at = r.stdout, 0
    for k, b in enumerate(batches):
        end = out.index(b"\n", at)
        size = int(out[at:end])
        got = out[end + 1:end + 1 + size]
        at = end + 1 + size
        assert M.sam_model(b)["sam"] == got, "batch %d" % k
    assert at == len(out)


def ops(*pairs):
    return [n << 4 | "MID".index(c) for n, c in pairs]


def codes(letters):
    return ["ACGT".index(c) if c in "ACGT" else 4 for c in letters]


def state(reads, names, alns, cigar, cigar_index, hits, hit_index, R):
    read_index = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([len(r) for r in reads], out=read_index[1:])
    return {"reads": np.array([c for r in reads for c in codes(r)], np.uint8), "read_index": read_index, "qual": None, "names": names,
            "alns": np.array(alns, np.int64), "cigar": np.array(cigar, np.uint32), "cigar_index": np.array(cigar_index, np.uint64),
            "hits": np.array(hits, np.int64), "hit_index": np.array(hit_index, np.uint64), "pairs": None, "source": None, "first_alns": 0,
            "md": None, "md_index": None, "ref_names": [b"chrA", b"chrB"][:R], "bounds": np.array([0, 100, 250][:R + 1], np.uint64)}


def test_the_model_gives_the_lines_written_by_hand():
    """the two States of tests/cli_format_check.cpp"""
    alns = [[12, 0, 0, 12, 10, 22, 12, 0, 0, 0, 0, 0], [6, 0, 2, 12, 120, 129, 8, 1, 1, 0, 1, 0], [7, 0, 3, 10, 40, 47, 7, 0, 0, 0, 0, 0],
            [6, 0, 0, 6, 140, 146, 6, 0, 0, 0, 0, 0], [5, 0, 0, 7, 200, 208, 7, 0, 0, 1, 1, 0], [0] * 12]
    cigar = ops((12, "M"), (5, "M"), (1, "I"), (4, "M"), (7, "M"), (6, "M"), (4, "M"), (1, "D"), (3, "M"))
    hits = [[0, 0, 60, 12, 0, 0, 0, 0], [1, M.REVERSE, 37, 6, 3, 0, 1, 1], [2, 0, 20, 7, 6, 1, 2, 0], [3, M.SECONDARY, 0, 6, 0, 0, 2, 1],
            [4, M.SUPPLEMENTARY | M.REVERSE, 11, 5, 2, 0, 4, 1]]
    reads = ["ACGTACGTACGT", "ACGTNACGTACGTAC", "AACCGGTTAC", "ACGTACGTAN"]
    got = []
    for R in (2, 0):
        s = state(reads, [b"r0", b"r1", b"r2", b"3"], alns, cigar, [0, 1, 4, 5, 6, 9, 9], hits, [0, 1, 2, 5, 5], R)
        got += (HEADER if R else [HEADER[0], HEADER[3]]) + [ln.decode() for ln in M.sam_model(s)["sam"].split(b"\n")[:-1]]
    assert got == SINGLE
    tbegs = [10, 50, 30, 30, 5, 200, 110, 60, 160, 190]
    p = state(["ACGTACGTAC"] * 12, [b"p%d" % (q // 2) for q in range(12)], [[10, 0, 0, 10, t, t + 10, 10, 0, 0, 0, 0, 0] for t in tbegs],
              ops(*[(10, "M")] * 10), list(range(11)),
              [[0, 0, 60, 10, 0, 0, 0, 0], [1, M.REVERSE, 60, 10, 0, 0, 1, 0], [2, 0, 30, 10, 1, 0, 2, 0], [3, M.REVERSE, 31, 10, 2, 0, 3, 0],
               [4, 0, 60, 10, 0, 0, 4, 0], [5, 0, 59, 10, 0, 0, 5, 1], [6, M.REVERSE, 50, 9, 4, 0, 6, 1], [7, 0, 3, 10, 10, 1, 7, 0],
               [8, M.SECONDARY, 0, 10, 0, 0, 7, 1], [9, M.REVERSE, 22, 8, 0, 0, 9, 1]], [0, 1, 2, 3, 4, 5, 6, 7, 7, 7, 7, 9, 10], 2)
    p["source"], p["first_alns"] = np.arange(10, dtype=np.uint32), 9
    p["pairs"] = np.array([[0, 1, M.PROPER, 50, 20, 0, 0, 40, 41, 1], [2, 3, 0, 10, 20, 0, 0, 12, 13, 0], [4, 5, 0, 0, 20, 0, 0, 60, 59, 0],
                           [6, M.NONE, 0, 0, 9, 0, 0, 50, 0, 0], [M.NONE, M.NONE, 0, 0, 0, 0, 0, 0, 0, 0], [8, 9, M.PROPER, 40, 18, 0, 0, 25, 26, 1]],
                          np.int64)
    assert [ln.decode() for ln in M.sam_model(p)["sam"].split(b"\n")[:-1]] == PAIRS


def test_properties_of_the_model(batches):
    for b in batches:
        m = M.sam_model(b)
        idx = m["line_index"]
        assert idx[0] == 0 and idx.size == len(m["lines"]) + 1 and int(idx[-1]) == len(m["sam"]) and np.all(idx[1:] > idx[:-1])
        assert m["read_line"][0] == 0 and int(m["read_line"][-1]) == len(m["lines"]) and np.all(np.diff(m["read_line"].astype(np.int64)) >= 1)
        for k, ln in enumerate(m["lines"]):
            assert ln == m["sam"][int(idx[k]):int(idx[k + 1])] and ln.endswith(b"\n") and ln.count(b"\n") == 1
            f = ln[:-1].split(b"\t")
            assert len(f) >= 11
            if f[5] != b"*":  # CIGAR: M + I + S add up to the length of SEQ
                assert sum(int(n) for n, c in re.findall(rb"(\d+)([MIDS])", f[5]) if c in b"MIS") == len(f[9])
            assert f[10] == b"*" or len(f[10]) == len(f[9])


def test_a_bad_read_of_every_kind_is_found():
    rng = np.random.default_rng(5)
    b = M.make_batch(rng, [20] * 6, [2] * 6, R=3, paired=True, chosen="first")
    assert M.bad_reads(b) == []

    def bad(change):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        change(c)
        return M.bad_reads(c)

    def set_hit(field, value):
        return lambda c: c["hits"].__setitem__((5, field), value)

    def set_aln(field, value):
        return lambda c: c["alns"].__setitem__((int(c["hits"][5][M.H_ALN]), field), value)

    assert bad(set_hit(M.H_ALN, 12)) == [2] and bad(set_hit(M.H_REF, 3)) == [2]
    assert bad(set_aln(M.A_REND, 21)) == [2] and bad(set_aln(M.A_RBEG, 21)) == [2]
    assert bad(lambda c: c["bounds"].__setitem__(int(c["hits"][5][M.H_REF]), int(c["alns"][int(c["hits"][5][M.H_ALN])][M.A_TBEG]) + 1)) != []
    assert bad(lambda c: c["pairs"].__setitem__((1, M.P_FLAGS), M.BAD_INPUT)) == [2, 3]
    assert bad(lambda c: c["pairs"].__setitem__((1, M.P_HIT1), 6)) == [2] and bad(lambda c: c["pairs"].__setitem__((1, M.P_HIT2), 4)) == [3]
    assert M.sam_model({**b, "pairs": np.where(np.arange(10) == 2, M.BAD_INPUT, b["pairs"])})["report"] == {"bad": 6, "first_bad": 0}


def test_sam_header_gives_the_header_lines_of_print_sam():
    import kiss_amd
    assert kiss_amd.sam_header(["chrA", b"chrB"], [0, 100, 250], "X").decode().split("\n") == HEADER + [""]
    assert kiss_amd.sam_header(None, None, "X").decode().split("\n") == [HEADER[0], HEADER[3], ""]
    assert kiss_amd.sam_header([], [0], b"X") == kiss_amd.sam_header(None, None, "X")
    with pytest.raises(ValueError):
        kiss_amd.sam_header(["chrA"], [0, 1, 2], "X")
