"""tests/bam_model.py, the BAM output defined in Python (include/kiss_hip_bam.h), held against what it can be held
against without a GPU: the SAM model (decode(encode(batch)) is its lines, byte for byte), hand values of reg2bin and one
hand-worked record, Python's gzip for the framing, zlib.crc32 for the CRC in pieces, and the header of the command line
(kiss_amd/csrc/host/cli_bam.hpp compiled alone with AddressSanitizer and UBSan) against kiss_amd.bam_writer.bam_header."""
import gzip
import struct
import subprocess
import zlib

import numpy as np
import pytest

import kiss_amd.bam_writer as W
from tests import bam_model as B
from tests import fm_sam_model as S
from tests.test_cli_format import program

BATCHES = 500


def clamp_tlen(b):
    """a TLEN of 2^31 or more does not fit BAM's i32: the batch gets 2^31 - 1 (the wrap has a hand-worked record below)"""
    if b["pairs"] is not None:
        for pr in b["pairs"]:
            if int(pr[S.P_TLEN]) >= 1 << 31:
                pr[S.P_TLEN] = (1 << 31) - 1
    return b


@pytest.fixture(scope="module")
def batches():
    """500 random batches with records that BAM can hold; beside them the ones it cannot (a position of 2^31 or more: one
    record of nearly 2^32 bases), which the encoder must refuse"""
    rng = np.random.default_rng(2025)
    good, refused = [], []
    while len(good) < BATCHES:
        b = S.random_batch(rng)
        if not b["ref_names"]:
            continue
        (refused if B.bad_reads_first(b) else good).append(clamp_tlen(b))
    return good, refused


def test_decode_of_encode_is_the_sam_model(batches):
    good, refused = batches
    kinds = {(b["pairs"] is not None, b["qual"] is not None, b["md"] is not None, len(b["ref_names"])) for b in good}
    assert len(kinds) == 2 * 2 * 2 * 2
    unmapped = tags = 0
    for k, b in enumerate(good):
        got, want = B.bam_model(b), S.sam_model(b)
        assert [B.bam_to_sam(r, b["ref_names"]) for r in got["records"]] == want["lines"], k
        assert B.split_records(got["bam"]) == got["records"], k
        assert sum(struct.unpack_from("<i", r)[0] + 4 for r in got["records"]) == got["report"]["bam_bytes"] == len(got["bam"]), k
        assert np.array_equal(got["read_rec"], want["read_line"]) and got["report"]["records"] == want["report"]["lines"], k
        assert got["report"]["unmapped_records"] == want["report"]["unmapped_lines"] and got["report"]["bad"] == 0, k
        unmapped += got["report"]["unmapped_records"]
        tags += got["bam"].count(b"YTZCP\0") + got["bam"].count(b"YRC\1")
    assert unmapped > 100 and tags > 100
    # what is refused is refused for a position alone, and is valid SAM
    assert refused
    for b in refused:
        assert not S.bad_reads(b) and len(b["ref_names"]) == 1 and int(b["bounds"][1]) > 1 << 31
        rep = B.bam_model(b)["report"]
        assert rep["bad"] == len(B.bad_reads_first(b)) and rep["first_bad"] == B.bad_reads_first(b)[0]


def test_reg2bin_by_hand():
    assert B.reg2bin(0, 1) == 4681 and B.reg2bin(-1, 0) == 4680
    assert B.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585 + 0       # across 2^14: one level up, bin of 128 Kib
    assert B.reg2bin(1 << 14, (1 << 14) + 1) == 4682
    assert B.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73 and B.reg2bin(0, 1 << 29) == 0
    assert B.reg2bin((1 << 31) - 1, 1 << 31) == 4681 + (1 << 17) - 1  # (the caller reduces it to 16 bits)


def hand_batch(tlen):
    """one pair on record chrB (it starts at 1000): mate 1 forward at 1004 (POS 5), 2S3M1D1M, mate 2 reverse at 1103 (POS 104), 4M"""
    reads = np.array([0, 1, 2, 3, 4, 0, 3, 3, 2, 1], np.uint8)           # ACGTNA, TTGC
    return {"reads": reads, "read_index": np.array([0, 6, 10], np.uint64), "qual": np.frombuffer(b"!!#$%&IIHG", np.uint8).copy(),
            "names": [b"p", b"p"], "alns": np.array([[9, 0, 2, 6, 1004, 1009, 0, 1, 0, 1, 0, 0], [8, 1, 0, 4, 1103, 1107, 0, 0, 0, 0, 0, 0]], np.int64),
            "cigar": np.array([3 << 4, 1 << 4 | 2, 1 << 4, 4 << 4], np.uint32), "cigar_index": np.array([0, 3, 4], np.uint64),
            "hits": np.array([[0, 0, 50, 9, 2, 0, 0, 1], [1, 1, 40, 8, 0, 0, 0, 1]], np.int64), "hit_index": np.array([0, 1, 2], np.uint64),
            "pairs": np.array([[0, 1, 1, tlen, 0, 0, 0, 33, 44, 0]], np.int64), "source": None, "first_alns": 0,
            "md": np.frombuffer(b"3^A14", np.uint8).copy(), "md_index": np.array([0, 4, 5], np.uint64), "ref_names": [b"chrA", b"chrB"],
            "bounds": np.array([0, 1000, 3000], np.uint64)}


def test_one_record_by_hand_and_the_tlen_that_wraps():
    got = B.bam_model(hand_batch(103))
    first = (struct.pack("<iiBBHHHIiii", 1, 4, 2, 33, 4681, 4, 1 | 2 | 32 | 64, 6, 1, 103, 103) + b"p\0"
             + struct.pack("<4I", 2 << 4 | 4, 3 << 4, 1 << 4 | 2, 1 << 4) + bytes([0x12, 0x48, 0xF1]) + bytes([0, 0, 2, 3, 4, 5])
             + b"NMI" + struct.pack("<I", 2) + b"MDZ3^A1\0" + b"ASI" + struct.pack("<I", 9) + b"XSI" + struct.pack("<I", 2)
             + b"YSI" + struct.pack("<I", 8) + b"YTZCP\0")
    assert got["records"][0] == struct.pack("<i", len(first)) + first
    # the reverse mate: flag 1 | 2 | 16 | 128, SEQ the reverse complement of TTGC = GCAA, QUAL reversed, TLEN negative
    second = (struct.pack("<iiBBHHHIiii", 1, 103, 2, 44, 4681, 1, 1 | 2 | 16 | 128, 4, 1, 4, -103) + b"p\0" + struct.pack("<I", 4 << 4)
              + bytes([0x42, 0x11]) + bytes([x - 33 for x in b"GHII"]) + b"NMI" + struct.pack("<I", 0) + b"MDZ4\0" + b"ASI" + struct.pack("<I", 8)
              + b"XSI" + struct.pack("<I", 0) + b"YSI" + struct.pack("<I", 9) + b"YTZCP\0")
    assert got["records"][1] == struct.pack("<i", len(second)) + second
    assert [B.bam_to_sam(r, [b"chrA", b"chrB"]) for r in got["records"]] == S.sam_model(hand_batch(103))["lines"]
    # TLEN 2^32 - 5: SAM prints 4294967291 and -4294967291; BAM keeps the low 32 bits, which read -5 and 5
    wrap = B.bam_model(hand_batch((1 << 32) - 5))["records"]
    assert struct.unpack_from("<i", wrap[0], 32)[0] == -5 and struct.unpack_from("<i", wrap[1], 32)[0] == 5
    assert wrap[0][:32] == got["records"][0][:32] and wrap[0][36:] == got["records"][0][36:]


def test_what_bam_cannot_hold_is_bad():
    b = hand_batch(103)
    b["names"] = [b"p", b""]
    assert B.bam_model(b)["report"] == {"bad": 1, "first_bad": 1}
    b["names"] = [b"x" * 255, b"y" * 254]
    assert B.bam_model(b)["report"] == {"bad": 1, "first_bad": 0}
    b = hand_batch(103)
    b["cigar"][3] = 4 << 4 | 3
    assert B.bam_model(b)["report"] == {"bad": 1, "first_bad": 1}
    b = hand_batch(103)
    b["bounds"] = np.array([0, 1000, 1 << 32], np.uint64)
    b["alns"][1][S.A_TBEG] = 1000 + (1 << 31)       # POS - 1 = 2^31 for mate 2, which is PNEXT - 1 of mate 1
    assert B.bam_model(b)["report"] == {"bad": 2, "first_bad": 0}
    b["alns"][1][S.A_TBEG] = 999 + (1 << 31)
    assert B.bam_model(b)["report"]["bad"] == 0


SIZES = (0, 1, 65279, 65280, 65281, 65505, 200000)
BLOCKS = (1, 7, 65280, 65505)


@pytest.mark.parametrize("eof", [False, True])
def test_the_framing_is_what_gzip_reads(eof):
    data = np.random.default_rng(5).integers(0, 256, max(SIZES), dtype=np.uint8).tobytes()
    for n in SIZES:
        for bb in BLOCKS:
            x = data[:n]
            framed = B.frame(x, bb, eof)
            assert len(framed) == B.out_bytes(n, bb, eof), (n, bb)
            if framed:
                assert gzip.decompress(framed) == x, (n, bb)
            assert framed.endswith(B.BGZF_EOF) == eof or not n
    assert B.frame(b"", 0, True) == B.BGZF_EOF == W.BGZF_EOF and len(B.BGZF_EOF) == 28 and gzip.decompress(B.BGZF_EOF) == b""
    assert B.frame(b"abc", 0) == B.frame(b"abc", 65280)


@pytest.mark.parametrize("piece", [1, 255, 1020, 1021])
def test_the_crc_in_pieces_is_zlibs(piece):
    rng = np.random.default_rng(piece)
    for lanes in (64, 256):
        for n in {piece * lanes, piece * lanes - 1, piece * (lanes - 1) + 1, max(1, piece * lanes - piece), piece}:
            if n > 65505 or -(-n // lanes) != piece and n != piece:
                continue
            for data in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), b"\0" * n, b"\xff" * n):
                assert B.crc32_pieces(data, lanes) == zlib.crc32(data), (lanes, n)
    assert B.crc_mul(0x80000000, 0x12345678) == 0x12345678 and B.crc_x8n(0) == 0x80000000 and B.crc_x8n(1) == 0x00800000
    x = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    assert B.frame(x, 7, True, crc=B.crc32_pieces) == B.frame(x, 7, True)


def test_the_header_of_the_command_line_is_bam_header(tmp_path):
    exe = program(tmp_path, "cli_bam_check")
    for names, bounds in (([b"chrA", b"chrB", b"c"], [0, 100, 250, 251]), ([b"one record"], [0, (1 << 31) - 1]), ([], [0])):
        want = W.bam_header(names, bounds, "X")
        assert want == B.bam_header(names, bounds, kiss_amd_sam_header(names, bounds))
        text = tmp_path / "text"
        text.write_bytes(kiss_amd_sam_header(names, bounds))
        got = subprocess.check_output([exe, str(text), str(len(names))] + [n.decode() for n in names] + [str(x) for x in bounds])
        assert got == want
        head, rest = B.skip_header(want + b"tail")
        assert head == want and rest == b"tail"
    with pytest.raises(ValueError):
        W.bam_header([b"long"], [0, 1 << 31], "X")
    text.write_bytes(b"")
    r = subprocess.run([exe, str(text), "1", "long", "0", str(1 << 31)], capture_output=True)
    assert r.returncode == 2 and b"2^31" in r.stderr and not r.stdout


def kiss_amd_sam_header(names, bounds):
    from kiss_amd import sam_header
    return sam_header(names, bounds, "X")
