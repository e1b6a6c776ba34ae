"""tests/deflate_model.py, the DEFLATE encoder of kiss_hip_bgzf_deflate_* defined in Python (include/kiss_hip_deflate.h; DESIGN.md
4.23), held against zlib's inflate and Python's gzip before any device runs it: every stream decodes to its payload, the coding
written is the cheapest of the three exact costs, no block takes more than its payload + 31 bytes, incompressible data gives the
stored framing of tests/bam_model.py byte for byte, and over BAM records the bytes stay within 1.05 of zlib level 1."""
import gzip
import zlib

import numpy as np
import pytest

from tests import bam_model as B
from tests import deflate_cases as C
from tests import deflate_model as D


def check_payload(P, what):
    """one payload as one block -> its plan"""
    pl = D.plan(P)
    s = D.stream(P, pl)
    assert zlib.decompress(s, wbits=-15) == P, what
    assert pl["btype"] == min(pl["cost"], key=lambda b: (pl["cost"][b], b)) and len(s) == -(-pl["cost"][pl["btype"]] // 8), what
    blk = D.block(P, pl)
    assert len(blk) <= len(P) + 31 and gzip.decompress(blk) == P, what
    if pl["btype"] == 0:
        assert blk == B.frame(P, len(P)), what
    assert pl["literals"] + pl["match_bytes"] == len(P), what
    return pl


@pytest.fixture(scope="module")
def long_cases():
    return C.long_cases()


def test_every_length_up_to_300():
    for fill in ("zeros", "ff", "random", "text"):
        src = {"zeros": bytes(300), "ff": b"\xff" * 300, "random": C.RANDOM[7:307], "text": C.text()[5000:5300]}[fill]
        for n in range(1, 301):
            check_payload(src[:n], "%s, %d bytes" % (fill, n))
    assert D.frame(b"") == b"" and D.frame(b"", eof=True) == B.BGZF_EOF
    assert D.frame_report(b"", 7, True) == (B.BGZF_EOF, [0], dict(blocks=0, out_bytes=28, stored_blocks=0, fixed_blocks=0, dynamic_blocks=0,
                                                                 literals=0, matches=0, match_bytes=0))


@pytest.mark.parametrize("n", [65279, 65280, 65281, 65505])
def test_lengths_around_a_block(n):
    for fill, src in (("zeros", bytes(n)), ("random", C.RANDOM[:n]), ("period 256", C.period(256, n))):
        for bb in (0, 65505):
            got, index, rep = D.frame_report(src, bb, True)
            assert gzip.decompress(got) == src, (fill, n, bb)
            assert rep["blocks"] == -(-n // (bb or 65280)) == len(index) - 1 and index[-1] + 28 == len(got) == rep["out_bytes"]
            assert len(got) <= B.out_bytes(n, bb, True)
            if fill == "random":   # (the full blocks: a last block of one byte is shorter with the fixed codes)
                full = n // (bb or 65280)
                assert got[:index[full]] == B.frame(src[:full * (bb or 65280)], bb) and rep["stored_blocks"] >= full
                if n - full * (bb or 65280) in (0, 65279):
                    assert got == B.frame(src, bb, True)


def test_short_payloads_and_the_match_limits():
    plans = {k: check_payload(P, k) for k, P in C.short_cases().items()}
    assert sum(plans["one distance symbol"]["d"]) == 1 and plans["one distance symbol"]["d_lens"][0] == 1
    assert sum(plans["no distance symbol"]["d"]) == 0 and plans["no distance symbol"]["d_lens"] == [1] + [0] * 29
    for k in (2, 3, 255, 256, 257):
        assert plans["period %d" % k]["match_bytes"] > 1000 - k, k
    # a run of k: one literal, then matches at distance 1 of at most 258
    want = {257: [(256, 1)], 258: [(257, 1)], 259: [(258, 1)], 260: [(258, 1)], 516: [(258, 1), (257, 1)]}
    for k, runs in want.items():
        got = [t for t in plans["run of %d" % k]["tokens"] if isinstance(t, tuple)]
        assert got == runs, (k, got)


def test_a_literal_code_past_15_bits_takes_the_halving_rule():
    """the payload is deflate_cases.deep_tree: the shuffled Fibonacci counts (4180 bytes) are checked with the short payloads, but
    their frequent bytes repeat, the matches take most of them and the first construction is 10 deep (measured), so they cannot
    carry this assertion"""
    assert sorted(np.bincount(np.frombuffer(C.fibonacci(), np.uint8)).tolist())[:5] == [1, 1, 2, 3, 5] and len(C.fibonacci()) == 4180
    pl = check_payload(C.deep_tree(), "deep tree")
    assert pl["matches"] == 0 and pl["first_depth"] > 15 and max(pl["ll_lens"]) <= 15 and pl["btype"] == 2, (pl["first_depth"], pl["btype"])
    rounds = []
    D.huff_lengths(pl["ll"], 15, rounds)
    assert len(rounds) >= 2 and rounds[0] == pl["first_depth"] and rounds[-1] <= 15


def test_long_payloads_and_the_distance_limit(long_cases):
    plans = {k: check_payload(P[:65505], k) for k, P in long_cases.items()}
    far = lambda k: [t for t in plans[k]["tokens"] if isinstance(t, tuple) and t[1] > 1000]
    for d in (32767, 32768):   # (the match may begin in the zeros in front of the 64 bytes; zeros match zeros nearby)
        (n, dist), = far("repeat at %d" % d)
        assert dist == d and n >= 64   # (the zeros behind the 64 bytes repeat as well)
    assert far("repeat at 32769") == []
    assert plans["random"]["btype"] == 0 and plans["text"]["btype"] == 2
    for fill in ("zeros", "ff"):
        P = long_cases[fill][:65280].ljust(65280, long_cases[fill][:1])
        pl = D.plan(P)
        assert -(-pl["cost"][1] // 8) == 415 and pl["literals"] == 1 and pl["matches"] == 254   # 1 + 253 * 258 + 5 = 65280
        assert len(D.block(P, pl)) < 1024


def test_random_payloads_with_planted_repeats():
    rng = np.random.default_rng(4)
    kinds = set()
    for k in range(500):
        kinds.add(check_payload(C.planted(rng), "payload %d" % k)["btype"])
    assert kinds == {0, 1, 2}


@pytest.mark.parametrize("qualities", [True, False])
def test_bam_records_against_zlib_level_1(long_cases, qualities):
    data = long_cases["records with qualities" if qualities else "records without qualities"]
    ours = ref = 0
    for at in range(0, len(data), 65280):
        P = data[at:at + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(c.compress(P) + c.flush())
        ours += len(D.stream(P))
    print("qualities %s: %d bytes, model %d, zlib level 1 %d, ratio %.4f" % (qualities, len(data), ours, ref, ours / ref))
    assert gzip.decompress(D.frame(data, eof=True)) == data
    assert ours <= 1.05 * ref, (ours, ref)
