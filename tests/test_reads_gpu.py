"""The reads parser on the device (kiss_amd/csrc/reads.hip; include/kiss_hip_reads.h) against tests/reads_model.py: every output
array and every report field, for files of lines and FASTQ files, on arrays placed with tests/dev_place.py -- the raw bytes at an
odd address, every output at the least alignment its element allows, guard bytes around each --, the capacity protocol, the
caller's stream (the method of tests/test_dev_stream_gpu.py: a decoy input while the stream is held up), the interleave call in
both forms, and the Python entries down to FMIndex.map.  Every input is below 2 MB."""
import ctypes

import numpy as np
import pytest

from tests import dev_place, gen
from tests import reads_model as rm
from tests.test_fasta_gpu import SMALL
from tests.test_lcp_model import FASTA_EDGE_CASES
from tests.test_reads_model import fastq_bytes, random_files

pytestmark = pytest.mark.gpu
GUARD = 512
INIT = 0xEE  # what an output holds before the call (dev_place.place_out)
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 10000)
E_INVALID = -1
vp, u64 = ctypes.c_void_p, ctypes.c_uint64


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=1 << 23, device=0)  # (four times the largest file)
    yield c
    c.close()


def device():
    import torch
    return torch.device("cuda", 0)


class Call:
    """one kiss_hip_reads_parse_dev call on placed arrays: rc, the report and the bytes of every output"""

    def __init__(self, ctx, raw, fmt, bases_cap, reads_cap, want_qual=True, want_names=True, raw_lead=1, byte_lead=3, fill=0x5A, stream=None):
        from kiss_amd import _lib
        self.lib, dev = ctx._lib, device()
        self.raw = dev_place.place(np.frombuffer(raw, np.uint8), raw_lead, GUARD, fill, device=dev)
        self.outs = {"codes": dev_place.place_out(bases_cap, byte_lead, GUARD, fill, device=dev),
                     "read_index": dev_place.place_out(8 * (reads_cap + 1), 8, GUARD, fill, device=dev)}
        if want_qual:
            self.outs["qual"] = dev_place.place_out(bases_cap, 4 - byte_lead, GUARD, fill, device=dev)
        if want_names:
            self.outs["name_off"] = dev_place.place_out(8 * reads_cap, 8, GUARD, fill, device=dev)
            self.outs["name_len"] = dev_place.place_out(4 * reads_cap, 4, GUARD, fill, device=dev)
        self.rep = _lib.ReadsReport()
        self.args = (ctx, len(raw), {"auto": 0, "lines": 1, "fastq": 2}[fmt], bases_cap, reads_cap)
        self.run(stream)

    def address(self, name):
        return vp(self.outs[name].placement.address) if name in self.outs else None

    def run(self, stream=None):
        ctx, nbytes, fmt, bases_cap, reads_cap = self.args
        self.rc = self.lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(self.raw.placement.address), nbytes, fmt, self.address("codes"),
                                                    self.address("qual"), bases_cap, self.address("read_index"), self.address("name_off"),
                                                    self.address("name_len"), reads_cap, ctypes.byref(self.rep), stream)
        return self

    def fetch(self, name, dtype):
        """through kiss_hip_copy_to_host: a blocking copy on the null stream, no torch call"""
        out = np.empty(self.outs[name].numel(), np.uint8)
        if out.size:
            assert self.lib.kiss_hip_copy_to_host(vp(out.ctypes.data), self.address(name), out.size) == 0
        return out.view(dtype)

    def untouched(self):
        for name, view in self.outs.items():
            assert (self.fetch(name, np.uint8) == INIT).all(), name + " was written"
        dev_place.check_canaries(self.raw, *self.outs.values())


REPORT_FIELDS = ("lines", "reads", "bases", "no_base", "empty_reads", "first_empty", "bad_records", "first_bad", "first_bad_kind", "has_qual")
NONE = 0xFFFFFFFFFFFFFFFF


def check_report(rep, m):
    assert {1: "lines", 2: "fastq"}[rep.format] == m["format"]
    for k in REPORT_FIELDS:
        want = m[k]
        if want is None and k in ("first_empty", "first_bad"):
            want = NONE
        if want is not None:  # (with bad records only the bad_* fields, lines and the format are defined)
            assert getattr(rep, k) == want, (k, getattr(rep, k), want)


def check_call(c, m, what=""):
    """a call with room against the model m: everything, or with bad records the refusal"""
    check_report(c.rep, m)
    if m["bad_records"]:
        assert c.rc == E_INVALID, (what, c.rc)
        c.untouched()
        return
    assert c.rc == 0, (what, c.rc)
    Q, B = m["reads"], m["bases"]
    assert np.array_equal(c.fetch("read_index", np.uint64)[:Q + 1], m["read_index"]), what
    got = c.fetch("codes", np.uint8)
    assert np.array_equal(got[:B], m["codes"]), (what, "codes")
    assert (got[B:] == INIT).all()
    if "qual" in c.outs:
        got = c.fetch("qual", np.uint8)
        if m["qual"] is None:
            assert (got == INIT).all(), "a file of lines has no qualities"
        else:
            assert np.array_equal(got[:B], m["qual"]), (what, "qual")
            assert (got[B:] == INIT).all()
    if "name_off" in c.outs:
        off, ln = c.fetch("name_off", np.uint64), c.fetch("name_len", np.uint32)
        assert np.array_equal(ln[:Q], m["name_len"]), (what, "name_len")
        named = m["name_len"] > 0
        assert np.array_equal(off[:Q][named], m["name_off"][named]), (what, "name_off")
        assert (c.fetch("name_len", np.uint8)[4 * Q:] == INIT).all() and (c.fetch("name_off", np.uint8)[8 * Q:] == INIT).all()
    assert (c.fetch("read_index", np.uint8)[8 * (Q + 1):] == INIT).all()
    dev_place.check_canaries(c.raw, *c.outs.values())


def parse_and_check(ctx, raw, fmt, raw_lead=1, byte_lead=3, slack=0, **kw):
    m = rm.parse(raw, fmt)
    Q, B = (0, 0) if m["bad_records"] else (m["reads"], m["bases"])
    c = Call(ctx, raw, fmt, B + slack, Q + slack, raw_lead=raw_lead, byte_lead=byte_lead, **kw)
    check_call(c, m, (fmt, raw[:60]))
    return c, m


# ---- files of lines -------------------------------------------------------------------------------------------------------------
LINES_FILES = [t.encode() for t, _ in FASTA_EDGE_CASES] + list(SMALL) + random_files(60)


@pytest.mark.parametrize("raw_lead,byte_lead", [(1, 3), (3, 1), (0, 1)])
def test_lines_edge_cases(ctx, raw_lead, byte_lead):
    for raw in LINES_FILES:
        parse_and_check(ctx, raw, "lines", raw_lead, byte_lead)
        parse_and_check(ctx, raw, "auto", raw_lead, byte_lead, slack=5)


def test_lines_across_tiles(ctx):
    """reads and headers longer than a tile, '\\r\\n' ends, a header right in front of a tile boundary"""
    rng = np.random.default_rng(11)
    letters = lambda n: bytes(rng.choice(list(b"ACGTNacgt"), n).tolist())  # noqa: E731
    raw = b">long " + b"x" * 5000 + b"\r\n" + letters(9000) + b"\r\n\r\n" + letters(4090) + b"\n>n2\n" + letters(1) + b"\n" + letters(4096)
    for lead in (0, 1, 3):
        parse_and_check(ctx, raw, "lines", lead)
        parse_and_check(ctx, raw + b"\n", "lines", lead)


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------
def shaped_records(seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    recs = []
    for r, L in enumerate(lengths):
        seq = bytes(rng.choice(list(b"ACGTNacgtRY"), L).tolist())
        qual = bytes(rng.integers(33, 127, L).astype(np.uint8).tolist())
        recs.append(([b"r%d" % r, b"name%d\twith a tab" % r, b"", b"n%d words" % r][r % 4], seq, [b"", b"again"][r % 2], qual))
    return recs


@pytest.mark.parametrize("variant", ["lf", "crlf", "no_final_newline", "crlf_no_final_newline", "trailing_empty_lines", "zero_length_read"])
@pytest.mark.parametrize("raw_lead", [1, 3])
def test_fastq_shapes(ctx, variant, raw_lead):
    recs = shaped_records(5)
    if variant == "zero_length_read":
        recs.insert(3, (b"empty", b"", b"", b""))
    raw = fastq_bytes(recs, b"\r\n" if variant.startswith("crlf") else b"\n", last_eol="no_final" not in variant)
    if variant == "trailing_empty_lines":
        raw += b"\n\n\r\n"
    for fmt in ("fastq", "auto"):
        c, m = parse_and_check(ctx, raw, fmt, raw_lead, 4 - raw_lead)
    assert m["reads"] == len(recs) and m["bases"] == sum(LENGTHS) and m["no_base"] > 0
    assert (m["empty_reads"], m["first_empty"]) == ((1, 3) if variant == "zero_length_read" else (0, None))
    assert m["names"][1] == "name1" and m["names"][2] == "2"  # (a name ends at a tab; an empty name is the read's number)


def file_with_byte_at(which, at):
    """a FASTQ file whose byte `at` is the '@' of a record, the '+' of a record, or a '\\n'"""
    first = (b"pad", b"ACGTACGT" * 40, b"", b"I" * 320)
    second = (b"second", b"ACGTN" * 13, b"", b"#" * 65)
    head = len(fastq_bytes([first]))
    target = {"@": head, "+": head + len(b"@second\n") + 65 + 1, "\n": head - 1}[which]
    assert target < at
    first = (b"pad" + b"p" * (at - target),) + first[1:]
    raw = fastq_bytes([first, second] + shaped_records(9, (257, 1, 64)))
    assert raw[at:at + 1] == which.encode() and (which == "\n" or raw[at - 1:at] == b"\n")
    return raw


@pytest.mark.parametrize("raw_lead", [0, 1, 3])
def test_fastq_bytes_on_a_tile_boundary(ctx, raw_lead):
    """with the file at a multiple of 16 (lead 0) the tiles are cut at the file's bytes 4096, 8192, ...; at lead 1 and 3 they are cut
    1 and 3 bytes earlier, so the same nine files put other bytes on the boundary"""
    for which in ("\n", "@", "+"):
        for at in (4095, 4096, 4097):
            parse_and_check(ctx, file_with_byte_at(which, at), "fastq", raw_lead)


def test_fastq_no_record_and_one_record(ctx):
    for raw in (b"", b"\n", b"\r\n\n", b"@r\nA\n+\nI\n", b"@r\nA\n+\nI", b"@\n\n+\n\n@r\nAC\n+\n!!\n"):
        for fmt in ("fastq", "auto"):
            c, m = parse_and_check(ctx, raw, fmt, slack=2)
    assert m["reads"] == 2 and m["empty_reads"] == 1


def many_short_reads(count=20000):
    rng = np.random.default_rng(3)
    seq, qual = rng.choice(list(b"ACGTN"), count), rng.integers(33, 127, count)
    return b"".join(b"@%d\n%c\n+\n%c\n" % (r, int(seq[r]), int(qual[r])) for r in range(count))


def test_fastq_20000_reads_of_one_base(ctx):
    c, m = parse_and_check(ctx, many_short_reads(), "fastq")
    assert m["reads"] == m["bases"] == 20000


def test_fastq_one_long_read_beside_20000_short_ones(ctx):
    """the copy is parallel over the bytes of the file: the long read is the work of many lanes, and arrives whole"""
    rng = np.random.default_rng(4)
    long_read = (b"long", bytes(rng.choice(list(b"ACGT"), 300000).tolist()), b"", bytes(rng.integers(33, 127, 300000).astype(np.uint8).tolist()))
    short = many_short_reads()
    half = short.index(b"@10000\n")
    raw = short[:half] + fastq_bytes([long_read]) + short[half:]
    assert len(raw) < 2_000_000
    c, m = parse_and_check(ctx, raw, "auto")
    assert m["reads"] == 20001 and m["bases"] == 320000 and m["names"][10000] == "long"


def bad_file(kind, where):
    """records of 1500 bases, so that record 1 straddles the first tile boundary; `where`: record 0, the last one, or 1"""
    recs = shaped_records(21, (1500,) * 6)
    lines = fastq_bytes(recs).split(b"\n")[:-1]
    r = {"first": 0, "last": 5, "straddling": 1}[where]
    if kind == rm.BAD_NO_AT:
        lines[4 * r] = b">" + lines[4 * r][1:]
    elif kind == rm.BAD_NO_PLUS:
        lines[4 * r + 2] = b""
    elif kind == rm.BAD_LENGTHS:
        lines[4 * r + 3] = lines[4 * r + 3][:-1]
    else:
        lines = lines[:4 * r + 3]  # (a last record of three lines: r is the last one then)
    raw = b"\n".join(lines) + b"\n"
    if where == "straddling":
        start = len(b"\n".join(lines[:4])) + 1
        assert start < 4096 < start + len(b"\n".join(lines[4:8]))
    return raw, r


@pytest.mark.parametrize("where", ["first", "last", "straddling"])
@pytest.mark.parametrize("kind", [rm.BAD_NO_AT, rm.BAD_NO_PLUS, rm.BAD_LENGTHS, rm.BAD_TRUNCATED])
def test_fastq_bad_records(ctx, kind, where):
    raw, r = bad_file(kind, where)
    m = rm.parse(raw, "fastq")
    assert (m["bad_records"], m["first_bad"], m["first_bad_kind"]) == (1, r, kind)
    c = Call(ctx, raw, "fastq", 9000, 6)  # (room for everything: what refuses the call is the record)
    check_call(c, m)
    assert c.rep.bad_records == 1 and c.rep.first_bad == r and c.rep.first_bad_kind == kind
    # two bad records: the smaller index is reported, with its lowest kind
    if kind == rm.BAD_LENGTHS and where == "last":
        lines = raw.split(b"\n")
        lines[4] = b"x"
        lines[7] = b"I"
        m2 = rm.parse(b"\n".join(lines), "fastq")
        assert (m2["bad_records"], m2["first_bad"], m2["first_bad_kind"]) == (2, 1, rm.BAD_NO_AT)
        check_call(Call(ctx, b"\n".join(lines), "fastq", 9000, 6), m2)


# ---- the capacity protocol ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["lines", "fastq"])
def test_size_then_fill(ctx, fmt):
    recs = shaped_records(8, (1, 65, 300, 4097))
    raw = fastq_bytes(recs) if fmt == "fastq" else b"".join(b">" + n + b"\n" + s + b"\n" for n, s, _, _ in recs)
    m = rm.parse(raw, fmt)
    Q, B = m["reads"], m["bases"]
    assert Q == 4 and B == 1 + 65 + 300 + 4097
    for bases_cap, reads_cap in ((0, 0), (B - 1, Q), (B, Q - 1), (0, Q), (B, 0)):
        c = Call(ctx, raw, fmt, bases_cap, reads_cap)
        assert c.rc == E_INVALID and c.rep.bad_records == 0 and (c.rep.reads, c.rep.bases) == (Q, B), (bases_cap, reads_cap)
        c.untouched()
    check_call(Call(ctx, raw, fmt, B, Q), m, "exact")
    check_call(Call(ctx, raw, fmt, B + 77, Q + 5), m, "more than needed")
    # NULL for what is not wanted; NULL codes while there is no room for a base
    for want_qual, want_names in ((False, True), (True, False), (False, False)):
        check_call(Call(ctx, raw, fmt, B, Q, want_qual=want_qual, want_names=want_names), m, (want_qual, want_names))
    from kiss_amd import _lib
    rep = _lib.ReadsReport()
    d_raw = dev_place.place(np.frombuffer(raw, np.uint8), 1, GUARD, 0, device=device())
    d_idx = dev_place.place_out(8, 8, GUARD, 0, device=device())
    rc = ctx._lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.placement.address), len(raw), 0, None, None, 0, vp(d_idx.placement.address), None, None,
                                           0, ctypes.byref(rep), None)
    assert rc == E_INVALID and (rep.reads, rep.bases, rep.bad_records) == (Q, B, 0)
    dev_place.check_canaries(d_raw, d_idx)
    assert (dev_place.read_back(d_idx) == INIT).all()
    # refused before anything runs
    assert ctx._lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.placement.address), len(raw), 3, None, None, 0, vp(d_idx.placement.address), None, None,
                                             0, None, None) == E_INVALID
    assert ctx._lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.placement.address), len(raw), 0, None, None, 0, None, None, None, 0, None,
                                             None) == E_INVALID
    assert ctx._lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.placement.address), len(raw), 0, None, None, 0, vp(d_idx.placement.address),
                                             vp(d_idx.placement.address), None, 0, None, None) == E_INVALID
    assert ctx._lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.placement.address), 0xFFFFF001, 0, None, None, 0, vp(d_idx.placement.address), None,
                                             None, 0, None, None) == _lib.KISS_HIP_E_UNSUPPORTED
    import kiss_amd
    with kiss_amd.Context(max_n=1 << 20) as small:  # a ctx whose scratch does not scan that many bytes
        big = np.zeros(1_500_000, np.uint8) + 65
        c = Call(small, big.tobytes(), "lines", 0, 0)
        assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED
        c.untouched()


# ---- the caller's stream ----------------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(ctx):
    """tests/test_dev_stream_gpu.py's method: after a warm-up on the NULL stream the input is overwritten with a decoy (a valid file
    of the same shape, other letters, qualities and names); a delay and then the copy that puts the real file back are queued
    on s; the call is made with s while s is busy; on return the outputs are read by a blocking copy on the null stream."""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    recs = shaped_records(31, (150,) * 400 + (3000, 1))
    swap = bytes.maketrans(b"ACGTacgtNRY", b"CATGcatgRYN")
    decoy_recs = [(n.replace(b"r", b"q").replace(b"n", b"m"), s.translate(swap), p, bytes(33 + (c - 33 + 1) % 94 for c in q)) for n, s, p, q in recs]
    raw, decoy = fastq_bytes(recs), fastq_bytes(decoy_recs)
    m, md = rm.parse(raw, "auto"), rm.parse(decoy, "auto")
    assert len(raw) == len(decoy) and np.array_equal(m["read_index"], md["read_index"])
    assert (m["codes"] != md["codes"]).mean() > 0.7 and (m["qual"] != md["qual"]).all() and m["names"] != md["names"]
    s = caller_stream()
    c = Call(ctx, raw, "auto", m["bases"], m["reads"], raw_lead=1)
    for _ in range(2):  # 1. warm up on the NULL stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(None)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    check_call(c, m, "warm-up on the NULL stream")
    staging = c.raw.clone()
    c.raw.copy_(torch.from_numpy(np.frombuffer(decoy, np.uint8).copy()))  # 2. the decoy; the outputs as before any call
    for v in c.outs.values():
        v.fill_(INIT)
    torch.cuda.synchronize()
    before = ctx.workspace_bytes()
    with Delayed(s, idle_ms) as delay:  # 3. a delay on s, and behind it the real input
        c.raw.copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.run(vp(s.cuda_stream))  # 4. the call, while s is busy
    got = {name: c.fetch(name, np.uint8).copy() for name in c.outs}  # 5. no torch synchronisation
    after = ctx.workspace_bytes()
    delay.check("kiss_hip_reads_parse_dev")
    assert after == before, "the timed call allocated work arrays (%d -> %d bytes)" % (before, after)
    assert c.rc == 0
    check_report(c.rep, m)
    assert np.array_equal(got["codes"], m["codes"]) and np.array_equal(got["qual"], m["qual"])
    assert np.array_equal(got["read_index"].view(np.uint64), m["read_index"])
    assert np.array_equal(got["name_off"].view(np.uint64), m["name_off"]) and np.array_equal(got["name_len"].view(np.uint32), m["name_len"])
    dev_place.check_canaries(c.raw, *c.outs.values())


# ---- interleave -------------------------------------------------------------------------------------------------------------------
def two_batches(P, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        lens = rng.integers(0, 40, P)
        if P > 3:
            lens[1], lens[2] = 0, 700  # (an empty read; a read longer than a lane's 16 bases many times over)
        index = np.zeros(P + 1, np.uint64)
        np.cumsum(lens, out=index[1:])
        n = int(index[-1])
        out.append((rng.integers(0, 5, n).astype(np.uint8), index, rng.integers(33, 127, n).astype(np.uint8)))
    return out


@pytest.mark.parametrize("with_qual", [True, False])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_interleave_both_forms(ctx, P, with_qual):
    import kiss_amd
    a, b = two_batches(P, 100 + P)
    if not with_qual:
        a, b = a[:2] + (None,), b[:2] + (None,)
    codes, index, qual = rm.interleave(a, b)
    host = kiss_amd.interleave_reads(a, b)
    assert np.array_equal(host["reads"], codes) and np.array_equal(host["read_index"], index)
    assert (host["qual"] is None) == (qual is None) and (qual is None or np.array_equal(host["qual"], qual))
    # the device form on placed arrays
    dev, lib, fill = device(), ctx._lib, (7, 9)
    ins = {}
    for tag, (c, i, q) in (("a", a), ("b", b)):
        ins["c" + tag] = dev_place.place(c, 1, GUARD, fill, device=dev)
        ins["i" + tag] = dev_place.place(i, 8, GUARD, fill, device=dev)
        if with_qual:
            ins["q" + tag] = dev_place.place(q, 3, GUARD, fill, device=dev)
    total = codes.size
    outs = {"codes": dev_place.place_out(total, 3, GUARD, fill, device=dev), "index": dev_place.place_out(8 * (2 * P + 1), 8, GUARD, fill, device=dev)}
    if with_qual:
        outs["qual"] = dev_place.place_out(total, 1, GUARD, fill, device=dev)
    adr = lambda d, k: vp(d[k].placement.address) if k in d else None  # noqa: E731

    def call(P_b, cap):
        got = u64(12345)
        rc = lib.kiss_hip_reads_interleave_dev(ctx._ctx, adr(ins, "ca"), adr(ins, "ia"), adr(ins, "qa"), P, adr(ins, "cb"), adr(ins, "ib"),
                                               adr(ins, "qb"), P_b, adr(outs, "codes"), adr(outs, "index"), adr(outs, "qual"), cap,
                                               ctypes.byref(got), None)
        return rc, got.value

    def untouched():
        for v in outs.values():
            assert (dev_place.read_back(v) == INIT).all()

    if P:
        assert call(P - 1, total)[0] == E_INVALID  # unequal counts
        untouched()
    if total:
        assert call(P, total - 1) == (E_INVALID, total)  # one short: the total is reported, nothing written
        untouched()
    assert call(P, total) == (0, total)
    assert np.array_equal(dev_place.read_back(outs["codes"]), codes) and np.array_equal(dev_place.read_back(outs["index"], np.uint64), index)
    if with_qual:
        assert np.array_equal(dev_place.read_back(outs["qual"]), qual)
    dev_place.check_canaries(*ins.values(), *outs.values())


def test_interleave_refusals(ctx):
    import kiss_amd
    from kiss_amd import _lib
    a, b = two_batches(8, 5)
    lib = ctx._lib
    keep = np.zeros(4096, np.uint8)
    out_idx = np.zeros(17, np.uint64)
    p = lambda x: vp(x.ctypes.data)  # noqa: E731

    def host(ia, ib, Pa=8, Pb=8, qa=None, qb=None, q=None):
        return lib.kiss_hip_reads_interleave_host(p(a[0]), p(ia), qa, Pa, p(b[0]), p(ib), qb, Pb, p(keep), p(out_idx), q, keep.size, None, 0)

    assert host(a[1], b[1]) == 0
    assert host(a[1], b[1], Pb=7) == E_INVALID                      # different read counts
    down = a[1].copy()
    down[4] = down[3] - 1
    assert host(down, b[1]) == E_INVALID and host(a[1], a[1] + np.uint64(1)) == E_INVALID  # decreasing; not starting at 0
    assert host(a[1], b[1], qa=p(a[2])) == E_INVALID              # qualities of one batch only
    with pytest.raises(ValueError):
        kiss_amd.interleave_reads(a, two_batches(7, 5)[1])
    # the device form looks at the indices on the device
    import torch
    d = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(device()) for k, v in
         (("ca", a[0]), ("ia", a[1]), ("cb", b[0]), ("ib", b[1]), ("down", down))}
    d_out, d_idx = torch.full((4096,), INIT, dtype=torch.uint8, device=device()), torch.full((17,), -1, dtype=torch.int64, device=device())
    rc = lib.kiss_hip_reads_interleave_dev(ctx._ctx, vp(d["ca"].data_ptr()), vp(d["down"].data_ptr()), None, 8, vp(d["cb"].data_ptr()),
                                           vp(d["ib"].data_ptr()), None, 8, vp(d_out.data_ptr()), vp(d_idx.data_ptr()), None, 4096, None, None)
    assert rc == E_INVALID and bool((d_out == INIT).all()) and bool((d_idx == -1).all())
    assert _lib.KISS_HIP_E_INVALID == E_INVALID


# ---- the Python entries -------------------------------------------------------------------------------------------------------------
def same_as_model(got, m):
    assert np.array_equal(got["reads"], m["codes"]) and np.array_equal(got["read_index"], m["read_index"])
    assert (got["qual"] is None) == (m["qual"] is None) and (m["qual"] is None or np.array_equal(got["qual"], m["qual"]))
    assert got["names"] == m["names"]
    rep = got["report"]
    assert rep["format"] == m["format"]
    for k in REPORT_FIELDS:
        assert rep[k] == m[k], k


def test_parse_reads_host_and_device_entries(ctx, tmp_path):
    import kiss_amd
    import torch
    recs = shaped_records(77, (1, 64, 500, 4100, 33))
    files = {"fastq": fastq_bytes(recs, b"\r\n"), "lines": b">a b\nACGTN\n\nacgtRY\r\n>second\nGG\nTT", "none": b"", "blank": b"\n\n"}
    for name, raw in files.items():
        m = rm.parse(raw, "auto")
        path = tmp_path / (name + ".txt")
        path.write_bytes(raw)
        same_as_model(kiss_amd.parse_reads(raw), m)                      # bytes, the library's own context
        same_as_model(kiss_amd.parse_reads(str(path), ctx=ctx), m)       # a path, the caller's context
        if name == "fastq":
            same_as_model(kiss_amd.parse_reads(raw, format="lines"), rm.parse(raw, "lines"))
            got = kiss_amd.parse_reads(raw, want_qual=False, want_names=False)
            assert got["qual"] is None and got["names"] is None and np.array_equal(got["reads"], m["codes"])
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):  # the device entry runs on the current torch stream
                d_raw = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(device(), non_blocking=True)
                out = kiss_amd.parse_reads_dev(d_raw, ctx=ctx)
                both = kiss_amd.interleave_reads_dev(out, out, ctx)
            side.synchronize()
            assert np.array_equal(out["reads"].cpu().numpy(), m["codes"]) and np.array_equal(out["qual"].cpu().numpy(), m["qual"])
            assert np.array_equal(out["name_len"].cpu().numpy().view(np.uint32), m["name_len"])
            want = rm.interleave((m["codes"], m["read_index"], m["qual"]), (m["codes"], m["read_index"], m["qual"]))
            assert np.array_equal(both["reads"].cpu().numpy(), want[0]) and np.array_equal(both["qual"].cpu().numpy(), want[2])
            assert np.array_equal(both["read_index"].cpu().numpy().view(np.uint64), want[1])
    with pytest.raises(ValueError, match="record 1"):
        kiss_amd.parse_reads(b"@a\nAC\n+\nII\n@b\nAC\n+\nI\n")


def test_parsed_reads_map_as_the_same_reads_given_as_arrays(ctx):
    import kiss_amd
    import kiss_amd.fm_index as fm
    S = gen.iid(30000, 17)
    rng = np.random.default_rng(18)
    cuts = [S[p:p + L].copy() for p, L in zip(rng.integers(0, 29000, 12), (150, 100, 64, 250, 150, 33, 150, 150, 80, 150, 120, 150))]
    for c in cuts[::3]:
        c[len(c) // 2] = (c[len(c) // 2] + 1) & 3
    letters = [bytes(b"ACGT"[x] for x in c) for c in cuts]
    letters[5] = letters[5][:10] + b"N" + letters[5][11:]
    raw = fastq_bytes([(b"r%d" % q, s, b"", b"I" * len(s)) for q, s in enumerate(letters)])
    parsed = kiss_amd.parse_reads(raw)
    arrays = [np.array([rm.CODES.get(c, 4) for c in s], np.uint8) for s in letters]
    f = fm.FMIndex(sa_intv=4).build(S, exact=True)
    a = f.map((parsed["reads"], parsed["read_index"]), S, both_strands=True)
    b = f.map(arrays, S, both_strands=True)
    f.close()
    assert sorted(a) == sorted(b) and a["select_report"]["mapped"] >= 8
    for k, x in a.items():
        if isinstance(x, np.ndarray):
            assert x.dtype == b[k].dtype and x.tobytes() == b[k].tobytes(), k
        elif isinstance(x, dict):
            assert {j: v for j, v in x.items() if not j.startswith("ms_")} == {j: v for j, v in b[k].items() if not j.startswith("ms_")}, k
