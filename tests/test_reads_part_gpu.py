"""The part call on the device (kiss_hip_reads_parse_part_dev / _host; include/kiss_hip_reads_part.h) against
tests/reads_part_model.py: every output array and every report field, on arrays placed as tests/test_reads_gpu.py places them
(the chunk at an odd address between guard bytes -- newlines, so that a byte read outside the chunk would be a line --, every
output at the least alignment of its element), the capacity protocol, the caller's stream, and the loop of part calls over a
file against parse_reads of the file.  Every input is below 2 MB."""
import ctypes

import numpy as np
import pytest

from tests import dev_place
from tests import reads_model as rm
from tests import reads_part_model as pm
from tests.test_reads_gpu import (E_INVALID, GUARD, INIT, Call, bad_file, check_call, check_report, device, file_with_byte_at,
                                  many_short_reads, shaped_records)
from tests.test_reads_model import fastq_bytes

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
NL = 0x0A


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=1 << 23, device=0)  # (four times the largest chunk)
    yield c
    c.close()


class PartCall(Call):
    """one kiss_hip_reads_parse_part_dev call on placed arrays"""

    def __init__(self, ctx, raw, fmt, final, max_records, bases_cap, reads_cap, **kw):
        from kiss_amd import _lib
        self.part = _lib.ReadsPartReport()
        self.final, self.max_records = int(final), int(max_records)
        super().__init__(ctx, raw, fmt, bases_cap, reads_cap, **kw)

    @property
    def rep(self):
        return self.part.parsed

    @rep.setter
    def rep(self, value):  # (the base class makes a report of its own kind: not used)
        pass

    def run(self, stream=None):
        ctx, nbytes, fmt, bases_cap, reads_cap = self.args
        self.rc = self.lib.kiss_hip_reads_parse_part_dev(ctx._ctx, vp(self.raw.placement.address), nbytes, fmt, self.final, self.max_records,
                                                         self.address("codes"), self.address("qual"), bases_cap, self.address("read_index"),
                                                         self.address("name_off"), self.address("name_len"), reads_cap,
                                                         ctypes.byref(self.part), stream)
        return self


def check_part(c, m, what=""):
    assert (c.part.records_complete, c.part.records, c.part.bytes_used) == (m["records_complete"], m["records"], m["bytes_used"]), what
    check_call(c, m, what)


def part_and_check(ctx, raw, fmt, final, max_records=0, raw_lead=1, byte_lead=3, slack=0, fill=NL, **kw):
    m = pm.parse_part(raw, fmt, final, max_records)
    Q, B = (0, 0) if m["bad_records"] else (m["reads"], m["bases"])
    c = PartCall(ctx, raw, fmt, final, max_records, B + slack, Q + slack, raw_lead=raw_lead, byte_lead=byte_lead, fill=fill, **kw)
    check_part(c, m, (fmt, final, max_records, len(raw), raw[:40]))
    return c, m


def lines_file(recs, eol=b"\n"):
    return b"".join((b">" + n + eol if r % 3 else b"") + s + eol + (eol if r % 4 == 1 else b"") for r, (n, s, _, _) in enumerate(recs))


# ---- where the chunk ends --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fastq", "lines"])
@pytest.mark.parametrize("raw_lead", [0, 1, 3])
def test_newline_at_a_tile_boundary_and_the_chunk_end_around_it(ctx, fmt, raw_lead):
    """byte `at` of the file is a '\\n' (the last one of record 0, or of a read line); the chunk ends on it, before it, behind it"""
    for at in (4095, 4096, 4097):
        raw = file_with_byte_at("\n", at)
        if fmt == "lines":
            raw = b">n\n" + b"A" * (at - 3) + raw[at:]
        assert raw[at] == NL
        for end in (at, at + 1, at + 2, len(raw)):
            for final in (False, True):
                c, m = part_and_check(ctx, raw[:end], fmt, final, raw_lead=raw_lead)
                if fmt == "fastq" and end <= at + 1:
                    assert m["records"] == int(end > at or final)  # (final at `at`: the file ends without a last '\n')


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_chunks_ending_at_behind_and_inside_a_line(ctx, fmt, eol):
    recs = shaped_records(41, (1, 63, 64, 65, 255, 300))
    recs.insert(2, (b"empty", b"", b"", b""))
    raw = fastq_bytes(recs, eol) if fmt == "fastq" else lines_file(recs, eol)
    ends = [i + 1 for i in range(len(raw)) if raw[i] == NL]
    some = sorted(set(ends[:6] + ends[-9:] + ends[::5]))
    for e in some:
        for end in (e, e + 1, e - 1, e - len(eol), e + 3):  # at a line's end, one byte behind, on its '\n' or '\r', inside the next
            if 0 <= end <= len(raw):
                part_and_check(ctx, raw[:end], fmt, False)
                part_and_check(ctx, raw[:end], fmt, True, slack=3)
    part_and_check(ctx, raw[:ends[3] + 2], "auto", False)


@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_max_records(ctx, fmt):
    recs = shaped_records(42, (5, 4097, 1, 64, 300))
    for raw in (fastq_bytes(recs) if fmt == "fastq" else lines_file(recs), fastq_bytes(recs, last_eol=False) if fmt == "fastq" else lines_file(recs)[:-1]):
        for final in (False, True):
            complete = pm.parse_part(raw, fmt, final)["records_complete"]
            assert complete == (5 if final or raw.endswith(b"\n") else 4)
            for max_records in (0, 1, complete - 1, complete, complete + 1):
                c, m = part_and_check(ctx, raw, fmt, final, max_records, slack=1)
                assert m["records"] == (complete if max_records == 0 else min(max_records, complete))
                assert m["bytes_used"] == len(raw) or not (final and m["records"] == complete)


def test_fastq_4k_plus_1_2_3_complete_lines_and_blank_lines(ctx):
    recs = shaped_records(43, (10, 70, 3))
    lines = fastq_bytes(recs).split(b"\n")[:-1] + [b"@next", b"ACGT", b"+"]
    for extra in (0, 1, 2, 3):
        raw = b"\n".join(lines[:12 + extra]) + b"\n"
        c, m = part_and_check(ctx, raw, "fastq", False)
        assert (m["records"], m["bytes_used"]) == (3, len(fastq_bytes(recs)))
        c, m = part_and_check(ctx, raw, "fastq", True)  # the end of the file: the parse refuses the truncated record
        assert (m["records"], m["first_bad"], m["first_bad_kind"]) == ((3, None, 0) if extra == 0 else (4, 3, rm.BAD_TRUNCATED))
    whole = fastq_bytes(recs)
    for blanks in (0, 1, 4, 5):  # lines that are empty so far are never consumed early; at the end of the file they are dropped
        for final in (False, True):
            c, m = part_and_check(ctx, whole + b"\n" * blanks, "fastq", final)
            assert (m["records"], m["bytes_used"]) == (3, len(whole) + (blanks if final else 0))
    empties = b"@a\n\n+\n\n@b\n\n+\n\n"  # empty reads at the cut: no line dropped from a prefix
    for end in (7, 8, 10, 14, 16):
        for final in (False, True):
            for max_records in (0, 1):
                part_and_check(ctx, empties[:end], "fastq", final, max_records, slack=1)
    for raw in (b"", b"\n", b"\n\r\n\n\n\n", b"@", b"ACGT", b">x\n"):  # nothing, blank lines only, no complete line
        for fmt in ("fastq", "lines", "auto"):
            for final in (False, True):
                part_and_check(ctx, raw, fmt, final, slack=2)


def test_many_short_reads_and_one_long_read(ctx):
    short = many_short_reads()
    c, m = part_and_check(ctx, short[:-3], "fastq", False)
    assert m["records"] == 19999
    c, m = part_and_check(ctx, short, "auto", False, 12345)
    assert m["records"] == 12345 and m["bases"] == 12345
    rng = np.random.default_rng(4)
    long_read = (b"long", bytes(rng.choice(list(b"ACGT"), 300000).tolist()), b"", bytes(rng.integers(33, 127, 300000).astype(np.uint8).tolist()))
    raw = short[:short.index(b"@100\n")] + fastq_bytes([long_read]) + short[:36]
    c, m = part_and_check(ctx, raw[:-1], "fastq", False)  # (the last record lacks its '\n': it stays behind)
    assert m["records"] == 100 + 1 + 3 and m["bases"] == 300000 + 103 and m["names"][100] == "long"
    c, m = part_and_check(ctx, raw[:400000], "fastq", False)  # the chunk ends inside the long read
    assert m["records"] == 100
    c, m = part_and_check(ctx, b">l\n" + long_read[1] + b"\nAC", "lines", False)
    assert m["records"] == 1 and m["bases"] == 300000


@pytest.mark.parametrize("where", ["first", "last", "straddling"])
@pytest.mark.parametrize("kind", [rm.BAD_NO_AT, rm.BAD_NO_PLUS, rm.BAD_LENGTHS, rm.BAD_TRUNCATED])
def test_bad_records_are_numbered_inside_the_chunk(ctx, kind, where):
    raw, r = bad_file(kind, where)
    for final in (False, True):
        c, m = part_and_check(ctx, raw, "fastq", final)
        if kind == rm.BAD_TRUNCATED and not final:  # not the end of the file: the three lines wait for the fourth
            assert m["bad_records"] == 0 and m["records"] == r
        else:
            assert (c.part.parsed.bad_records, c.part.parsed.first_bad, c.part.parsed.first_bad_kind) == (1, r, kind)
    if where == "last" and kind != rm.BAD_TRUNCATED:
        head = len(b"\n".join(raw.split(b"\n")[:8])) + 1  # two records consumed before: the chunk's first_bad is r - 2
        c, m = part_and_check(ctx, raw[head:], "fastq", False)
        assert (c.part.parsed.first_bad, c.part.parsed.first_bad_kind) == (r - 2, kind)
        c, m = part_and_check(ctx, raw, "fastq", False, r)  # max_records keeps the bad record out of the prefix
        assert m["bad_records"] == 0 and m["records"] == r


# ---- the capacity protocol, the addresses ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["lines", "fastq"])
def test_size_then_fill(ctx, fmt):
    from kiss_amd import _lib
    recs = shaped_records(8, (1, 65, 300, 4097, 20))
    raw = (fastq_bytes(recs) if fmt == "fastq" else lines_file(recs))[:-1]  # (no last '\n': the last record is one only with final)
    for final, max_records in ((False, 0), (True, 3), (True, 0)):
        m = pm.parse_part(raw, fmt, final, max_records)
        Q, B = m["reads"], m["bases"]
        assert Q == (3 if max_records else 5 if final else 4)
        for bases_cap, reads_cap in ((0, 0), (B - 1, Q), (B, Q - 1), (0, Q), (B, 0)):
            c = PartCall(ctx, raw, fmt, final, max_records, bases_cap, reads_cap, fill=NL)
            assert c.rc == E_INVALID and c.rep.bad_records == 0 and (c.rep.reads, c.rep.bases) == (Q, B), (bases_cap, reads_cap)
            assert (c.part.records_complete, c.part.records, c.part.bytes_used) == (m["records_complete"], Q, m["bytes_used"])
            c.untouched()
        check_part(PartCall(ctx, raw, fmt, final, max_records, B, Q, fill=NL), m, "exact")
        check_part(PartCall(ctx, raw, fmt, final, max_records, B + 77, Q + 5, fill=NL), m, "more than needed")
        for want_qual, want_names in ((False, True), (True, False), (False, False)):
            check_part(PartCall(ctx, raw, fmt, final, max_records, B, Q, want_qual=want_qual, want_names=want_names, fill=NL), m)
    d_raw = dev_place.place(np.frombuffer(raw, np.uint8), 1, GUARD, 0, device=device())
    d_idx = dev_place.place_out(8, 8, GUARD, 0, device=device())
    call = lambda nbytes, f, idx, noff: ctx._lib.kiss_hip_reads_parse_part_dev(  # noqa: E731
        ctx._ctx, vp(d_raw.placement.address), nbytes, f, 0, 0, None, None, 0, idx, noff, None, 0, None, None)
    idx = vp(d_idx.placement.address)
    assert call(len(raw), 3, idx, None) == E_INVALID and call(len(raw), 0, None, None) == E_INVALID and call(len(raw), 0, idx, idx) == E_INVALID
    assert call(0xFFFFF001, 0, idx, None) == _lib.KISS_HIP_E_UNSUPPORTED
    dev_place.check_canaries(d_raw, d_idx)
    assert (dev_place.read_back(d_idx) == INIT).all()
    import kiss_amd
    with kiss_amd.Context(max_n=1 << 20) as small:  # a ctx whose scratch does not scan that many bytes
        c = PartCall(small, (np.zeros(1_500_000, np.uint8) + 65).tobytes(), "lines", False, 0, 0, 0)
        assert c.rc == _lib.KISS_HIP_E_UNSUPPORTED
        c.untouched()


@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_the_chunk_at_every_address_mod_16(ctx, fmt):
    recs = shaped_records(44, (1, 63, 64, 65, 255, 256, 257, 5000))
    raw = (fastq_bytes(recs, b"\r\n") if fmt == "fastq" else lines_file(recs))[:-40]
    for lead in range(16):
        part_and_check(ctx, raw, fmt, False, 0, raw_lead=lead, byte_lead=lead % 4)
        part_and_check(ctx, raw, fmt, True, 6, raw_lead=lead, byte_lead=(lead + 1) % 4)


def test_the_host_entry_and_the_python_wrappers(ctx):
    import kiss_amd
    import torch
    recs = shaped_records(45, (7, 300, 4100, 2))
    raw = fastq_bytes(recs)[:-1]
    for final, max_records in ((False, 0), (True, 0), (True, 2)):
        m = pm.parse_part(raw, "auto", final, max_records)
        got = kiss_amd.batches.parse_reads_part(raw, final=final, max_records=max_records, first_read=10)
        dev = kiss_amd.batches.parse_reads_part_dev(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(device()), "fastq", final, max_records, ctx=ctx)
        for g in (got, dev):
            rep = g["report"]
            assert (rep["records_complete"], rep["records"], rep["bytes_used"], rep["reads"], rep["format"]) == (
                m["records_complete"], m["records"], m["bytes_used"], m["reads"], "fastq")
        assert np.array_equal(got["reads"], m["codes"]) and np.array_equal(got["qual"], m["qual"]) and np.array_equal(got["read_index"], m["read_index"])
        assert np.array_equal(dev["reads"].cpu().numpy(), m["codes"]) and np.array_equal(dev["read_index"].cpu().numpy().view(np.uint64), m["read_index"])
        assert got["names"] == [n if n != str(q) else str(10 + q) for q, n in enumerate(m["names"])] and got["names"][2:3] == ["12"][:len(got["names"]) - 2]
    bad = raw.replace(b"\n+again\n", b"\n-\n")
    with pytest.raises(ValueError, match="record 11"):  # (record 1 of the chunk, 10 consumed before)
        kiss_amd.batches.parse_reads_part(bad, final=False, first_read=10)


# ---- the caller's stream ----------------------------------------------------------------------------------------------------------
def test_work_runs_on_the_callers_stream_and_is_done_on_return(ctx):
    """the method of tests/test_reads_gpu.py: the chunk is overwritten with a decoy (other letters, qualities and names, and its
    line ends elsewhere, so that the decoy's cut is another one); a delay and then the copy that puts the real chunk back are queued
    on s; the call is made with s while s is busy"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    recs = shaped_records(31, (150,) * 400 + (3000, 1))
    raw = fastq_bytes(recs)[:-700]
    decoy_recs = [(n + b"x", s[:-1].translate(bytes.maketrans(b"ACGTacgtNRY", b"CATGcatgRYN")), p, bytes(33 + (c - 33 + 1) % 94 for c in q[:-1]))
                  for n, s, p, q in recs]
    decoy = fastq_bytes(decoy_recs)[:len(raw)]
    m, md = pm.parse_part(raw, "auto", False, 390), pm.parse_part(decoy, "auto", False, 390)
    assert len(decoy) == len(raw) and m["bytes_used"] != md["bytes_used"] and m["records"] == md["records"] == 390
    s = caller_stream()
    c = PartCall(ctx, raw, "auto", False, 390, m["bases"], m["reads"], raw_lead=1, fill=NL)
    for _ in range(2):  # 1. warm up on the NULL stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(None)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    check_part(c, m, "warm-up on the NULL stream")
    staging = c.raw.clone()
    c.raw.copy_(torch.from_numpy(np.frombuffer(decoy, np.uint8).copy()))  # 2. the decoy; the outputs as before any call
    for v in c.outs.values():
        v.fill_(INIT)
    torch.cuda.synchronize()
    before = ctx.workspace_bytes()
    with Delayed(s, idle_ms) as delay:  # 3. a delay on s, and behind it the real chunk
        c.raw.copy_(staging, non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    c.run(vp(s.cuda_stream))  # 4. the call, while s is busy
    got = {name: c.fetch(name, np.uint8).copy() for name in c.outs}  # 5. no torch synchronisation
    after = ctx.workspace_bytes()
    delay.check("kiss_hip_reads_parse_part_dev")
    assert after == before, "the timed call allocated work arrays (%d -> %d bytes)" % (before, after)
    assert c.rc == 0 and (c.part.records, c.part.bytes_used) == (390, m["bytes_used"])
    check_report(c.rep, m)
    assert np.array_equal(got["codes"], m["codes"]) and np.array_equal(got["qual"], m["qual"])
    assert np.array_equal(got["read_index"].view(np.uint64), m["read_index"])
    assert np.array_equal(got["name_off"].view(np.uint64), m["name_off"]) and np.array_equal(got["name_len"].view(np.uint32), m["name_len"])
    dev_place.check_canaries(c.raw, *c.outs.values())


# ---- the loop of part calls is the parse of the file ------------------------------------------------------------------------------
def fifty_kb(fmt):
    rng = np.random.default_rng(46)
    lo, hi = (0, 220) if fmt == "fastq" else (1, 400)  # (a file of lines has no empty reads)
    recs = shaped_records(46, tuple(int(x) for x in rng.integers(lo, hi, 230)) + (9000,))
    raw = fastq_bytes(recs, b"\r\n") if fmt == "fastq" else lines_file(recs)
    assert 45000 < len(raw) < 100000
    return raw + b"\n\n"


@pytest.mark.parametrize("chunk", [4096, 4097, 10000])
@pytest.mark.parametrize("fmt", ["fastq", "lines"])
def test_the_loop_of_part_calls_is_parse_reads_of_the_file(ctx, tmp_path, fmt, chunk):
    import kiss_amd
    raw = fifty_kb(fmt)
    path = tmp_path / "reads"
    path.write_bytes(raw)
    whole = kiss_amd.parse_reads(raw, ctx=ctx)
    assert whole["report"]["reads"] == 231 and whole["report"]["format"] == fmt
    for batch_reads in (0, 60, 7):  # 0: the plain loop of part calls, every whole record of a chunk a batch
        if batch_reads:
            got = list(kiss_amd.batches.read_batches(str(path), batch_reads=batch_reads, chunk_bytes=chunk, ctx=ctx))
            assert [b["records"] for b in got] == [min(batch_reads, 231 - a) for a in range(0, 231, batch_reads)]  # (a chunk grows)
        else:
            got, pos, size, now = [], 0, chunk, "auto"
            while pos < len(raw):
                end = min(len(raw), pos + size)
                b = kiss_amd.batches.parse_reads_part(raw[pos:end], now, end == len(raw), 0, first_read=sum(x["records"] for x in got))
                rep = b["report"]
                now, pos, size = rep["format"], pos + rep["bytes_used"], chunk if rep["records"] else 2 * size
                if rep["records"]:
                    got.append(dict(b, records=rep["records"], first_read=sum(x["records"] for x in got)))
                if end == len(raw) and rep["records"] == rep["records_complete"]:
                    break
            assert len(got) >= 3 and all(b["records"] > 0 for b in got)
        assert [b["first_read"] for b in got] == np.cumsum([0] + [b["records"] for b in got[:-1]]).tolist()
        assert np.array_equal(np.concatenate([b["reads"] for b in got]), whole["reads"])
        index = np.concatenate([[0]] + [b["read_index"][1:].astype(np.int64) + int(sum(int(x["read_index"][-1]) for x in got[:i]))
                                        for i, b in enumerate(got)])
        assert np.array_equal(index, whole["read_index"].astype(np.int64))
        assert [n for b in got for n in b["names"]] == whole["names"]
        if fmt == "fastq":
            assert np.array_equal(np.concatenate([b["qual"] for b in got]), whole["qual"])
        else:
            assert all(b["qual"] is None for b in got)
