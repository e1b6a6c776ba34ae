"""kiss_hip_bai_* (include/kiss_hip_bai.h) restated as plain loops: which records are BAD, the interval and the
bin of a record, the virtual offsets, the chunks, the linear index and the bytes of FILE.bai with the counts of the report.  And the
other side: a parser of those bytes, the specification's reader rule (reg2bins, the linear index's lower bound) and a fetch that
walks the BGZF blocks of a file at the virtual offsets.  Nothing here is fast and nothing is shared with the library;
tests/test_bai_model.py holds build + fetch against brute force and against a file worked by hand."""
import struct
import zlib

from tests import bam_model as B
from tests import bam_sort_model as SM

PSEUDO_BIN = 37450
MAX_END = 1 << 29
COFF_END = 1 << 48
REF_OPS = (0, 2, 3, 7, 8)  # M, D, N, =, X


def make_record(ref, pos, flag=0, cigar=(), name=b"r", tail=b"", bin_=0xBEEF):
    """a record with the fields the index reads, a cigar of (len, op) pairs, and `tail` behind it; the bin field holds nonsense:
    it is not trusted"""
    name = bytes(name) + b"\0"
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), 0, bin_, len(cigar) & 0xFFFF, flag, 0, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", (n << 4 | op) & 0xFFFFFFFF) for n, op in cigar) + bytes(tail)
    return struct.pack("<i", len(body)) + body


def interval(rec):
    """(refID, beg, end, flag) of a record; `why` it is BAD by the index's own rules or None.  The record is fine by the sort's"""
    _, ref, pos, l_name = struct.unpack_from("<iiiB", rec, 0)
    n_ops, flag = struct.unpack_from("<HH", rec, 16)
    why = None
    reflen = 0
    if ref >= 0 and pos == -1:
        why = "pos"
    if not flag & 4:
        if 36 + l_name + 4 * n_ops > len(rec):
            why = why or "cigar bytes"
        else:
            for i in range(n_ops):
                w, = struct.unpack_from("<I", rec, 36 + l_name + 4 * i)
                if w & 15 > 8:
                    why = why or "op code"
                if w & 15 in REF_OPS:
                    reflen += w >> 4
    end = pos + (1 if flag & 4 else max(1, reflen))
    if ref >= 0 and why is None and end > MAX_END:
        why = "end"
    return ref, pos, end, flag, why


def bad_records(bam, rec_index, n_ref):
    """the BAD records, ascending"""
    raw = bytes(bytearray(bam))
    ri = [int(x) for x in rec_index]
    records = len(ri) - 1
    by_sort = set(SM.bad_records(raw, ri, n_ref))
    bad = set(by_sort)
    for r in range(records):
        if r in by_sort:
            continue
        if r > 0 and r - 1 not in by_sort and SM.key_of(raw, ri[r], n_ref) < SM.key_of(raw, ri[r - 1], n_ref):
            bad.add(r)
        if interval(raw[ri[r]:ri[r + 1]])[4]:
            bad.add(r)
    return sorted(bad)


def build(bam, rec_index, n_ref, block_bytes=0, block_index=None, file_base=0):
    """-> dict(status, report[, bai]): status "ok" with the bytes of the index, "invalid" (a BAD record: bad and first_bad in the
    report; or a block_index that decreases) or "unsupported" (a coff of 2^48 or more)"""
    raw = bytes(bytearray(bam))
    ri = [int(x) for x in rec_index]
    records = len(ri) - 1
    bb = block_bytes or B.BLOCK_DEFAULT
    assert 1 <= bb <= B.BLOCK_MAX
    report = dict(records=records, bam_bytes=len(raw), bai_bytes=0, chunks=0, bins=0, windows=0, mapped=0, unmapped_placed=0, no_coor=0, bad=0,
                  first_bad=0)
    if records == 0:
        bai = b"BAI\1" + struct.pack("<i", n_ref) + bytes(8 * n_ref) + bytes(8)
        report["bai_bytes"] = len(bai)
        return {"status": "ok", "bai": bai, "report": report}
    if file_base >= COFF_END:
        return {"status": "unsupported", "report": report}
    bi = None if block_index is None else [int(x) for x in block_index]
    if bi is not None and any(bi[b + 1] < bi[b] for b in range(len(bi) - 1)):
        return {"status": "invalid", "report": report}
    bad = bad_records(raw, ri, n_ref)
    if bad:
        report.update(bad=len(bad), first_bad=bad[0])
        return {"status": "invalid", "report": report}

    def coff(b):
        return file_base + (bi[b] if bi is not None else b * (bb + B.OVERHEAD))

    if coff(len(raw) // bb) >= COFF_END:
        return {"status": "unsupported", "report": report}

    def voff_at(u):
        return coff(u // bb) << 16 | u % bb

    refs = [dict(bins={}, lin={}, first=None, last=None, mapped=0, unmapped=0, windows=0) for _ in range(n_ref)]
    prev = None
    for r in range(records):
        ref, beg, end, flag, _ = interval(raw[ri[r]:ri[r + 1]])
        if ref < 0:
            report["no_coor"] += 1
            continue
        t = refs[ref]
        voff, vend = voff_at(ri[r]), voff_at(ri[r + 1])
        bin_ = B.reg2bin(beg, end)
        if prev == (ref, bin_):
            t["bins"][bin_][-1][1] = vend
        else:
            t["bins"].setdefault(bin_, []).append([voff, vend])
            report["chunks"] += 1
        prev = (ref, bin_)
        if t["first"] is None:
            t["first"] = voff
        t["last"] = vend
        t["unmapped" if flag & 4 else "mapped"] += 1
        report["unmapped_placed" if flag & 4 else "mapped"] += 1
        t["windows"] = max(t["windows"], 1 + ((end - 1) >> 14))
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if w not in t["lin"] or voff < t["lin"][w]:
                t["lin"][w] = voff
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for t in refs:
        have = t["first"] is not None
        out.append(struct.pack("<i", len(t["bins"]) + (1 if have else 0)))
        report["bins"] += len(t["bins"])
        for bin_ in sorted(t["bins"]):
            out.append(struct.pack("<Ii", bin_, len(t["bins"][bin_])))
            for cb, ce in t["bins"][bin_]:
                out.append(struct.pack("<QQ", cb, ce))
        if have:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, t["first"], t["last"], t["mapped"], t["unmapped"]))
        out.append(struct.pack("<i", t["windows"]))
        report["windows"] += t["windows"]
        lin = [None] * t["windows"]
        for w in range(t["windows"] - 1, -1, -1):  # (the last window is covered)
            lin[w] = t["lin"][w] if w in t["lin"] else lin[w + 1]
        out.append(struct.pack("<%dQ" % len(lin), *lin))
    out.append(struct.pack("<Q", report["no_coor"]))
    bai = b"".join(out)
    report["bai_bytes"] = len(bai)
    return {"status": "ok", "bai": bai, "report": report}


# ---- the reader ----------------------------------------------------------------------------------------------------------
def parse(bai):
    """the bytes of an index -> dict(refs: a list of dict(bins: {bin: [(beg, end)]} in file order of the bins, order: the bin
    numbers as they stand, pseudo: None or (first, last, mapped, unmapped), ioffset: list), n_no_coor); asserts that no byte is left"""
    bai = bytes(bai)
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    at = 8
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, at)
        at += 4
        t = dict(bins={}, order=[], pseudo=None, ioffset=[])
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", bai, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", bai, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            t["order"].append(bin_)
            if bin_ == PSEUDO_BIN:
                assert n_chunk == 2
                t["pseudo"] = chunks[0] + chunks[1]
            else:
                assert bin_ not in t["bins"]
                t["bins"][bin_] = chunks
        n_intv, = struct.unpack_from("<i", bai, at)
        at += 4
        t["ioffset"] = list(struct.unpack_from("<%dQ" % n_intv, bai, at))
        at += 8 * n_intv
        refs.append(t)
    n_no_coor, = struct.unpack_from("<Q", bai, at)
    assert at + 8 == len(bai)
    return {"refs": refs, "n_no_coor": n_no_coor}


def reg2bins(beg, end):
    """the SAM specification's reg2bins on [beg, end), as one range of bin numbers per level"""
    end -= 1
    return [range(0, 1)] + [range(first + (beg >> shift), first + (end >> shift) + 1) for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681))]


def query_chunks(parsed, ref, beg, end):
    """the chunks a reader has to look into for [beg, end) of reference ref, by the specification's rule: the bins of reg2bins,
    without the chunks that end at or before the linear index's offset of the window of beg; ascending"""
    t = parsed["refs"][ref]
    if beg >> 14 >= len(t["ioffset"]):
        return []
    least = t["ioffset"][beg >> 14]
    got = []
    levels = reg2bins(beg, end)
    for bin_, chunks in t["bins"].items():  # (the bins of the list that the reference has)
        if any(bin_ in level for level in levels):
            got += [(cb, ce) for cb, ce in chunks if ce > least]
    return sorted(got)


class BgzfReader:
    """a BGZF file read at virtual offsets: the block at a compressed offset is inflated when it is asked for"""

    def __init__(self, data):
        self.data = bytes(data)
        self.blocks = {}

    def block(self, coff):
        if coff not in self.blocks:
            d = self.data
            assert d[coff:coff + 4] == b"\x1f\x8b\x08\x04" and d[coff + 12:coff + 14] == b"BC", coff
            bsize = struct.unpack_from("<H", d, coff + 16)[0] + 1
            pay = zlib.decompress(d[coff + 18:coff + bsize - 8], -15)
            assert struct.unpack_from("<II", d, coff + bsize - 8) == (zlib.crc32(pay) & 0xFFFFFFFF, len(pay))
            self.blocks[coff] = (pay, coff + bsize)
        return self.blocks[coff]

    def norm(self, voff):
        """the end of a block is offset 0 of the next one: one place with two names (the definition names the end of the LAST, short
        block of the records by that block; a reader's tell stands in the block behind it)"""
        pay, nxt = self.block(voff >> 16)
        return nxt << 16 if voff & 0xFFFF == len(pay) and nxt < len(self.data) else voff   # (the end-of-file block is the last place)

    def read(self, voff, n):
        """n bytes from voff -> (the bytes, the virtual offset behind them: at the end of a block, offset 0 of the next one)"""
        coff, at = voff >> 16, voff & 0xFFFF
        out = b""
        while True:
            pay, nxt = self.block(coff)
            take = pay[at:at + n - len(out)]
            out += take
            at += len(take)
            if len(out) == n:
                return out, self.norm(coff << 16 | at)
            assert at == len(pay)
            coff, at = nxt, 0


def file_frame(file_bytes, header_bytes):
    """a whole BAM file whose header (header_bytes unframed bytes) is framed in blocks of its own -> (file_base, block_index): the
    bytes in front of the first record block and the offsets of the record blocks from there, blocks + 1 of them (the end-of-file
    block and every other empty block is not counted)"""
    rd = BgzfReader(file_bytes)
    at, seen, base, index = 0, 0, None, []
    while at < len(rd.data):
        pay, nxt = rd.block(at)
        if seen == header_bytes and base is None:
            base = at
        if base is not None and pay:
            index.append(at - base)
        seen += len(pay)
        assert seen <= header_bytes or base is not None, "the header does not end on a block"
        at = nxt
    end = at - len(B.BGZF_EOF) if rd.data.endswith(B.BGZF_EOF) else at
    return base, index + [end - base]


def fetch(file_bytes, parsed, ref, beg, end):
    """the records of [beg, end) on reference ref as a reader finds them through the index: every record inside the chunks of
    query_chunks that overlaps the region, each once, in file order"""
    rd = file_bytes if isinstance(file_bytes, BgzfReader) else BgzfReader(file_bytes)  # (a reader keeps the blocks it has inflated)
    got, seen = [], set()
    for cb, ce in query_chunks(parsed, ref, beg, end):
        at, ce = rd.norm(cb), rd.norm(ce)
        while at < ce:
            head, nxt = rd.read(at, 4)
            rec, nxt = rd.read(nxt, struct.unpack("<i", head)[0])
            rec = head + rec
            r, b, e, _, _ = interval(rec)
            if r == ref and b < end and e > beg and at not in seen:
                seen.add(at)
                got.append((at, rec))
            at = nxt
        assert at == ce, (at, ce)
    return [rec for _, rec in sorted(got)]


def overlapping(records, ref, beg, end):
    """brute force: the records of the list that overlap [beg, end) of ref, in order"""
    out = []
    for rec in records:
        r, b, e, _, _ = interval(rec)
        if r == ref and b < end and e > beg:
            out.append(rec)
    return out
