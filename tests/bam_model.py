"""The BAM output restated as plain Python (include/kiss_hip_bam.h): an encoder, batch dict -> the records, their
index arrays and the report; an independent decoder, one record -> its SAM line; the BGZF framing with stored blocks; and the
CRC-32 of a block computed piece by piece and combined by multiplication with x^(8 len) modulo the polynomial, as the device does.

A batch is the dict of tests/fm_sam_model.py, and WHICH records a read has, their FLAG, MAPQ, place, TLEN and tags are that
model's rules: the encoder walks the reads exactly as fm_sam_model.read_lines does, and the test holds decode(encode(batch))
against fm_sam_model.sam_model's lines byte for byte."""
import struct
import zlib

import numpy as np

from tests import fm_sam_model as S

NONE = S.NONE
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK_DEFAULT, BLOCK_MAX, OVERHEAD = 65280, 65505, 31


# ---- the records ---------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """the SAM specification's reg2bin on [beg, end), with Python's (arithmetic) shifts"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _pos0(b, h):
    """(record index, POS - 1) of hit h"""
    t = b["hits"][h]
    ref = int(t[S.H_REF])
    return ref, int(b["alns"][int(t[S.H_ALN])][S.A_TBEG]) - int(b["bounds"][ref])


def _exists(b, h):
    t = b["hits"][h]
    a, ref = int(t[S.H_ALN]), int(t[S.H_REF])
    return a < len(b["alns"]) and ref < len(b["ref_names"]) and int(b["alns"][a][S.A_TBEG]) >= int(b["bounds"][ref])


def bad_reads_first(b):
    """the reads that are BAD before any record is laid out: for SAM, by the name, by L, by a position"""
    bad = set(S.bad_reads(b))
    Q, H = len(b["read_index"]) - 1, int(b["hit_index"][-1])
    for q in range(Q):
        L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
        if not 1 <= len(b["names"][q]) <= 254 or L >= 1 << 28:
            bad.add(q)
        look = list(range(int(b["hit_index"][q]), int(b["hit_index"][q + 1])))
        if b["pairs"] is not None:
            pr = b["pairs"][q // 2]
            other = int(pr[S.P_HIT1] if q & 1 else pr[S.P_HIT2])
            if other != NONE and other < H:
                look.append(other)
        for h in look:
            if _exists(b, h) and _pos0(b, h)[1] >= 1 << 31:
                bad.add(q)
    return sorted(bad)


def _nibbles(b, q, reverse):
    codes = [int(c) for c in b["reads"][int(b["read_index"][q]):int(b["read_index"][q + 1])]]
    if reverse:
        codes = [3 - c if c <= 3 else c for c in codes[::-1]]
    nib = [1 << c if c <= 3 else 15 for c in codes] + [0]
    return bytes(nib[2 * j] << 4 | nib[2 * j + 1] for j in range((len(codes) + 1) // 2))


def _qual(b, q, reverse):
    L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
    if b["qual"] is None:
        return b"\xff" * L
    ql = [(int(x) - 33) & 0xFF for x in b["qual"][int(b["read_index"][q]):int(b["read_index"][q + 1])]]
    return bytes(ql[::-1] if reverse else ql)


def _pack(ref, pos, name, mapq, bin_, cigar, flag, L, nref, npos, tlen, seq, qual, tags):
    body = struct.pack("<iiBBHHHIiiI", ref, pos, len(name) + 1, mapq & 0xFF, bin_ & 0xFFFF, len(cigar), flag & 0xFFFF, L, nref, npos,
                       tlen & 0xFFFFFFFF)
    body += name + b"\0" + b"".join(struct.pack("<I", w) for w in cigar) + seq + qual + tags
    return struct.pack("<i", len(body)) + body


def unmapped_record(b, q, bits, place):
    """place: None or (record index, POS - 1)"""
    L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
    ref, pos = place if place else (-1, -1)
    return _pack(ref, pos, b["names"][q], 0, reg2bin(pos, pos + 1), [], bits | 4, L, ref, pos, 0, _nibbles(b, q, False), _qual(b, q, False), b""), None


def hit_record(b, q, h, bits=0, place=None, chosen=False, mapq=None, tlen=0, mate_score=None, proper=False, paired=False):
    """-> (the record, why BAM cannot hold it or None)"""
    t = b["hits"][h]
    a, hflags = int(t[S.H_ALN]), int(t[S.H_FLAGS])
    k = b["alns"][a]
    L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
    reverse = bool(hflags & S.REVERSE)
    flag = bits | (16 if reverse else 0)
    if not chosen:
        flag |= (256 if hflags & S.SECONDARY else 0) | (2048 if hflags & S.SUPPLEMENTARY else 0)
    ref, pos = _pos0(b, h)
    ops = [int(w) for w in b["cigar"][int(b["cigar_index"][a]):int(b["cigar_index"][a + 1])]]
    why = "op code" if any(w & 15 > 2 for w in ops) else None
    reflen = sum(w >> 4 for w in ops if w & 15 in (0, 2))
    cigar = ([int(k[S.A_RBEG]) << 4 | 4] if int(k[S.A_RBEG]) else []) + ops + ([(L - int(k[S.A_REND])) << 4 | 4] if L > int(k[S.A_REND]) else [])
    if len(cigar) > 65535:
        why = "ops"
    tags = b"NMI" + struct.pack("<I", (int(k[S.A_MISM]) + int(k[S.A_INS]) + int(k[S.A_DEL])) & 0xFFFFFFFF)
    if b["md"] is not None:
        tags += b"MDZ" + bytes(bytearray(b["md"][int(b["md_index"][h]):int(b["md_index"][h + 1])])) + b"\0"
    tags += b"ASI" + struct.pack("<I", int(t[S.H_SCORE]))
    if not hflags & S.SECONDARY:
        tags += b"XSI" + struct.pack("<I", int(t[S.H_SUB]))
    if mate_score is not None:
        tags += b"YSI" + struct.pack("<I", mate_score)
    if proper:
        tags += b"YTZCP\0"
    if paired and b["source"] is not None and int(b["source"][a]) >= int(b["first_alns"]):
        tags += b"YRC\x01"
    nref, npos = place if place else (-1, -1)
    if why == "ops":  # (n_cigar_op does not hold the count: the record is never written)
        cigar = cigar[:65535]
    rec = _pack(ref, pos, b["names"][q], int(t[S.H_MAPQ]) if mapq is None else mapq, reg2bin(pos, pos + max(1, reflen)), cigar, flag, L, nref, npos,
                tlen, _nibbles(b, q, reverse), _qual(b, q, reverse), tags)
    if len(rec) - 4 >= 1 << 31:
        why = "block_size"
    return rec, why


def read_records(b, q):
    """the records of read q, as fm_sam_model.read_lines gives its lines -> (list of (record, why), unmapped records)"""
    hb, he = int(b["hit_index"][q]), int(b["hit_index"][q + 1])
    if b["pairs"] is None:
        if he == hb:
            return [unmapped_record(b, q, 0, None)], 1
        return [hit_record(b, q, h) for h in range(hb, he)], 0
    pr = b["pairs"][q // 2]
    i = q & 1
    chosen = [int(pr[S.P_HIT1]), int(pr[S.P_HIT2])]
    mine, other = chosen[i], chosen[1 - i]
    bits = 1 | (128 if i else 64) | (0 if other != NONE else 8)
    if other != NONE and int(b["hits"][other][S.H_FLAGS]) & S.REVERSE:
        bits |= 32
    place = _pos0(b, other) if other != NONE else (_pos0(b, mine) if mine != NONE else None)
    if mine == NONE:
        return [unmapped_record(b, q, bits, place)], 1
    proper = bool(int(pr[S.P_FLAGS]) & S.PROPER)
    tlen = 0
    if other != NONE and int(pr[S.P_TLEN]):
        ti, to = S._place(b, mine)[2], S._place(b, other)[2]
        tlen = int(pr[S.P_TLEN]) if ti < to or (ti == to and i == 0) else -int(pr[S.P_TLEN])
    out = [hit_record(b, q, mine, bits | (2 if proper else 0), place, True, int(pr[S.P_MAPQ2] if i else pr[S.P_MAPQ1]), tlen,
                      int(b["hits"][other][S.H_SCORE]) if other != NONE else None, proper, True)]
    for h in range(hb, he):
        if h == mine:
            continue
        if h == hb:  # the first hit of the read, displaced by the pair
            out.append(hit_record(b, q, h, bits | 256, place, mapq=0, paired=True))
        else:
            out.append(hit_record(b, q, h, bits, place, paired=True))
    return out, 0


def bam_model(b):
    """-> dict(records: list of bytes, bam: their concatenation, rec_index, read_rec, report: records, bam_bytes, unmapped_records,
    longest, bad, first_bad); with a bad read only report (bad, first_bad).  R = 0 is refused by the call: an assertion here"""
    assert len(b["ref_names"]) > 0
    bad = bad_reads_first(b)
    if bad:
        return {"report": {"bad": len(bad), "first_bad": bad[0]}}
    Q = len(b["read_index"]) - 1
    recs, read_rec, unmapped = [], [0], 0
    for q in range(Q):
        got, u = read_records(b, q)
        if any(why for _, why in got):
            bad.append(q)
        recs += [r for r, _ in got]
        unmapped += u
        read_rec.append(len(recs))
    if bad:
        return {"report": {"bad": len(bad), "first_bad": bad[0]}}
    rec_index = [0]
    for r in recs:
        rec_index.append(rec_index[-1] + len(r))
    return {"records": recs, "bam": b"".join(recs), "rec_index": np.array(rec_index, np.uint64), "read_rec": np.array(read_rec, np.uint64),
            "report": {"records": len(recs), "bam_bytes": rec_index[-1], "unmapped_records": unmapped, "longest": max(len(x) for x in recs),
                       "bad": 0, "first_bad": 0}}


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def split_records(bam):
    """the records of a byte string, each with its block_size field"""
    out, at = [], 0
    while at < len(bam):
        size, = struct.unpack_from("<i", bam, at)
        assert size >= 32 and at + 4 + size <= len(bam), (at, size)
        out.append(bytes(bam[at:at + 4 + size]))
        at += 4 + size
    return out


def bam_to_sam(record, ref_names):
    """one record (with its block_size) -> its SAM line, as the SAM writers print it"""
    size, ref, pos, l_name, mapq, bin_, n_cigar, flag, L, nref, npos, tlen = struct.unpack_from("<iiiBBHHHIiii", record, 0)
    assert size == len(record) - 4
    at = 36
    name = record[at:at + l_name - 1]
    assert record[at + l_name - 1] == 0
    at += l_name
    cigar = b""
    for w in struct.unpack_from("<%dI" % n_cigar, record, at):
        cigar += b"%d" % (w >> 4) + b"MIDNSHP=X"[w & 15:(w & 15) + 1]
    at += 4 * n_cigar
    seq = bytearray()
    for i in range(L):
        byte = record[at + i // 2]
        seq.append(b"=ACMGRSVTWYHKDBN"[byte >> 4 if i % 2 == 0 else byte & 15])
    at += (L + 1) // 2
    ql = record[at:at + L]
    at += L
    qual = b"*" if L and all(x == 0xFF for x in ql) else bytes(x + 33 for x in ql)
    rname = ref_names[ref] if ref >= 0 else b"*"
    if nref < 0:
        rnext = b"*"
    elif ref >= 0 and ref_names[nref] == ref_names[ref]:
        rnext = b"="
    else:
        rnext = ref_names[nref]
    f = [name, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cigar or b"*", rnext, b"%d" % (npos + 1), b"%d" % tlen, bytes(seq), qual]
    while at < len(record):
        tag, typ = record[at:at + 2], record[at + 2:at + 3]
        at += 3
        if typ == b"I":
            f.append(tag + b":i:%d" % struct.unpack_from("<I", record, at))
            at += 4
        elif typ == b"C":
            f.append(tag + b":i:%d" % record[at])
            at += 1
        elif typ == b"Z":
            end = record.index(b"\0", at)
            f.append(tag + b":Z:" + record[at:end])
            at = end + 1
        else:
            raise AssertionError("tag type %r" % typ)
    return b"\t".join(f) + b"\n"


def bam_header(ref_names, bounds, text):
    """the unframed BAM header over the header text"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(ref_names))
    for r, nm in enumerate(ref_names):
        out += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", int(bounds[r + 1]) - int(bounds[r]))
    return out


def skip_header(raw):
    """the decompressed bytes of a BAM file -> (the header's bytes, the rest)"""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        at += 4 + l_name + 4
    return raw[:at], raw[at:]


# ---- the framing -----------------------------------------------------------------------------------------------------------
def frame(data, block_bytes=0, eof=False, crc=zlib.crc32):
    data = bytes(data)
    bb = block_bytes or BLOCK_DEFAULT
    assert 1 <= bb <= BLOCK_MAX
    out = []
    for at in range(0, len(data), bb):
        pay = data[at:at + bb]
        n = len(pay)
        out.append(bytes.fromhex("1f8b08040000000000ff0600424302") + b"\0" + struct.pack("<H", n + OVERHEAD - 1) + b"\x01"
                   + struct.pack("<HH", n, n ^ 0xFFFF) + pay + struct.pack("<II", crc(pay) & 0xFFFFFFFF, n))
    return b"".join(out) + (BGZF_EOF if eof else b"")


def out_bytes(n, block_bytes=0, eof=False):
    bb = block_bytes or BLOCK_DEFAULT
    return n + OVERHEAD * (-(-n // bb)) + (28 if eof else 0)


# ---- CRC-32 in pieces --------------------------------------------------------------------------------------------------------
POLY = 0xEDB88320
TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ (POLY if _c & 1 else 0)
    TABLE.append(_c)


def crc_mul(a, b):
    """a * b modulo the polynomial, reflected: bit 31 is x^0"""
    p = 0
    for k in range(32):
        if a & (0x80000000 >> k):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def crc_x8n(m):
    """x^(8 m) modulo the polynomial by the squares x^(8 * 2^j), m < 2^16"""
    assert 0 <= m < 1 << 16
    sq = 0x40000000
    for _ in range(3):
        sq = crc_mul(sq, sq)
    p = 0x80000000
    for j in range(16):
        if m >> j & 1:
            p = crc_mul(p, sq)
        sq = crc_mul(sq, sq)
    return p


def crc_raw(piece, c):
    for x in piece:
        c = TABLE[(c ^ x) & 0xFF] ^ (c >> 8)
    return c


def crc32_pieces(data, lanes=256):
    """the CRC-32 of data as the device computes it: lane t runs the table CRC over [t * piece, (t + 1) * piece), piece =
    ceil(len / lanes), from 0 (lane 0 from 0xFFFFFFFF); its register times x^(8 * the bytes behind the piece); the XOR of all,
    complemented"""
    data = bytes(data)
    n = len(data)
    assert n > 0
    piece = -(-n // lanes)
    acc = 0
    for t in range(lanes):
        beg, end = min(t * piece, n), min((t + 1) * piece, n)
        c = crc_raw(data[beg:end], 0xFFFFFFFF if t == 0 else 0)
        if end > beg and end < n:
            c = crc_mul(c, crc_x8n(n - end))
        acc ^= c
    return acc ^ 0xFFFFFFFF
