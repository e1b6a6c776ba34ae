"""Duplicate marking restated as plain Python loops (include/kiss_hip_markdup.h): markdup_model(bam, rec_index,
n_ref, min_qual) -> the marked bytes, dup and the report, or the BAD records.  A second, independent statement of which templates
are duplicates (markdup_by_dicts: dictionaries from end and from pair of ends to lists of templates, max by (score, -index)) is
what tests/test_markdup_model.py holds the loops against.  record() builds one record with tests/bam_model.py's encoder."""
import struct

import numpy as np

from tests import bam_model as B

DUP = 0x400
U5_LIMIT = 1 << 32
MAX_N_REF = (1 << 30) - 1
OPS = "MIDNSHP=X"


def record(name, flag, ref, pos, cigar=(), qual=b"", mapq=0, nref=-1, npos=-1, tlen=0, tags=b"", l_seq=None):
    """one record with its block_size.  name: bytes without the NUL; cigar: (length, op letter or code) pairs; qual: the quality
    bytes, whose count is l_seq (the bases are all 'A')"""
    words = [(int(n) << 4) | (OPS.index(op) if isinstance(op, str) else int(op)) for n, op in cigar]
    L = len(qual) if l_seq is None else l_seq
    reflen = sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8))
    seq = bytes([0x11] * (L // 2) + ([0x10] if L & 1 else []))
    return B._pack(ref, pos, name, mapq, B.reg2bin(pos, pos + max(1, reflen)) if pos >= 0 else 4680, words, flag, L, nref, npos, tlen, seq, bytes(qual), tags)


def join(records):
    """records -> (bam as a uint8 array, rec_index)"""
    ri = [0]
    for r in records:
        ri.append(ri[-1] + len(r))
    return np.frombuffer(b"".join(records), np.uint8).copy(), np.array(ri, np.uint64)


def bad_records(bam, rec_index, n_ref):
    """the BAD records in ascending order, and the parsed fields of the others (None for a BAD one)"""
    raw = bytes(bam)
    ri = [int(x) for x in rec_index]
    n = len(ri) - 1
    bad, fields = [], []
    for r in range(n):
        a, b = ri[r], ri[r + 1]
        is_bad = (r == 0 and a != 0) or (r == n - 1 and b != len(raw)) or b <= a or b > len(raw) or b - a < 36
        f = None
        if not (b <= a or b > len(raw) or b - a < 36):
            size = b - a
            block_size, ref, pos, l_name, _mapq, _bin, n_ops, flag, l_seq = struct.unpack_from("<iiiBBHHHI", raw, a)
            if block_size < 0 or block_size != size - 4 or ref < -1 or ref >= n_ref or pos < -1:
                is_bad = True
            if l_name == 0 or 36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq > size:
                is_bad = True
            if not is_bad:
                at = a + 36
                name = raw[at:at + l_name]
                ops = struct.unpack_from("<%dI" % n_ops, raw, at + l_name)
                q_at = at + l_name + 4 * n_ops + (l_seq + 1) // 2
                if any(w & 15 > 8 for w in ops):
                    is_bad = True
                f = dict(at=a, ref=ref, pos=pos, flag=flag, name=name, ops=ops, qual=raw[q_at:q_at + l_seq])
                if not is_bad and _mapped_primary(f) and not -U5_LIMIT <= u5_of(f) < U5_LIMIT:
                    is_bad = True
        if is_bad:
            bad.append(r)
            f = None
        fields.append(f)
    return bad, fields


def _primary(f):
    return f["flag"] & 0x900 == 0


def _mapped_primary(f):
    return _primary(f) and f["flag"] & 4 == 0 and f["ref"] >= 0


def u5_of(f):
    ops = f["ops"]
    lead = 0
    for w in ops:
        if w & 15 not in (4, 5):
            break
        lead += w >> 4
    trail = 0
    for w in reversed(ops):
        if w & 15 not in (4, 5):
            break
        trail += w >> 4
    reflen = 0
    for w in ops:
        if w & 15 in (0, 2, 3, 7, 8):
            reflen += w >> 4
    if f["flag"] >> 4 & 1:
        return f["pos"] + reflen - 1 + trail
    return f["pos"] - lead


def end_of(f):
    return (f["ref"], u5_of(f), f["flag"] >> 4 & 1)


def templates_of(fields, min_qual):
    """the templates in file order: dict(first, count, cls, ends (sorted for a pair), score)"""
    out = []
    r, n = 0, len(fields)
    while r < n:
        e = r + 1
        while e < n and fields[e]["name"] == fields[r]["name"]:
            e += 1
        score, mapped = 0, []
        for f in fields[r:e]:
            if _primary(f):
                for q in f["qual"]:
                    if min_qual <= q and q != 0xFF:
                        score += q
                if _mapped_primary(f):
                    mapped.append(f)
        if not mapped:
            cls, ends = "none", []
        elif len(mapped) == 1:
            cls, ends = "fragment", [end_of(mapped[0])]
        elif len(mapped) == 2 and sorted(f["flag"] & 0xC0 for f in mapped) == [0x40, 0x80]:
            cls, ends = "pair", sorted(end_of(f) for f in mapped)
        else:
            cls, ends = "ambiguous", []
        out.append(dict(first=r, count=e - r, cls=cls, ends=ends, score=score))
        r = e
    return out


def duplicates_by_loops(tmpl):
    """the indices of the duplicate templates, by plain loops over all of them"""
    dup = set()
    for i, t in enumerate(tmpl):
        if t["cls"] == "pair":
            for j, u in enumerate(tmpl):
                if j != i and u["cls"] == "pair" and u["ends"] == t["ends"] and (u["score"] > t["score"] or (u["score"] == t["score"] and j < i)):
                    dup.add(i)
        elif t["cls"] == "fragment":
            for j, u in enumerate(tmpl):
                if u["cls"] == "pair" and t["ends"][0] in u["ends"]:
                    dup.add(i)
                if j != i and u["cls"] == "fragment" and u["ends"] == t["ends"] and (u["score"] > t["score"] or (u["score"] == t["score"] and j < i)):
                    dup.add(i)
    return dup


def duplicates_by_dicts(tmpl):
    """the same, stated independently: dictionaries from a pair of ends and from an end to the templates there"""
    by_pair, by_end, pair_ends = {}, {}, set()
    for i, t in enumerate(tmpl):
        if t["cls"] == "pair":
            by_pair.setdefault(tuple(t["ends"]), []).append(i)
            pair_ends.update(t["ends"])
        elif t["cls"] == "fragment":
            by_end.setdefault(t["ends"][0], []).append(i)
    dup = set()
    for group in by_pair.values():
        keep = max(group, key=lambda i: (tmpl[i]["score"], -i))
        dup.update(i for i in group if i != keep)
    for end, group in by_end.items():
        if end in pair_ends:
            dup.update(group)
        else:
            keep = max(group, key=lambda i: (tmpl[i]["score"], -i))
            dup.update(i for i in group if i != keep)
    return dup


def markdup_model(bam, rec_index, n_ref, min_qual=15, decide=duplicates_by_loops):
    """-> dict(bam: the marked bytes as uint8, dup: uint8 per record, report, templates, dup_templates); with a BAD record only
    report (bad, first_bad).  n_ref above MAX_N_REF is refused by the call: an assertion here"""
    assert 0 <= n_ref <= MAX_N_REF
    raw = np.array(np.frombuffer(bytes(bam), np.uint8))
    n = len(rec_index) - 1
    bad, fields = bad_records(raw, rec_index, n_ref)
    if bad:
        return {"report": {"records": n, "bad": len(bad), "first_bad": bad[0]}}
    tmpl = templates_of(fields, min_qual)
    dups = decide(tmpl)
    dup = np.zeros(n, np.uint8)
    for i, t in enumerate(tmpl):
        for r in range(t["first"], t["first"] + t["count"]):
            at = fields[r]["at"] + 18
            flag = int(raw[at]) | int(raw[at + 1]) << 8
            flag = flag | DUP if i in dups else flag & ~DUP
            raw[at], raw[at + 1] = flag & 0xFF, flag >> 8
            dup[r] = 1 if i in dups else 0
    count = lambda c: sum(1 for t in tmpl if t["cls"] == c)
    rep = dict(records=n, templates=len(tmpl), pairs=count("pair"), fragments=count("fragment"), unmapped_templates=count("none"),
               ambiguous=count("ambiguous"), dup_pairs=sum(1 for i in dups if tmpl[i]["cls"] == "pair"),
               dup_fragments=sum(1 for i in dups if tmpl[i]["cls"] == "fragment"), dup_records=int(dup.sum()), bad=0, first_bad=0)
    return {"bam": raw, "dup": dup, "report": rep, "templates": tmpl, "dup_templates": sorted(dups)}


def flags_of(bam, rec_index):
    raw = bytes(bam)
    return [struct.unpack_from("<H", raw, int(a) + 18)[0] for a in rec_index[:-1]]
