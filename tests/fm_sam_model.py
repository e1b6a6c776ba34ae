"""The alignment lines of the SAM output restated as plain Python loops over lines and fields: one definition, field by field, of
what sam_read_lines / sam_pair_lines of kiss_amd/csrc/host/cli_format.hpp print (tests/test_fm_sam_model.py holds the two against
each other byte for byte), together with the rule that says which reads no writer may touch (bad_reads) and the random batches
the test uses.  It is the yardstick for a writer on the device.

A batch is a dict: reads (uint8), read_index (Q + 1), qual (uint8 or None), names (list of bytes), alns ((C, 12) ints in the
order of kiss_hip_aln), cigar (u32 ops), cigar_index (C + 1), hits ((H, 8) ints in the order of kiss_hip_hit), hit_index (Q + 1),
pairs ((Q / 2, 10) ints in the order of kiss_hip_pair, or None), source (C ints or None), first_alns, md (bytes or None),
md_index (H + 1), ref_names (list of bytes; R = its length), bounds (R + 1).

The rules.  Single end: read q has max(1, its hits) lines, its hits in hit order or the FLAG 4 line.  Paired: the lines of mate
1, then of mate 2; of a mate the pair's chosen hit first -- without its own 256 / 2048, with 1, 2, 8, 32, 64 / 128, the pair's MAPQ,
the signed TLEN, YS, YT:Z:CP --, then its other hits in hit order (hit number 0, displaced: 256 and MAPQ 0); a mate that did
not map is ONE line at its partner's place, whatever hits it has.  RNEXT is = when the NAME BYTES of the two records are equal,
so two records of one name give =, and without records every set RNEXT is =.  YR:i:1 only with pairs.  A read is BAD when a hit
of it names an alignment or a record that does not exist, lies in front of its record, has rbeg > rend or rend > L, or when its
pair carries KISS_HIP_PAIR_BAD_INPUT or chooses a hit that is not the read's."""
import numpy as np

NONE = 0xFFFFFFFF
REVERSE, SECONDARY, SUPPLEMENTARY = 1, 2, 4
PROPER, BAD_INPUT = 1, 64
A_RBEG, A_REND, A_TBEG, A_MISM, A_INS, A_DEL = 2, 3, 4, 7, 8, 9
H_ALN, H_FLAGS, H_MAPQ, H_SCORE, H_SUB, H_REF = 0, 1, 2, 3, 4, 7
P_HIT1, P_HIT2, P_FLAGS, P_TLEN, P_MAPQ1, P_MAPQ2 = 0, 1, 2, 3, 7, 8


def _num(x):
    return str(int(x)).encode()


def bad_reads(b):
    """the reads that are BAD, ascending"""
    Q, C, R = len(b["read_index"]) - 1, len(b["alns"]), len(b["ref_names"])
    bad = []
    for q in range(Q):
        L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
        hb, he = int(b["hit_index"][q]), int(b["hit_index"][q + 1])
        is_bad = False
        for h in range(hb, he):
            t = b["hits"][h]
            a, ref = int(t[H_ALN]), int(t[H_REF])
            if a >= C or (R and ref >= R):
                is_bad = True
                continue
            k = b["alns"][a]
            if int(k[A_RBEG]) > int(k[A_REND]) or int(k[A_REND]) > L:
                is_bad = True
            if R and int(k[A_TBEG]) < int(b["bounds"][ref]):
                is_bad = True
        if b["pairs"] is not None:
            pr = b["pairs"][q // 2]
            mine = int(pr[P_HIT2] if q & 1 else pr[P_HIT1])
            if int(pr[P_FLAGS]) & BAD_INPUT:
                is_bad = True
            if mine != NONE and not hb <= mine < he:
                is_bad = True
        if is_bad:
            bad.append(q)
    return bad


def _seq(b, q, reverse):
    codes = [int(c) for c in b["reads"][int(b["read_index"][q]):int(b["read_index"][q + 1])]]
    if reverse:
        return bytes(b"ACGT"[3 - c] if c <= 3 else ord("N") for c in codes[::-1])
    return bytes(b"ACGT"[c] if c <= 3 else ord("N") for c in codes)


def _qual(b, q, reverse):
    if b["qual"] is None:
        return b"*"
    ql = bytes(bytearray(b["qual"][int(b["read_index"][q]):int(b["read_index"][q + 1])]))
    return ql[::-1] if reverse else ql


def _place(b, h):
    """(record name, POS, tbeg) of hit h"""
    R = len(b["ref_names"])
    t = b["hits"][h]
    tbeg = int(b["alns"][int(t[H_ALN])][A_TBEG])
    ref = int(t[H_REF])
    return (b["ref_names"][ref] if R else b"*"), tbeg - (int(b["bounds"][ref]) if R else 0) + 1, tbeg


def unmapped_line(b, q, bits, place):
    f = [b["names"][q], _num(bits | 4), place[0] if place else b"*", _num(place[1] if place else 0), b"0", b"*", b"=" if place else b"*",
         _num(place[1] if place else 0), b"0", _seq(b, q, False), _qual(b, q, False)]
    return b"\t".join(f) + b"\n"


def hit_line(b, q, h, bits=0, place=None, chosen=False, mapq=None, tlen=0, mate_score=None, proper=False, paired=False):
    t = b["hits"][h]
    a, hflags = int(t[H_ALN]), int(t[H_FLAGS])
    k = b["alns"][a]
    L = int(b["read_index"][q + 1]) - int(b["read_index"][q])
    reverse = bool(hflags & REVERSE)
    flag = bits | (16 if reverse else 0)
    if not chosen:
        flag |= (256 if hflags & SECONDARY else 0) | (2048 if hflags & SUPPLEMENTARY else 0)
    rname, pos, _ = _place(b, h)
    cigar = b""
    if int(k[A_RBEG]):
        cigar += _num(k[A_RBEG]) + b"S"
    for x in range(int(b["cigar_index"][a]), int(b["cigar_index"][a + 1])):
        w = int(b["cigar"][x])
        cigar += _num(w >> 4) + (b"MID"[w & 15:(w & 15) + 1] if (w & 15) <= 2 else b"?")
    if L > int(k[A_REND]):
        cigar += _num(L - int(k[A_REND])) + b"S"
    if place is None:
        rnext = b"*"
    elif place[0] == rname:
        rnext = b"="
    else:
        rnext = place[0]
    f = [b["names"][q], _num(flag), rname, _num(pos), _num(t[H_MAPQ] if mapq is None else mapq), cigar, rnext, _num(place[1] if place else 0),
         _num(tlen), _seq(b, q, reverse), _qual(b, q, reverse),
         b"NM:i:" + _num((int(k[A_MISM]) + int(k[A_INS]) + int(k[A_DEL])) & 0xFFFFFFFF)]
    if b["md"] is not None:
        f.append(b"MD:Z:" + bytes(bytearray(b["md"][int(b["md_index"][h]):int(b["md_index"][h + 1])])))
    f.append(b"AS:i:" + _num(t[H_SCORE]))
    if not hflags & SECONDARY:
        f.append(b"XS:i:" + _num(t[H_SUB]))
    if mate_score is not None:
        f.append(b"YS:i:" + _num(mate_score))
    if proper:
        f.append(b"YT:Z:CP")
    if paired and b["source"] is not None and int(b["source"][a]) >= int(b["first_alns"]):
        f.append(b"YR:i:1")
    return b"\t".join(f) + b"\n"


def read_lines(b, q):
    """the lines of read q -> (list of bytes, how many of them are unmapped lines)"""
    hb, he = int(b["hit_index"][q]), int(b["hit_index"][q + 1])
    if b["pairs"] is None:
        if he == hb:
            return [unmapped_line(b, q, 0, None)], 1
        return [hit_line(b, q, h) for h in range(hb, he)], 0
    pr = b["pairs"][q // 2]
    i = q & 1
    chosen = [int(pr[P_HIT1]), int(pr[P_HIT2])]
    mine, other = chosen[i], chosen[1 - i]
    bits = 1 | (128 if i else 64) | (0 if other != NONE else 8)
    if other != NONE and int(b["hits"][other][H_FLAGS]) & REVERSE:
        bits |= 32
    place = _place(b, other) if other != NONE else (_place(b, mine) if mine != NONE else None)
    if mine == NONE:
        return [unmapped_line(b, q, bits, place)], 1
    proper = bool(int(pr[P_FLAGS]) & PROPER)
    tlen = 0
    if other != NONE and int(pr[P_TLEN]):
        ti, to = _place(b, mine)[2], _place(b, other)[2]
        tlen = int(pr[P_TLEN]) if ti < to or (ti == to and i == 0) else -int(pr[P_TLEN])
    out = [hit_line(b, q, mine, bits | (2 if proper else 0), place, True, int(pr[P_MAPQ2] if i else pr[P_MAPQ1]), tlen,
                    int(b["hits"][other][H_SCORE]) if other != NONE else None, proper, True)]
    for h in range(hb, he):
        if h == mine:
            continue
        if h == hb:  # the first hit of the read, displaced by the pair
            out.append(hit_line(b, q, h, bits | 256, place, mapq=0, paired=True))
        else:
            out.append(hit_line(b, q, h, bits, place, paired=True))
    return out, 0


def sam_model(b):
    """-> dict(lines: list of bytes, sam: their concatenation, line_index (CSR over the lines), read_line (the first line of
    every read), report: lines, sam_bytes, unmapped_lines, longest, bad, first_bad); with a bad read only report (bad, first_bad)"""
    bad = bad_reads(b)
    if bad:
        return {"report": {"bad": len(bad), "first_bad": bad[0]}}
    Q = len(b["read_index"]) - 1
    lines, read_line, unmapped = [], [0], 0
    for q in range(Q):
        got, u = read_lines(b, q)
        lines += got
        unmapped += u
        read_line.append(len(lines))
    line_index = [0]
    for ln in lines:
        line_index.append(line_index[-1] + len(ln))
    return {"lines": lines, "sam": b"".join(lines), "line_index": np.array(line_index, np.uint64), "read_line": np.array(read_line, np.uint64),
            "report": {"lines": len(lines), "sam_bytes": line_index[-1], "unmapped_lines": unmapped, "longest": max([len(x) for x in lines] or [0]),
                       "bad": 0, "first_bad": 0}}


# ---- batches -------------------------------------------------------------------------------------------------------------
def ops_for(rng, span, n_ops=None, max_len=None):
    """ops whose M and I lengths add up to span (len << 4 | op); n_ops: exactly that many M / I ops, as far as span allows"""
    if span == 0:
        return []
    parts = int(n_ops) if n_ops else int(rng.integers(1, min(span, 5) + 1))
    parts = max(1, min(parts, span))
    cuts = np.sort(rng.choice(np.arange(1, span), parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
    lens = np.diff(np.concatenate(([0], cuts, [span])))
    out = []
    for j, ln in enumerate(lens):
        out.append(int(ln) << 4 | (j & 1))                       # M, I, M, I, ...
        if n_ops is None and rng.integers(0, 4) == 0:
            out.append(int(rng.integers(1, max_len or 100000)) << 4 | 2)  # a deletion, of 1 to 5 digits
    return out


def make_batch(rng, lengths, n_hits, R=3, paired=False, qual=True, md=True, source=True, names=None, big=False, same_names=False,
               chosen="any", n_ops=None, md_len=None):
    """A valid batch.  lengths: the read lengths; n_hits: the hits of every read; chosen: which hit of a mate the pair takes
    ('first', 'middle', 'last', 'none', 'any'); big: numbers of up to 10 digits; n_ops: the ops of every alignment."""
    Q = len(lengths)
    assert not paired or Q % 2 == 0
    read_index = np.zeros(Q + 1, np.uint64)
    np.cumsum(lengths, out=read_index[1:])
    bases = int(read_index[-1])
    reads = rng.integers(0, 6, bases).astype(np.uint8)
    ref_names = [[b"chrA", b"chrB", b"chrA" if same_names else b"c"][r] for r in range(R)]
    top = (1 << 32) - 4096 if big else 100000
    bounds = np.sort(1 + (top - 2) // R * np.arange(1, R) - rng.integers(0, 1000, R - 1)) if R > 1 else np.zeros(0, np.int64)
    bounds = np.concatenate(([0], bounds, [top])).astype(np.uint64) if R else np.zeros(1, np.uint64)
    H = int(sum(n_hits))
    hit_index = np.zeros(Q + 1, np.uint64)
    np.cumsum(n_hits, out=hit_index[1:])
    order = rng.permutation(H)  # hit h owns alignment order[h]
    alns = np.zeros((H, 12), np.int64)
    hits = np.zeros((H, 8), np.int64)
    op_lists = [None] * H
    score_top = (1 << 30) - 1 if big else 300
    for q in range(Q):
        L = int(lengths[q])
        for j, h in enumerate(range(int(hit_index[q]), int(hit_index[q + 1]))):
            a = int(order[h])
            clip = rng.integers(0, 3)  # none, left, both
            rbeg = 0 if clip == 0 or L < 3 else int(rng.integers(1, max(2, L // 3)))
            rend = L if clip != 2 or L < 3 else int(rng.integers(max(rbeg, L - L // 3), L))
            ref = int(rng.integers(0, R)) if R else 0
            lo, hi = (int(bounds[ref]), int(bounds[ref + 1])) if R else (0, top)
            tbeg = int(rng.choice([lo, hi - 1, int(rng.integers(lo, hi))]))
            alns[a] = [rng.integers(0, score_top), 0, rbeg, rend, tbeg, tbeg + 1, 0, rng.integers(0, 50), rng.integers(0, 9), rng.integers(0, 9), 0, 0]
            op_lists[a] = ops_for(rng, rend - rbeg, n_ops)
            flags = (j + q) & 7 if j else int(rng.integers(0, 2))  # every combination of the three bits
            hits[h] = [a, flags, rng.integers(0, 61), rng.integers(0, score_top + 1), rng.integers(0, score_top + 1), 0, 0, ref]
    cigar_index = np.zeros(H + 1, np.uint64)
    np.cumsum([len(x) for x in op_lists], out=cigar_index[1:])
    cigar = np.array([w for x in op_lists for w in x], np.uint32)
    b = {"reads": reads, "read_index": read_index, "qual": rng.integers(33, 127, bases).astype(np.uint8) if qual else None,
         "names": names if names is not None else [("r%d" % rng.integers(0, 10 ** int(rng.integers(1, 9)))).encode() for _ in range(Q)],
         "alns": alns, "cigar": cigar, "cigar_index": cigar_index, "hits": hits, "hit_index": hit_index, "pairs": None, "source": None,
         "first_alns": 0, "md": None, "md_index": None, "ref_names": ref_names, "bounds": bounds}
    if md:
        strings = []
        for h in range(H):
            n = md_len if md_len is not None else int(rng.integers(0, 12))
            strings.append(bytes(rng.choice(np.frombuffer(b"0123456789ACGT^", np.uint8), n).astype(np.uint8)))
        b["md"] = np.frombuffer(b"".join(strings), np.uint8).copy()
        b["md_index"] = np.zeros(H + 1, np.uint64)
        np.cumsum([len(x) for x in strings], out=b["md_index"][1:])
    if paired:
        if source:
            b["source"] = rng.integers(0, 2 * H + 1, H).astype(np.uint32)
            b["first_alns"] = H
        pairs = np.zeros((Q // 2, 10), np.int64)
        for p in range(Q // 2):
            pick = []
            for q in (2 * p, 2 * p + 1):
                hb, he = int(hit_index[q]), int(hit_index[q + 1])
                how = chosen if chosen != "any" else ["first", "middle", "last", "none"][int(rng.integers(0, 4))]
                if he == hb or how == "none":
                    pick.append(NONE)
                else:
                    pick.append({"first": hb, "middle": (hb + he - 1) // 2, "last": he - 1}[how])
            tlen = int(rng.choice([0, 1, rng.integers(0, 1000), (1 << 32) - 1 if big else 999999]))
            pairs[p] = [pick[0], pick[1], int(rng.integers(0, 2)) | int(rng.integers(0, 32)) << 1 & 62, tlen, 0, 0, 0, rng.integers(0, 61),
                        rng.integers(0, 61), 0]
        b["pairs"] = pairs
    return b


def random_batch(rng):
    """a small batch of every kind: single and paired, with and without qualities, MD, source, R = 0 / 1 / 3, two records of one
    name, every flag combination, chosen hits first, in the middle and last, unmapped mates, both mates unmapped"""
    paired = bool(rng.integers(0, 2))
    Q = int(rng.integers(1, 5)) * (2 if paired else 1)
    lengths = rng.integers(1, 40, Q)
    n_hits = rng.choice([0, 0, 1, 2, 3, 9], Q)
    return make_batch(rng, lengths, n_hits, R=int(rng.choice([0, 1, 3])), paired=paired, qual=bool(rng.integers(0, 2)), md=bool(rng.integers(0, 2)),
                      source=bool(rng.integers(0, 2)), big=bool(rng.integers(0, 4) == 0), same_names=bool(rng.integers(0, 2)))
