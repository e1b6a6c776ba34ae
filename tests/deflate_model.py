"""The DEFLATE encoder of kiss_hip_bgzf_deflate_* (include/kiss_hip_deflate.h) restated as plain loops: one BGZF
block is one deflate block (BFINAL = 1) over the payload's token sequence, coded stored, fixed or dynamic, whichever has the
fewest bits (a tie goes to the lower BTYPE).  The output is a pure function of (data, block_bytes, eof).

  candidates : positions are cut into segments of 256; h(p) = (le32(P[p .. p + 4)) * 0x9E3779B1 mod 2^32) >> 19, defined for
               p + 4 <= L; T[h] = the largest position of an EARLIER segment with that hash.  Position p has at most two candidates:
               T[h(p)] when it exists and p - T[h(p)] <= 32768, and p - 1.
  match      : len(p, q) = the common prefix of P[p ..] and P[q ..], at most min(258, L - p); a match needs len >= 4; the longer
               candidate wins, a tie goes to the smaller distance.
  parse      : greedy from 0, no lazy evaluation.
  codes      : Huffman lengths from the counts: the used symbols sorted by (count, symbol), the two-queue merge that takes the
               leaf when leaf <= internal, the depths; a depth above the limit (15; 7 for the code-length code) halves every
               non-zero count to (c + 1) >> 1 and builds again.  Canonical codes.  No distance symbol in use, or one: symbol 0, or
               that one, gets length 1.
  header     : HLIT / HDIST trimmed (at least 257 / 1), the lengths sent as code-length symbols 0 .. 15 only, HCLEN trimmed.
  bits       : Huffman codes from their most significant bit, everything else from the least; zero padding to a byte.
Only the positions the parse visits need their match, so tokens() looks at those; the table takes every position of a segment
once the segment is parsed."""
import struct
import zlib

import numpy as np

from tests import bam_model as B

SEG = 256
HASH_BITS = 13
HASH_MUL = 0x9E3779B1
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
BGZF_HEAD = bytes.fromhex("1f8b08040000000000ff0600424302") + b"\0"


# ---- symbols -----------------------------------------------------------------------------------------------------------------
def len_symbol(n):
    """match length 3 .. 258 -> (symbol, extra bits, their value)"""
    if n == 258:
        return 285, 0, 0
    k = n - 3
    if k < 8:
        return 257 + k, 0, 0
    nb = k.bit_length() - 3
    return 261 + 4 * nb + ((k >> nb) & 3), nb, k & ((1 << nb) - 1)


def dist_symbol(dist):
    """distance 1 .. 32768 -> (symbol, extra bits, their value)"""
    d = dist - 1
    if d < 4:
        return d, 0, 0
    nb = d.bit_length() - 2
    return 2 * nb + 2 + ((d >> nb) & 1), nb, d & ((1 << nb) - 1)


def ll_extra(sym):
    return 0 if sym < 265 or sym == 285 else (sym - 261) >> 2


def d_extra(sym):
    return 0 if sym < 4 else (sym >> 1) - 1


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # (288 lengths: 286 and 287 take part in the code, never in a stream)
FIXED_D = [5] * 30


# ---- matching ----------------------------------------------------------------------------------------------------------------
def hashes(P):
    """h(p) for every p with p + 4 <= L"""
    a = np.frombuffer(P, np.uint8).astype(np.uint64)
    if a.size < 4:
        return np.zeros(0, np.int64)
    w = a[:-3] | a[1:-2] << np.uint64(8) | a[2:-1] << np.uint64(16) | a[3:] << np.uint64(24)
    return (((w * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def match_len(P, p, q):
    cap = min(MAX_MATCH, len(P) - p)
    n = 0
    while n < cap and P[p + n] == P[q + n]:
        n += 1
    return n


def tokens(P):
    """the token sequence of a payload: an int (a literal) or (len, dist)"""
    L = len(P)
    h = hashes(P)
    T = np.zeros(1 << HASH_BITS, np.int64)   # position + 1, 0: empty
    out = []
    p = 0
    for s0 in range(0, L, SEG):
        s1 = min(s0 + SEG, L)
        while p < s1:
            best, dist = 0, 0
            if p >= 1:
                n = match_len(P, p, p - 1)
                if n >= MIN_MATCH:
                    best, dist = n, 1
            if p + 4 <= L and T[h[p]] and p - (T[h[p]] - 1) <= MAX_DIST:
                q = int(T[h[p]]) - 1
                n = match_len(P, p, q)
                if n >= MIN_MATCH and n > best:   # (a tie stays with the smaller distance)
                    best, dist = n, p - q
            if best:
                out.append((best, dist))
                p += best
            else:
                out.append(P[p])
                p += 1
        hs = h[s0:max(s0, min(s1, L - 3))]
        np.maximum.at(T, hs, np.arange(s0, s0 + hs.size) + 1)
    return out


# ---- codes -------------------------------------------------------------------------------------------------------------------
def huff_depths(counts):
    """the depths of the two-queue merge over the symbols with a non-zero count (at least two of them)"""
    leaves = sorted((c, s) for s, c in enumerate(counts) if c)
    assert len(leaves) >= 2
    n = len(leaves)
    weight = [c for c, _ in leaves]
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for node in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= node or weight[li] <= weight[ii]):
                pick = li
                li += 1
            else:
                pick = ii
                ii += 1
            parent[pick] = node
            w += weight[pick]
        weight.append(w)
    depth = [0] * (2 * n - 1)
    for node in range(2 * n - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    lens = [0] * len(counts)
    for k, (_, s) in enumerate(leaves):
        lens[s] = depth[k]
    return lens


def huff_lengths(counts, limit, rounds=None):
    """code lengths within `limit`: the depths, built again from halved counts while one is too deep.  rounds: a list that receives
    the largest depth of every construction"""
    counts = list(counts)
    while True:
        lens = huff_depths(counts)
        if rounds is not None:
            rounds.append(max(lens))
        if max(lens) <= limit:
            return lens
        counts = [(c + 1) >> 1 if c else 0 for c in counts]


def dist_lengths(counts):
    used = [s for s, c in enumerate(counts) if c]
    if len(used) >= 2:
        return huff_lengths(counts, 15)
    lens = [0] * len(counts)
    lens[used[0] if used else 0] = 1
    return lens


def canonical(lens):
    """RFC 1951 3.2.2 -> the codes, most significant bit first"""
    top = max(lens)
    bl = [0] * (top + 2)
    for n in lens:
        if n:
            bl[n] += 1
    nxt = [0] * (top + 2)
    code = 0
    for b in range(1, top + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, bits):
        """from the least significant bit"""
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        """a Huffman code, from its most significant bit"""
        self.put(int(format(code, "0%db" % bits)[::-1], 2) if bits else 0, bits)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


def counts_of(toks):
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in toks:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])[0]] += 1
            d[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    return ll, d


def token_bits(ll, d, ll_lens, d_lens):
    return sum(c * (ll_lens[s] + ll_extra(s)) for s, c in enumerate(ll)) + sum(c * (d_lens[s] + d_extra(s)) for s, c in enumerate(d))


def plan(P):
    """everything the encoder decides about one payload"""
    L = len(P)
    assert 1 <= L <= B.BLOCK_MAX
    toks = tokens(P)
    ll, d = counts_of(toks)
    rounds = []
    ll_lens = huff_lengths(ll, 15, rounds)
    d_lens = dist_lengths(d)
    hlit = max(257, max(s for s in range(286) if ll_lens[s]) + 1)
    hdist = max(1, max(s for s in range(30) if d_lens[s]) + 1)
    seq = ll_lens[:hlit] + d_lens[:hdist]
    cl = [0] * 19
    for n in seq:
        cl[n] += 1
    cl_lens = huff_lengths(cl, 7)
    hclen = max(4, max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1)
    cost = {0: 40 + 8 * L,
            1: 3 + token_bits(ll, d, FIXED_LL, FIXED_D),
            2: 3 + 14 + 3 * hclen + sum(cl_lens[n] for n in seq) + token_bits(ll, d, ll_lens, d_lens)}
    btype = min(cost, key=lambda b: (cost[b], b))
    return dict(tokens=toks, ll=ll, d=d, ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens, hlit=hlit, hdist=hdist, hclen=hclen, seq=seq,
                cost=cost, btype=btype, first_depth=rounds[0],
                literals=sum(1 for t in toks if not isinstance(t, tuple)), matches=sum(1 for t in toks if isinstance(t, tuple)),
                match_bytes=sum(t[0] for t in toks if isinstance(t, tuple)))


def stream(P, pl=None):
    """the raw deflate stream of one payload"""
    pl = pl or plan(P)
    L = len(P)
    if pl["btype"] == 0:
        return b"\x01" + struct.pack("<HH", L, L ^ 0xFFFF) + bytes(P)
    w = Bits()
    w.put(1, 1)
    w.put(pl["btype"], 2)
    if pl["btype"] == 1:
        ll_lens, d_lens = FIXED_LL, FIXED_D
    else:
        ll_lens, d_lens = pl["ll_lens"], pl["d_lens"]
        cl_codes = canonical(pl["cl_lens"])
        w.put(pl["hlit"] - 257, 5)
        w.put(pl["hdist"] - 1, 5)
        w.put(pl["hclen"] - 4, 4)
        for k in range(pl["hclen"]):
            w.put(pl["cl_lens"][CL_ORDER[k]], 3)
        for n in pl["seq"]:
            w.code(cl_codes[n], pl["cl_lens"][n])
    ll_codes, d_codes = canonical(ll_lens), canonical(d_lens)
    for t in pl["tokens"]:
        if isinstance(t, tuple):
            s, nb, v = len_symbol(t[0])
            w.code(ll_codes[s], ll_lens[s])
            w.put(v, nb)
            s, nb, v = dist_symbol(t[1])
            w.code(d_codes[s], d_lens[s])
            w.put(v, nb)
        else:
            w.code(ll_codes[t], ll_lens[t])
    w.code(ll_codes[256], ll_lens[256])
    got = w.done()
    assert len(got) == -(-pl["cost"][pl["btype"]] // 8)
    return got


def block(P, pl=None):
    """one BGZF block"""
    s = stream(P, pl)
    return BGZF_HEAD + struct.pack("<H", len(s) + 25) + s + struct.pack("<II", zlib.crc32(P) & 0xFFFFFFFF, len(P))


def frame_report(data, block_bytes=0, eof=False):
    """-> (the bytes of out, block_index as a list, the report's counts)"""
    data = bytes(data)
    bb = block_bytes or B.BLOCK_DEFAULT
    assert 1 <= bb <= B.BLOCK_MAX
    out, index = [], [0]
    rep = dict(blocks=0, out_bytes=0, stored_blocks=0, fixed_blocks=0, dynamic_blocks=0, literals=0, matches=0, match_bytes=0)
    for at in range(0, len(data), bb):
        P = data[at:at + bb]
        pl = plan(P)
        out.append(block(P, pl))
        index.append(index[-1] + len(out[-1]))
        rep["blocks"] += 1
        rep[("stored_blocks", "fixed_blocks", "dynamic_blocks")[pl["btype"]]] += 1
        for k in ("literals", "matches", "match_bytes"):
            rep[k] += pl[k]
    got = b"".join(out) + (B.BGZF_EOF if eof else b"")
    rep["out_bytes"] = len(got)
    return got, index, rep


def frame(data, block_bytes=0, eof=False):
    return frame_report(data, block_bytes, eof)[0]
