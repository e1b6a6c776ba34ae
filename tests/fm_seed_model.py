"""Model of the maximal exact match seeds (kiss_hip_fmi_seeds_*).  It knows nothing of the GPU code or of FM-indexes: the
ground truth is the text itself, searched with bytes.find.

Text S: n bases 0..3.  A read R: L >= 1 bytes; 0..3 are bases, any other value is "no base" and no match contains it (the
text holds no such byte, so bytes.find never matches across one).  For an end e in 1..L, ms[e] is the largest
l <= min(e, max_len or e) with R[e - l, e) in S; start[e] = e - ms[e].  e ends a seed iff ms[e] >= min_len and (e == L or
start[e + 1] > start[e]); the seed is (start[e], ms[e]).
"""
import numpy as np


def text_bytes(S):
    return (np.asarray(S, dtype=np.uint8) & 3).tobytes()


def revcomp(R):
    """R'[j] = 3 - R[L - 1 - j]; the complement of a no-base is itself"""
    out = np.asarray(R, dtype=np.uint8)[::-1].copy()
    base = out < 4
    out[base] = 3 - out[base]
    return out


def virtual_reads(reads, both_strands):
    """V = Q, or V = 2 Q with virtual read 2 q = read q and 2 q + 1 = its reverse complement"""
    out = []
    for R in reads:
        R = np.asarray(R, dtype=np.uint8)
        out.append(R)
        if both_strands:
            out.append(revcomp(R))
    return out


class Windows:
    """The same two questions as bytes.find -- does P occur, and where -- answered for short P (at most KMAX bases) from the
    sorted list of the text's windows of that length; longer P go to bytes.find.  Only there to keep the tests quick: a
    failing find reads the whole text.  tests/test_fm_seed_model.py holds it against bytes.find."""
    KMAX = 12

    def __init__(self, S):
        self.S = np.asarray(S, dtype=np.uint8) & 3
        self.T = self.S.tobytes()
        self._tables = {}

    def _table(self, l):
        if l not in self._tables:
            code = np.zeros(self.S.size - l + 1, np.int64)
            for j in range(l):
                code = code * 4 + self.S[j:self.S.size - l + 1 + j]
            order = np.argsort(code, kind="stable")  # equal windows stay in ascending position
            self._tables[l] = (code[order], order)
        return self._tables[l]

    def _span(self, P):
        code = 0
        for c in P:
            if c > 3:
                return None, 0, 0
            code = code * 4 + c
        codes, order = self._table(len(P))
        return order, int(np.searchsorted(codes, code, "left")), int(np.searchsorted(codes, code, "right"))

    def occurs(self, P):
        if 0 < len(P) <= min(self.KMAX, self.S.size):
            _, lo, hi = self._span(P)
            return hi > lo
        return self.T.find(P) >= 0

    def find_all(self, P):
        if 0 < len(P) <= min(self.KMAX, self.S.size):
            order, lo, hi = self._span(P)
            return order[lo:hi].astype(np.int64) if hi > lo else np.zeros(0, np.int64)
        return occurrences(self.T, P)


def ms_of(T, R, max_len=0):
    """ms[e] for e = 1..L as an array of L entries (entry e - 1).  Occurrence is monotone in the length (a suffix of a
    string that occurs occurs), so the length is found by binary search; ms[e] <= ms[e - 1] + 1 bounds it from above.
    T: the text as bytes, or a Windows of it."""
    if isinstance(T, Windows):
        return _ms_of(T.occurs, R, max_len)
    return _ms_of(lambda P: T.find(P) >= 0, R, max_len)


def _ms_of(occurs, R, max_len):
    Rb = np.asarray(R, dtype=np.uint8).tobytes()
    L = len(Rb)
    out = np.zeros(L, np.int64)
    prev = 0
    for e in range(1, L + 1):
        hi = min(e, max_len or e, prev + 1)
        if occurs(Rb[e - hi:e]):
            lo = hi
        elif hi > 1 and occurs(Rb[e - hi + 1:e]):  # (the usual case after a miss: one base shorter)
            lo = hi - 1
        else:
            hi = max(hi - 1, 1)
            lo = 0  # the longest length known to occur; hi: the shortest known not to
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if occurs(Rb[e - mid:e]):
                    lo = mid
                else:
                    hi = mid
        out[e - 1] = prev = lo
    return out


def ms_brute(T, R, max_len=0):
    """the definition, length by length (small reads only)"""
    Rb = np.asarray(R, dtype=np.uint8).tobytes()
    out = np.zeros(len(Rb), np.int64)
    for e in range(1, len(Rb) + 1):
        for l in range(min(e, max_len or e), 0, -1):
            if T.find(Rb[e - l:e]) >= 0:
                out[e - 1] = l
                break
    return out


def seeds_from_ms(ms, min_len):
    """[(start, len)] by the rule, ascending e"""
    L = len(ms)
    out = []
    for e in range(1, L + 1):
        m = int(ms[e - 1])
        if m < min_len:
            continue
        if e == L or (e + 1 - int(ms[e])) > (e - m):
            out.append((e - m, m))
    return out


def seeds_by_enumeration(T, R, min_len, max_len=0):
    """the maximal elements under containment of {substrings of R of length <= max_len that occur in S}, of length
    >= min_len, ascending start (small reads only)"""
    Rb = np.asarray(R, dtype=np.uint8).tobytes()
    L = len(Rb)
    occ = [(s, l) for s in range(L) for l in range(1, min(L - s, max_len or L) + 1) if T.find(Rb[s:s + l]) >= 0]
    have = set(occ)
    cap = max_len or L

    def contained(s, l):  # in another member: one base longer on either side is enough (members are closed under substrings)
        return l < cap and ((s > 0 and (s - 1, l + 1) in have) or (s + l < L and (s, l + 1) in have))
    return sorted((s, l) for s, l in occ if l >= min_len and not contained(s, l))


def occurrences(T, P):
    """every p with T[p, p + len(P)) == P, ascending (overlaps count)"""
    out = []
    p = T.find(P)
    while p >= 0:
        out.append(p)
        p = T.find(P, p + 1)
    return np.array(out, np.int64)


def lf_pairs_of(R, ms, max_len=0):
    """(range, base) pairs a backward search per end evaluates: ms[e] that succeed, and one more that empties the range when
    it stopped neither at the cap, nor at the read's start, nor at a no-base"""
    R = np.asarray(R, dtype=np.uint8)
    total = 0
    for e in range(1, R.size + 1):
        m = int(ms[e - 1])
        total += m
        if m < min(e, max_len or e) and R[e - 1 - m] < 4:
            total += 1
    return total


class Batch:
    """ms of every virtual read of a batch under one max_len; seeds() then applies (min_len, max_occ).  Occurrence lists are
    kept per distinct seed string."""

    def __init__(self, S, reads, both_strands, max_len=0):
        self.W = Windows(S)
        self.T = self.W.T
        self.max_len = max_len
        self.vreads = virtual_reads(reads, both_strands)
        self.Q = len(reads)
        self.V = len(self.vreads)
        self.ms_list = [ms_of(self.W, R, max_len) for R in self.vreads]
        self.ms = np.concatenate(self.ms_list) if self.ms_list else np.zeros(0, np.int64)
        self.bases = int(self.ms.size)
        self.lf_pairs = sum(lf_pairs_of(R, m, max_len) for R, m in zip(self.vreads, self.ms_list))
        self._occ = {}

    def forward_only(self):
        """the same batch without the reverse complements (a batch made with both_strands), nothing searched again"""
        b = object.__new__(Batch)
        b.W, b.T, b.max_len, b.Q, b._occ = self.W, self.T, self.max_len, self.Q, self._occ
        assert self.V == 2 * self.Q
        b.vreads, b.ms_list = self.vreads[::2], self.ms_list[::2]
        b.V = len(b.vreads)
        b.ms = np.concatenate(b.ms_list) if b.ms_list else np.zeros(0, np.int64)
        b.bases = int(b.ms.size)
        b.lf_pairs = sum(lf_pairs_of(R, m, b.max_len) for R, m in zip(b.vreads, b.ms_list))
        return b

    def capped(self, max_len):
        """the same batch under a cap, nothing searched again: occurrence is monotone in the length, so the largest
        l <= min(e, max_len) that occurs is min(max_len, the largest l <= e that occurs)"""
        assert self.max_len == 0 and max_len > 0
        b = object.__new__(Batch)
        b.W, b.T, b.max_len, b.Q, b.V, b._occ, b.vreads = self.W, self.T, max_len, self.Q, self.V, self._occ, self.vreads
        b.ms_list = [np.minimum(m, max_len) for m in self.ms_list]
        b.ms = np.concatenate(b.ms_list) if b.ms_list else np.zeros(0, np.int64)
        b.bases = int(b.ms.size)
        b.lf_pairs = sum(lf_pairs_of(R, m, max_len) for R, m in zip(b.vreads, b.ms_list))
        return b

    def occ(self, P):
        if P not in self._occ:
            self._occ[P] = self.W.find_all(P)
        return self._occ[P]

    def seeds(self, min_len, max_occ):
        """-> dict(start, len, count, seed_index, positions, pos_index, located_seeds, checksum, strings)"""
        start, length, count, sidx, pos, pidx, strings = [], [], [], [0], [], [0], []
        located = npos = checksum = 0
        for R, ms in zip(self.vreads, self.ms_list):
            Rb = R.tobytes()
            for s, l in seeds_from_ms(ms, min_len):
                P = Rb[s:s + l]
                o = self.occ(P)
                start.append(s)
                length.append(l)
                count.append(len(o))
                strings.append(P)
                if max_occ == 0 or len(o) <= max_occ:
                    pos.append(o)
                    npos += len(o)
                    checksum += int(o.sum())
                    located += 1
                pidx.append(npos)
            sidx.append(len(start))
        i64 = lambda x: np.array(x, np.int64)  # noqa: E731
        return {"start": i64(start), "len": i64(length), "count": i64(count), "seed_index": i64(sidx),
                "positions": np.concatenate(pos) if pos else np.zeros(0, np.int64), "pos_index": i64(pidx),
                "located_seeds": located, "checksum": checksum, "strings": strings}
