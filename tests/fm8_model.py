"""Plain numpy / Python model of the FM-index over a byte text (kiss_amd/csrc/fm8.hip), and the brute-force
search its answers are held against.  No GPU, no library: what the device results are compared with.

A hit of a pattern P (length L >= 1) in a text S of n bytes is a position p in [0, n - L] with S[p : p + L] == P;
overlapping hits all count; bytes compare as unsigned values."""
import numpy as np


def brute(S, P):
    """ascending positions of P in S by repeated bytes.find (S, P: bytes)"""
    out, at = [], S.find(P) if len(P) else -1
    while at >= 0:
        out.append(at)
        at = S.find(P, at + 1)
    return out


def brute_batch(S, pats):
    """-> (counts, index (Q + 1), positions, checksum) in the layout of FMIndexBytes.query_batch"""
    per = [brute(S, P) for P in pats]
    counts = np.array([len(x) for x in per], dtype=np.uint64)
    index = np.zeros(len(pats) + 1, np.uint64)
    np.cumsum(counts, out=index[1:])
    positions = np.array([p for x in per for p in x], dtype=np.uint32)
    return counts, index, positions, int(positions.astype(np.uint64).sum())


def exact_sa(S):
    """the exact suffix array in the library's convention: n + 1 entries, SA[0] = n, shorter suffix first on a tie"""
    n = len(S)
    return np.array([n] + sorted(range(n), key=lambda i: S[i:]), dtype=np.uint32)


def exact_sa_doubling(S):
    """the same by prefix doubling in numpy (texts too long, or too repetitive, for sorting slices)"""
    a = np.frombuffer(S, dtype=np.uint8).astype(np.int64)
    n = a.size
    if n == 0:
        return np.zeros(1, np.uint32)
    rank = a + 1
    h = 1
    while True:
        second = np.zeros(n, np.int64)
        if h < n:
            second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        key = rank[order] * (n + 2) + second[order]
        new = np.empty(n, np.int64)
        new[order] = np.concatenate(([0], np.cumsum(key[1:] != key[:-1]))) + 1
        rank = new
        if int(rank.max()) == n:
            break
        h *= 2
    return np.concatenate(([n], np.argsort(rank, kind="stable"))).astype(np.uint32)


def sizes(n, sa_intv, sigma):
    """entries of every array, as kiss_hip_fmi8_sizes_for has them"""
    N = n + 1
    return {"n_sa": N, "bwt_bytes": (N // 256 + 1) * 256, "occ1_entries": sigma * (N // 65536 + 1),
            "occ2_entries": sigma * (N // 256 + 1), "sa_entries": (N + sa_intv - 1) // sa_intv,
            "b_words": 0 if sa_intv == 1 else (N + 63) // 64, "b_occ_entries": 0 if sa_intv == 1 else N // 64 + 1}


class Model:
    """bwt (N bytes, the primary row holds 0), C (257), pri, sigma, map, the sampled SA -- and a backward search on them"""

    def __init__(self, S, sa_intv=4, SA=None):
        S = bytes(S)
        self.S, self.n, self.N, self.sa_intv = S, len(S), len(S) + 1, sa_intv
        self.SA = exact_sa(S) if SA is None else np.asarray(SA, dtype=np.uint32)
        a = np.frombuffer(S, dtype=np.uint8)
        prev = self.SA.astype(np.int64) - 1
        self.pri = int(np.nonzero(self.SA == 0)[0][0])
        self.bwt = np.where(prev >= 0, a[np.maximum(prev, 0)] if self.n else 0, 0).astype(np.uint8)
        hist = np.bincount(a, minlength=256)
        self.C = np.concatenate(([1], 1 + np.cumsum(hist))).astype(np.uint32)
        self.sigma = int((hist > 0).sum())
        self.map = np.full(256, 0xFF, np.uint8)
        self.map[hist > 0] = np.arange(self.sigma, dtype=np.uint8)
        self.sampled = self.SA % sa_intv == 0
        self.sa = self.SA[self.sampled]
        # occ[c][i] = occurrences of byte c in bwt[0, i), the primary row left out (dense: small texts only)
        self._occ = None

    def occ(self, c, i):
        if self._occ is None:
            m = np.zeros((256, self.N + 1), np.int64)
            rows = np.arange(self.N)
            keep = rows != self.pri
            m[self.bwt[keep], rows[keep] + 1] = 1
            self._occ = np.cumsum(m, axis=1)
        return int(self._occ[c, i])

    def search(self, P):
        """(beg, end) of P by backward search; (0, 0) when there is no hit"""
        beg, end = 0, self.N
        for c in reversed(bytes(P)):
            beg, end = int(self.C[c]) + self.occ(c, beg), int(self.C[c]) + self.occ(c, end)
            if beg >= end:
                return 0, 0
        return (beg, end) if len(P) else (0, 0)

    def locate_row(self, row):
        step = 0
        while not self.sampled[row]:
            c = int(self.bwt[row])
            row = int(self.C[c]) + self.occ(c, row)
            step += 1
            assert step < self.sa_intv
        return int(self.SA[row]) + step

    def locate(self, P):
        beg, end = self.search(P)
        return sorted(self.locate_row(r) for r in range(beg, end))


# ---- text families and patterns of the tests ---------------------------------------------------------------------------
def zipf64(n, seed, copies=4):
    """Zipf over 64 symbols (bytes 32..95) with planted repeats: the shape of tools/bench_general.py's text"""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 65)
    a = (rng.choice(64, size=n, p=w / w.sum()) + 32).astype(np.uint8)
    for _ in range(copies if n > 64 else 0):
        ln = int(rng.integers(1, max(2, n // 8)))
        src, dst = (int(x) for x in rng.integers(0, n - ln, 2))
        a[dst:dst + ln] = a[src:src + ln].copy()
    return a.tobytes()


WORDS = (b"the", b"of", b"and", b"suffix", b"array", b"index", b"pattern", b"a", b"in", b"search", b"text", b"byte", b"rank",
         b"is", b"to", b"block", b"count", b"wave", b"lane", b"GPU", b"Burrows", b"Wheeler")


def english_like(n, seed):
    """words from a small vocabulary with spaces, punctuation and line ends"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += WORDS[int(rng.integers(len(WORDS)))]
        out += (b" ", b" ", b" ", b", ", b".\n", b"; ")[int(rng.integers(6))]
    return bytes(out[:n])


def periodic(n, period, seed):
    rng = np.random.default_rng(seed)
    unit = rng.integers(0, 256, period, dtype=np.uint8)
    return np.resize(unit, n).tobytes()


def families(n, seed):
    """name -> text of n bytes"""
    rng = np.random.default_rng(seed)
    return {
        "one_byte": b"\x61" * n,
        "00_ff": rng.choice(np.array([0, 255], np.uint8), size=n).tobytes(),
        "uniform256": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
        "zipf64": zipf64(n, seed),
        "english": english_like(n, seed),
        "period3": periodic(n, 3, seed),
        "period400": periodic(n, 400, seed),
    }


def absent_byte(S):
    present = set(S)
    return next((bytes([v]) for v in range(255, -1, -1) if v not in present), None)


def patterns_for(S, count, seed, max_len=300):
    """ragged patterns, lengths 1..max_len: substrings, substrings with one byte changed, a byte that does not occur, the
    last L bytes, the whole text, a pattern longer than the text"""
    rng = np.random.default_rng(seed)
    n = len(S)
    pats = []
    for i in range(count if n else 0):
        L = int(rng.integers(1, min(max_len, n) + 1)) if i % 3 else int(rng.integers(1, min(8, n) + 1))
        p = int(rng.integers(0, n - L + 1))
        P = bytearray(S[p:p + L])
        if i % 4 == 1:
            j = int(rng.integers(L))
            P[j] = (P[j] + 1 + int(rng.integers(255))) % 256
        pats.append(bytes(P))
    miss = absent_byte(S)
    if miss is not None:
        pats.append(miss)
        if n:
            pats.append(S[:min(n, 5)] + miss + S[:min(n, 3)])
    for L in (1, 2, 17, 300):
        if 1 <= L <= n:
            pats.append(S[n - L:])
    if 1 <= n <= 70000:  # (one lane walks it byte by byte: the 3 * 2^20 text has a test of its own for this one)
        pats.append(S)
    pats.append((S + b"\x00")[:n + 1] if n else b"\x00")
    pats.append(S + S[:1] + b"zz")
    return pats
