"""Host models of the LCP array (kiss_hip_ctx_lcp_*): LCP[0] = 0, LCP[i] = lcp of suffixes SA[i-1] and SA[i] (SA[0] = n).

kasai    : plain-Python Kasai over an exact SA (small and medium texts).
brute    : the definition, pair by pair (tiny texts: checks kasai).
lcp_hash_check : an independent vectorised check for large texts.  LCP[i] = L is accepted only if the L-symbol prefixes
           of both suffixes are equal (polynomial prefix hashes under two prime moduli) and the next symbols differ or one
           suffix ends there.  Needs no SA order: it checks whatever pairs SA lists.
"""
import numpy as np


def naive_sa(S):
    b = bytes(np.asarray(S, dtype=np.uint8))
    n = len(b)
    return np.array([n] + sorted(range(n), key=lambda i: b[i:]), dtype=np.uint32)


def brute(S, SA):
    b = bytes(np.asarray(S, dtype=np.uint8))
    n = len(b)
    out = np.zeros(n + 1, dtype=np.uint32)
    for i in range(1, n + 1):
        a, c = int(SA[i - 1]), int(SA[i])
        h = 0
        while a + h < n and c + h < n and b[a + h] == b[c + h]:
            h += 1
        out[i] = h
    return out


def kasai(S, SA):
    b = bytes(np.asarray(S, dtype=np.uint8))
    n = len(b)
    sa = [int(x) for x in SA]
    rank = [0] * (n + 1)
    for r, p in enumerate(sa):
        rank[p] = r
    lcp = [0] * (n + 1)
    h = 0
    for p in range(n):
        r = rank[p]
        q = sa[r - 1]
        if q == n:  # the predecessor is the empty suffix
            h = 0
            continue
        while p + h < n and q + h < n and b[p + h] == b[q + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return np.array(lcp, dtype=np.uint32)


_MODS = (2147483647, 1000000007)  # primes below 2^31: a product of two residues stays below 2^62


def _pow_table(base, count, mod):
    """base^k mod `mod` for k in [0, count), vectorised as (base^65536)^(k >> 16) * base^(k & 65535)"""
    lo = np.empty(65536, dtype=np.int64)
    v = 1
    for k in range(65536):
        lo[k] = v
        v = v * base % mod
    big = v  # base^65536
    nhi = (count >> 16) + 1
    hi = np.empty(nhi, dtype=np.int64)
    v = 1
    for k in range(nhi):
        hi[k] = v
        v = v * big % mod
    k = np.arange(count, dtype=np.int64)
    return hi[k >> 16] * lo[k & 65535] % mod


def lcp_hash_check(S, SA, LCP, seed=1, chunk=1 << 24):
    """True iff every LCP[i] (i >= 1) is the lcp of suffixes SA[i-1], SA[i] (and LCP[0] == 0); raises AssertionError with
    the first bad index otherwise"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    SA = np.asarray(SA, dtype=np.int64)
    LCP = np.asarray(LCP, dtype=np.int64)
    n = S.size
    assert SA.size == n + 1 and LCP.size == n + 1 and int(LCP[0]) == 0
    if n == 0:
        return True
    rng = np.random.default_rng(seed)
    sym = S.astype(np.int64) + 1
    for mod in _MODS:
        base = int(rng.integers(1000, mod - 1))
        inv = pow(base, mod - 2, mod)
        # C[j] = sum_{k < j} sym[k] * base^-k: the hash of S[a, a + L) is (C[a + L] - C[a]) * base^a
        C = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(sym * _pow_table(inv, n, mod) % mod, out=C[1:])  # < n * 2^31: no overflow
        C %= mod
        fwd = _pow_table(base, n + 1, mod)
        for lo in range(1, n + 1, chunk):
            hi = min(n + 1, lo + chunk)
            a, b, L = SA[lo - 1:hi - 1], SA[lo:hi], LCP[lo:hi]
            bad = (a + L > n) | (b + L > n)
            if bad.any():
                raise AssertionError("LCP[%d] runs past the text" % (lo + int(np.argmax(bad))))
            ha = (C[a + L] - C[a]) % mod * fwd[a] % mod
            hb = (C[b + L] - C[b]) % mod * fwd[b] % mod
            bad = ha != hb
            if bad.any():
                raise AssertionError("LCP[%d] too long (prefixes differ)" % (lo + int(np.argmax(bad))))
            ea, eb = a + L, b + L
            end = (ea == n) | (eb == n)
            nxt_a = S[np.minimum(ea, n - 1)]
            nxt_b = S[np.minimum(eb, n - 1)]
            bad = ~end & (nxt_a == nxt_b)
            if bad.any():
                raise AssertionError("LCP[%d] too short (next symbols equal)" % (lo + int(np.argmax(bad))))
    return True
