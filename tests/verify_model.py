"""Host model of kiss_hip_ctx_verify_sa_dev, written from the comment above kiss_hip_verify_report in include/kiss_hip.h
and the reference's own test property (tests/kiss.cpp:26-28), not from the kernels:

    SA[0] = n, SA is a permutation of [0, n], and for every i >= 1
        bounded k (k < n):  S.substr(SA[i-1], k) <= S.substr(SA[i], k)       (unsigned bytes, a proper prefix is smaller)
        k >= n:             S[a] < S[b] or (S[a] == S[b] and rank[a+1] < rank[b+1]),   a = SA[i-1], b = SA[i],
                            rank = inverse SA; the empty suffix is smaller than everything and may stand at index 0 only.

report(S, SA, k)                  the whole report, every pair looked at.
report_near(S, SA_bad, k, touched) the same verdict for a VALID suffix array modified at the indexes `touched`.
is_suffix_array(S, SA)            the yes/no form of the k >= n proof.
digest(SA)                        the order-sensitive 64-bit sum, restated in numpy uint64 wrap-around arithmetic.

Defined behaviour only.  order_violations is meaningful only when SA is a permutation of [0, n]: the k >= n proof reads
rank[v] for values v that a non-permutation never wrote, so for such an input in exact mode the model returns
order_violations = first_violation = None (and ok = 0, which holds whatever the ranks are); `comparable(model)` lists the
fields a test may compare with the device's report.  The bounded-k comparison needs no ranks and skips pairs with an
entry > n, so there the model states every field for every input.
"""
import numpy as np

K_UNBOUNDED = 0xFFFFFFFF
FIELDS = ("exact", "ok", "sa0_ok", "out_of_range", "duplicates", "order_violations", "first_violation", "tied_pairs",
          "digest")


def digest(SA):
    """sum over i of splitmix64_finaliser((i << 32) ^ SA[i] ^ 0x5851F42D4C957F2D * i), everything modulo 2^64"""
    sa = np.ascontiguousarray(SA, dtype=np.uint32).astype(np.uint64)
    total = 0
    step = 1 << 22
    with np.errstate(over="ignore"):
        for lo in range(0, sa.size, step):
            v = sa[lo:lo + step]
            i = np.arange(lo, lo + v.size, dtype=np.uint64)
            x = (i << np.uint64(32)) ^ v ^ (np.uint64(0x5851F42D4C957F2D) * i)
            x = x + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
            total += int(np.add.reduce(x, dtype=np.uint64))
    return total & 0xFFFFFFFFFFFFFFFF


def permutation_part(SA, n):
    """(out_of_range, duplicates, sa0_ok).  A value that occurs c times is met c - 1 times with its mark already set,
    whatever the visiting order: duplicates = sum over in-range values of (count - 1)."""
    sa = np.ascontiguousarray(SA, dtype=np.uint32)
    assert sa.size == n + 1
    inside = sa[sa <= n]
    out_of_range = int(sa.size - inside.size)
    duplicates = int(inside.size - np.count_nonzero(np.bincount(inside, minlength=n + 1)))
    return out_of_range, duplicates, 1 if int(sa[0]) == n else 0


def _inverse(sa, n):
    rank = np.empty(n + 1, np.uint32)
    rank[sa] = np.arange(n + 1, dtype=np.uint32)
    return rank


def exact_violations(S, SA):
    """indexes i >= 1 (ascending int64 array) at which the k >= n proof fails; SA must be a permutation of [0, n]"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    sa = np.ascontiguousarray(SA, dtype=np.uint32)
    n = S.size
    if n == 0:
        return np.zeros(0, np.int64)
    rank = _inverse(sa, n)
    a, b = sa[:-1], sa[1:]
    a_end, b_end = a == n, b == n
    x, y = S[np.minimum(a, n - 1)], S[np.minimum(b, n - 1)]
    ra, rb = rank[np.minimum(a, n - 1) + 1], rank[np.minimum(b, n - 1) + 1]
    in_order = (x < y) | ((x == y) & (ra < rb))
    bad = b_end | (~a_end & ~in_order)
    return np.flatnonzero(bad).astype(np.int64) + 1


def is_suffix_array(S, sa):
    """linear-time proof: SA[0] = n, a permutation of [0, n], and (S[a], rank[a + 1]) strictly increasing along SA"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    n = S.size
    sa = np.asarray(sa)
    if sa.size != n + 1 or int(sa[0]) != n:
        return False
    if permutation_part(sa, n)[:2] != (0, 0):
        return False
    return exact_violations(S, sa).size == 0


class _LazyBytes:
    """b[p:q] as bytes without copying a multi-megabyte text first"""

    def __init__(self, S):
        self.S = S

    def __getitem__(self, sl):
        return self.S[sl].tobytes()


def _bounded_pairs(b, n, sa, k, idx):
    """(violating indexes, number of tied pairs) among the pairs i in idx, Python bytes compared"""
    viol, tied = [], 0
    for i in idx:
        p, q = int(sa[i - 1]), int(sa[i])
        if p > n or q > n:
            continue
        left, right = b[p:p + k], b[q:q + k]
        if left > right:
            viol.append(i)
        elif left == right and len(left) == k and len(right) == k:
            tied += 1
    return viol, tied


def _assemble(n, k, SA, viol, tied):
    oor, dup, sa0 = permutation_part(SA, n)
    exact = 1 if k >= n else 0
    rep = {"exact": exact, "sa0_ok": sa0, "out_of_range": oor, "duplicates": dup, "tied_pairs": tied, "digest": digest(SA)}
    if viol is None:  # exact mode on a non-permutation: not a function of the input
        rep["order_violations"] = rep["first_violation"] = None
        rep["ok"] = 0
    else:
        rep["order_violations"] = len(viol)
        rep["first_violation"] = int(min(viol)) if len(viol) else 0
        rep["ok"] = 1 if (sa0 and not oor and not dup and not len(viol)) else 0
    return rep


def report(S, SA, k):
    """the report kiss_hip_ctx_verify_sa_dev owes for (S, SA, k), every adjacent pair evaluated"""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    sa = np.ascontiguousarray(SA, dtype=np.uint32)
    n, k = S.size, int(k) & 0xFFFFFFFF
    if k >= n:
        oor, dup, _ = permutation_part(sa, n)
        return _assemble(n, k, sa, None if (oor or dup) else exact_violations(S, sa), 0)
    viol, tied = _bounded_pairs(S.tobytes(), n, sa, k, range(1, n + 1))
    return _assemble(n, k, sa, viol, tied)


def near_pairs(n, touched):
    """the pair indexes i in [1, n] (pair SA[i-1], SA[i]) that contain a touched index"""
    out = set()
    for t in touched:
        for i in (int(t), int(t) + 1):
            if 1 <= i <= n:
                out.add(i)
    return sorted(out)


def report_near(S, SA_bad, k, touched):
    """report() for a VALID suffix array (k-ordered for this k, or exact) modified at the indexes `touched` only.
    Bounded k: a valid array violates nowhere, so only the pairs that contain a touched index are compared; tied_pairs
    is then the count over THOSE pairs (compare differences: bad minus unmodified, both over the same pairs).
    k >= n: a changed rank is read by pairs anywhere in the array, so every pair is evaluated (vectorised)."""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    sa = np.ascontiguousarray(SA_bad, dtype=np.uint32)
    n, k = S.size, int(k) & 0xFFFFFFFF
    if k >= n:
        return report(S, sa, k)
    idx = near_pairs(n, touched)
    b = _LazyBytes(S)
    viol, tied = _bounded_pairs(b, n, sa, k, idx)
    return _assemble(n, k, sa, viol, tied)


def comparable(model):
    """the fields of a model report that are a function of the input (see the module docstring)"""
    return [f for f in FIELDS if model[f] is not None]


def mismatches(device, model, fields=None):
    """[(field, device value, model value)] over the comparable fields"""
    return [(f, device[f], model[f]) for f in (fields or comparable(model)) if device[f] != model[f]]
