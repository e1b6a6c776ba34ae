"""Generators of BAD (and of deliberately still-good) suffix arrays for the tests of kiss_hip_ctx_verify_sa_dev.

Every generator starts from a CORRECT suffix array and returns a Case: (S, SA_bad, k, touched, what_must_hold) where
`touched` lists the SA indexes that differ from the correct array and `what_must_hold` is a dict of report fields whose
value follows from the construction alone (the tests check it against the model on the CPU and against the device on the
GPU; the remaining fields come from tests/verify_model.py).  Plain numpy: no device, no library.
"""
from collections import namedtuple

import numpy as np

K_UNBOUNDED = 0xFFFFFFFF
Case = namedtuple("Case", "S SA k touched what_must_hold")

K_GRID = (1, 7, 8, 9, 31, 32, 33, 250, 256)  # multiples of 8 and not: the 8-byte steps and the byte loop that finishes
DECIDERS = ((0x7F, 0x80), (0x80, 0xFF), (0x7F, 0xFF), (0x00, 0x80))  # (smaller, larger) bytes that decide a pair
SEAMS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)  # wave / workgroup seams


def deciders_for(d):
    """d = 0: the two deciding bytes start the suffixes, and no other byte value of the text may lie between them"""
    return [xy for xy in DECIDERS if d or xy[0] >= 0x7F]


def depths(k):
    """the first-difference depths that matter for order k: k - 9 ... k + 1"""
    return [d for d in range(k - 9, k + 2) if d >= 0]


def naive_sa(S):
    b = np.ascontiguousarray(S, dtype=np.uint8).tobytes()
    n = len(b)
    return np.array([n] + sorted(range(n), key=lambda i: b[i:]), dtype=np.uint32)


def common_prefix(S, p, q):
    n = S.size
    h = 0
    while p + h < n and q + h < n and S[p + h] == S[q + h]:
        h += 1
    return h


def swapped(SA, i, j):
    bad = np.array(SA, dtype=np.uint32, copy=True)
    bad[i], bad[j] = SA[j], SA[i]
    return bad


def _depth_verdict(d, k):
    # the pair is in the wrong order and its first difference (or the end of the shorter one) lies at depth d
    return {"ok": 0, "order_violations": 1} if d < k else {"ok": 1, "order_violations": 0}


def depth_pair_bytes(d, k, where, decider, seed, filler=700):
    """Byte text with exactly two suffixes that start with the marker byte 0x7E: B x ... and B y ... (B = marker + d - 1
    random bytes of 0x40..0x7D, x < y the decider bytes), everything else below 0x40.  They fill the marker's bucket,
    so they are adjacent in the suffix array, and they agree for exactly d bytes.  d = 0: no block, x and y occur once
    each and no other byte value lies between them.
      where = "mid"      both substrings have the full length k
              "near_end" the second copy ends 2 bytes before the text does: its substring is shorter than k (la != lb)
              "prefix"   the text ends with the second copy: that suffix is a proper prefix of the first (depth d: the
                         shorter one ends there), and must come first
    The two are swapped: a violation iff d < k."""
    rng = np.random.default_rng(seed)
    x, y = decider
    fill = lambda m: rng.integers(1, 0x40, m, dtype=np.uint8)  # (0x00 stays free to be a decider)
    B = rng.integers(0x40, 0x7E, d, dtype=np.uint8)
    if d:
        B[0] = 0x7E
    X, Y = np.array([x], np.uint8), np.array([y], np.uint8)
    head = [fill(filler), B, X, fill(max(filler, k + 16)), B]
    if where == "mid":
        tail = [Y, fill(k + 40)]
    elif where == "near_end":
        tail = [Y, fill(2)]
    else:
        assert where == "prefix" and d >= 1
        tail = []
    S = np.concatenate(head + tail)
    p = filler
    q = p + d + 1 + max(filler, k + 16)
    n = S.size
    SA = naive_sa(S)
    # the construction is asserted, not trusted
    i = int(np.flatnonzero(SA == (q if where == "prefix" else p))[0]) + 1
    lo, hi = int(SA[i - 1]), int(SA[i])
    assert {lo, hi} == {p, q}, "the planted pair is not adjacent"
    assert common_prefix(S, p, q) == d, "the planted pair does not agree for exactly d bytes"
    if where == "prefix":
        assert q + d == n and (lo, hi) == (q, p)
    else:
        assert (int(S[p + d]), int(S[q + d])) == (x, y) and (lo, hi) == (p, q)
        assert (n - q < k) == (where == "near_end" and k > d + 3)
    return Case(S, swapped(SA, i - 1, i), k, (i - 1, i), dict(_depth_verdict(d, k), first_violation=i if d < k else 0))


def depth_pair_dna(d, k, seed, sorter, n=1500):
    """DNA codes: two copies of one random block of length d followed by different bases.  Between the two in the
    suffix array every adjacent pair agrees for at least d bases and at least one for exactly d: that one is swapped."""
    rng = np.random.default_rng(seed)
    S = rng.integers(0, 4, max(n, 3 * k + 3 * d + 64), dtype=np.uint8)
    p, q = 100, 100 + d + 1 + k + 50
    S[q:q + d] = S[p:p + d]
    S[q + d] = (S[p + d] + 1 + rng.integers(0, 3)) % 4
    assert common_prefix(S, p, q) == d
    SA = sorter(S, K_UNBOUNDED)
    rank = np.empty(S.size + 1, np.int64)
    rank[SA] = np.arange(S.size + 1)
    lo, hi = sorted((int(rank[p]), int(rank[q])))
    found = [i for i in range(lo + 1, hi + 1) if common_prefix(S, int(SA[i - 1]), int(SA[i])) == d]
    assert found, "no adjacent pair agrees for exactly d bases"
    i = found[0]
    a, b = int(SA[i - 1]), int(SA[i])
    assert a + d < S.size and b + d < S.size and S[a + d] < S[b + d]
    return Case(S, swapped(SA, i - 1, i), k, (i - 1, i), dict(_depth_verdict(d, k), first_violation=i if d < k else 0))


def adjacent_swap(S, SA, k, i):
    """SA[i-1] <-> SA[i].  i = 1 moves the sentinel off index 0."""
    hold = {"duplicates": 0, "out_of_range": 0, "sa0_ok": 0 if i == 1 else 1}
    if i == 1 or k >= S.size:
        hold["ok"] = 0  # a different permutation is not THE suffix array; the sentinel belongs at index 0
    return Case(S, swapped(SA, i - 1, i), k, (i - 1, i), hold)


def far_swap(S, SA, k, i, j):
    assert i != j
    hold = {"duplicates": 0, "out_of_range": 0, "sa0_ok": 0 if min(i, j) == 0 else 1}
    if min(i, j) == 0 or k >= S.size:
        hold["ok"] = 0
    return Case(S, swapped(SA, i, j), k, (i, j), hold)


def tie_runs(S, SA, k, min_entries=2):
    """[(first, last)] SA index ranges (inclusive) of maximal runs of entries whose k-byte substrings are equal and have
    the full length k, longest first"""
    b = np.ascontiguousarray(S, dtype=np.uint8).tobytes()
    n = len(b)
    runs, start = [], None
    for i in range(1, n + 2):
        tied = False
        if i <= n:
            p, q = int(SA[i - 1]), int(SA[i])
            tied = p + k <= n and q + k <= n and b[p:p + k] == b[q:q + k]
        if tied and start is None:
            start = i - 1
        if not tied and start is not None:
            if i - start >= min_entries:
                runs.append((start, i - 1))
            start = None
    return sorted(runs, key=lambda r: r[0] - r[1])


def tie_group_permute(S, SA, k_tie, k, run, how):
    """rotate (by one) or reverse the entries SA[first..last] of a run that agrees through k_tie bases.  For k <= k_tie
    the property still holds; for k >= n the array is no longer the suffix array."""
    first, last = run
    bad = np.array(SA, dtype=np.uint32, copy=True)
    seg = bad[first:last + 1].copy()
    bad[first:last + 1] = np.roll(seg, 1) if how == "rotate" else seg[::-1]
    assert not np.array_equal(bad, SA)
    hold = {"duplicates": 0, "out_of_range": 0, "sa0_ok": 1}
    if k < S.size and k <= k_tie:
        hold.update(ok=1, order_violations=0)
    elif k >= S.size:
        hold["ok"] = 0
    return Case(S, bad, k, tuple(range(first, last + 1)), hold)


def sentinel_swap(S, SA, k, j):
    """SA[0] <-> SA[j]: still a permutation, the sentinel is not first"""
    assert j >= 1
    return Case(S, swapped(SA, 0, j), k, (0, j), {"ok": 0, "sa0_ok": 0, "duplicates": 0, "out_of_range": 0})


def sentinel_twice(S, SA, k, j):
    """the value n also written at index j >= 1 (SA[j] is lost)"""
    assert j >= 1
    bad = np.array(SA, dtype=np.uint32, copy=True)
    bad[j] = S.size
    return Case(S, bad, k, (j,), {"ok": 0, "sa0_ok": 1, "duplicates": 1, "out_of_range": 0})


def sentinel_missing(S, SA, k, replacement):
    """SA[0] overwritten: by a value of the array (a duplicate) or by one that is out of range"""
    n = S.size
    bad = np.array(SA, dtype=np.uint32, copy=True)
    bad[0] = replacement
    assert replacement != n
    inside = replacement <= n
    return Case(S, bad, k, (0,), {"ok": 0, "sa0_ok": 0, "duplicates": 1 if inside else 0,
                                  "out_of_range": 0 if inside else 1})


def duplicate_values(S, SA, k, src, dsts):
    """SA[src] copied over the indexes dsts: len(dsts) + 1 copies of one value"""
    bad = np.array(SA, dtype=np.uint32, copy=True)
    dsts = [int(j) for j in dsts]
    assert src not in dsts and len(set(dsts)) == len(dsts)
    bad[dsts] = SA[src]
    return Case(S, bad, k, tuple(dsts), {"ok": 0, "duplicates": len(dsts), "out_of_range": 0,
                                         "sa0_ok": 0 if 0 in dsts else 1})


def out_of_range_values(S, SA, k, idxs, values):
    n = S.size
    bad = np.array(SA, dtype=np.uint32, copy=True)
    idxs = [int(j) for j in idxs]
    assert len(set(idxs)) == len(idxs) == len(values) and all(n < int(v) <= 0xFFFFFFFF for v in values)
    bad[idxs] = np.array(values, dtype=np.uint32)
    return Case(S, bad, k, tuple(idxs), {"ok": 0, "duplicates": 0, "out_of_range": len(idxs),
                                         "sa0_ok": 0 if 0 in idxs else 1})


def compose(first, *others):
    """several mutations at DISJOINT index sets of one array: the counts of the permutation part add up"""
    bad = np.array(first.SA, dtype=np.uint32, copy=True)
    touched = set(first.touched)
    hold = {"ok": 0, "duplicates": first.what_must_hold.get("duplicates", 0),
            "out_of_range": first.what_must_hold.get("out_of_range", 0), "sa0_ok": first.what_must_hold.get("sa0_ok", 1)}
    for c in others:
        assert c.S is first.S and c.k == first.k and not (touched & set(c.touched))
        idx = list(c.touched)
        bad[idx] = c.SA[idx]
        touched |= set(c.touched)
        hold["duplicates"] += c.what_must_hold.get("duplicates", 0)
        hold["out_of_range"] += c.what_must_hold.get("out_of_range", 0)
        hold["sa0_ok"] &= c.what_must_hold.get("sa0_ok", 1)
    return Case(first.S, bad, first.k, tuple(sorted(touched)), hold)


# ---- the seeded randomised block (tests/test_verify_model.py on the CPU, tests/test_verify_mutations_gpu.py on the GPU)
RANDOM_KS = (1, 2, 7, 8, 9, 31, 32, 33, 250, 256, 1000, K_UNBOUNDED)
RANDOM_BLOCKS, RANDOM_CASES_PER_BLOCK = 8, 40
MUTATION_COUNTS = (0, 0, 0, 1, 1, 2, 3)  # mutations per case
RANDOM_SEED = 7100  # chosen on the CPU so that the model's verdicts meet RANDOM_SHARES (test_verify_model.py asserts it)
RANDOM_SHARES = {"rejected": 0.25, "accepted": 0.25, "exact": 40, "tied": 20}  # shares of all cases / absolute counts


def random_case(rng, dna_sorter, random_text):
    """one (text, k, 0-3 mutations) case: Case with touched = every modified index"""
    n = int(rng.integers(0, 5001)) if rng.integers(0, 4) else int(rng.integers(0, 70))
    k = RANDOM_KS[int(rng.integers(0, len(RANDOM_KS)))]
    if rng.integers(0, 3) == 0:  # random bytes, sometimes with a copy deeper than most k
        S = rng.integers(0, 256, n, dtype=np.uint8) if rng.integers(0, 2) else rng.integers(0x7E, 0x82, n, dtype=np.uint8)
        if n > 700:
            S[n - 300:] = S[10:310]
        SA = naive_sa(S)
    else:
        S = random_text(rng, n) if n else np.zeros(0, np.uint8)
        SA = dna_sorter(S, k)
    bad = np.array(SA, dtype=np.uint32, copy=True)
    touched = set()
    for _ in range(int(rng.choice(MUTATION_COUNTS)) if n >= 8 else 0):
        kind = int(rng.integers(0, 6))
        free = [i for i in rng.permutation(n + 1)[:12].tolist() if i not in touched and i >= 1]
        if len(free) < 4:
            break
        i = free[0]
        if kind == 0 and i - 1 not in touched:  # adjacent swap
            bad[i - 1], bad[i] = bad[i], bad[i - 1]
            touched |= {i - 1, i}
        elif kind == 1:  # far swap
            j = free[1]
            bad[i], bad[j] = bad[j], bad[i]
            touched |= {i, j}
        elif kind == 2 and k < n:  # reverse a tie group (bounded k: still fine)
            runs = tie_runs(S, bad, k)
            runs = [r for r in runs if not (touched & set(range(r[0], r[1] + 1)))]
            if runs:
                first, last = runs[0]
                bad[first:last + 1] = bad[first:last + 1][::-1].copy()
                touched |= set(range(first, last + 1))
        elif kind == 3 and 0 not in touched:  # the sentinel elsewhere
            bad[0], bad[i] = bad[i], bad[0]
            touched |= {0, i}
        elif kind == 4:  # duplicates
            for j in free[1:1 + int(rng.integers(1, 3))]:
                bad[j] = bad[i]
                touched.add(j)
        elif kind == 5:  # out of range
            bad[i] = [n + 1, 0xFFFFFFFF, n + 1 + int(rng.integers(0, 1000))][int(rng.integers(0, 3))]
            touched.add(i)
    return Case(S, bad, k, tuple(sorted(touched)), {})


def shares(models):
    """what RANDOM_SHARES speaks of, counted on model reports"""
    return {"cases": len(models), "rejected": sum(1 for m in models if not m["ok"]),
            "accepted": sum(1 for m in models if m["ok"]), "exact": sum(1 for m in models if m["exact"]),
            "tied": sum(1 for m in models if m["tied_pairs"] > 0)}


def check_shares(sh):
    assert sh["cases"] >= 300, sh
    assert sh["rejected"] >= RANDOM_SHARES["rejected"] * sh["cases"], sh
    assert sh["accepted"] >= RANDOM_SHARES["accepted"] * sh["cases"], sh
    assert sh["exact"] >= RANDOM_SHARES["exact"] and sh["tied"] >= RANDOM_SHARES["tied"], sh


# ---- the case lists of the small and medium families: the CPU tests run them through the model, the GPU tests through
# ---- the device and the model
GEOMETRY_SIZES = (0, 1, 2, 30, 31, 32, 62, 63, 64, 254, 255, 256, 257)  # n + 1 around bitmap words and workgroups
FAMILIES = ("depth_bytes", "depth_dna", "adjacent_swap", "far_swap", "tie_group", "sentinel", "value_faults", "none")


def _bases(dna_sorter, random_text, ks):
    """(name, S, k, correct SA for that k) over DNA texts and one byte text with values on both sides of 0x80"""
    from tests import gen
    rng = np.random.default_rng(4242)
    texts = [("random_text", random_text(rng, 3000), dna_sorter), ("genome_like", gen.genome_like(6000, 11), dna_sorter),
             ("bytes", rng.integers(0x7C, 0x84, 1400, dtype=np.uint8), lambda S, k: naive_sa(S))]
    for name, S, sorter in texts:
        for k in ks:
            yield name, S, k, sorter(S, k)


def cases(family, dna_sorter, random_text):
    """yields (label, Case) for one family"""
    from tests import gen
    if family == "depth_bytes":
        for k in K_GRID:
            for d in depths(k):
                for where in ("mid", "near_end"):
                    for xy in deciders_for(d):
                        yield "k%d d%d %s %02x/%02x" % (k, d, where, xy[0], xy[1]), depth_pair_bytes(d, k, where, xy, 31 * k + d)
                if d:
                    yield "k%d d%d prefix" % (k, d), depth_pair_bytes(d, k, "prefix", DECIDERS[0], 31 * k + d)
    elif family == "depth_dna":
        for k in K_GRID:
            for d in depths(k):
                yield "k%d d%d" % (k, d), depth_pair_dna(d, k, 17 * k + d, dna_sorter)
    elif family == "adjacent_swap":
        for name, S, k, SA in _bases(dna_sorter, random_text, (8, 32, 256, K_UNBOUNDED)):
            n = S.size
            for i in SEAMS + (n - 1, n):
                yield "%s k%d i%d" % (name, k, i), adjacent_swap(S, SA, k, i)
            buckets = [i for i in range(2, n + 1) if S[SA[i - 1]] != S[SA[i]]]  # pairs with different first characters
            assert buckets
            for i in buckets[:2] + buckets[-1:]:
                yield "%s k%d bucket seam i%d" % (name, k, i), adjacent_swap(S, SA, k, i)
    elif family == "far_swap":
        rng = np.random.default_rng(77)
        for name, S, k, SA in _bases(dna_sorter, random_text, (8, 256, K_UNBOUNDED)):
            for _ in range(12):
                i, j = (int(v) for v in rng.choice(S.size + 1, 2, replace=False))
                yield "%s k%d %d<->%d" % (name, k, i, j), far_swap(S, SA, k, i, j)
    elif family == "tie_group":
        rng = np.random.default_rng(78)
        head = rng.integers(0, 4, 4000, dtype=np.uint8)
        texts = [("periodic", gen.periodic(20_000, 171, 4, 5)), ("genome_like", gen.genome_like(40_000, 7)),
                 ("ends_in_its_beginning", np.concatenate([head, rng.integers(0, 4, 3000, dtype=np.uint8), head[:1500]]))]
        for name, S in texts:
            SA = dna_sorter(S, K_UNBOUNDED)
            for k_tie in (32, 256):
                runs = tie_runs(S, SA, k_tie)
                assert runs, "the text has no run of suffixes that agree through %d bases" % k_tie
                for run in runs[:2] + runs[-1:]:
                    for how in ("rotate", "reverse"):
                        for k in (k_tie, 8, K_UNBOUNDED):
                            yield ("%s tie%d k%d %s %d..%d" % (name, k_tie, k, how, run[0], run[1]),
                                   tie_group_permute(S, SA, k_tie, k, run, how))
    elif family == "sentinel":
        for name, S, k, SA in _bases(dna_sorter, random_text, (32, K_UNBOUNDED)):
            n = S.size
            for j in (1, 64, n):
                yield "%s k%d SA[0]<->SA[%d]" % (name, k, j), sentinel_swap(S, SA, k, j)
            for j in (1, 255, n):
                yield "%s k%d n twice, at %d" % (name, k, j), sentinel_twice(S, SA, k, j)
            for v in (int(SA[5]), 0, n - 1, n + 1, 0xFFFFFFFF):
                yield "%s k%d SA[0]=%d" % (name, k, v), sentinel_missing(S, SA, k, v)
    elif family == "value_faults":
        rng = np.random.default_rng(79)
        for name, S, k, SA in _bases(dna_sorter, random_text, (32, K_UNBOUNDED)):
            n = S.size
            for r in (1, 2, 5, 64):
                idx = [int(v) for v in rng.choice(np.arange(1, n + 1), r + 1, replace=False)]
                yield "%s k%d %d copies" % (name, k, r + 1), duplicate_values(S, SA, k, idx[0], idx[1:])
            for values in ([n + 1], [0xFFFFFFFF], [n + 1, 0xFFFFFFFF, n + 7], [n + 1] * 3 + [0x80000000, 0xFFFFFFFE]):
                idx = rng.choice(np.arange(1, n + 1), len(values), replace=False)
                yield "%s k%d out of range %s" % (name, k, values), out_of_range_values(S, SA, k, idx, values)
            dup = duplicate_values(S, SA, k, 7, [900, 901])
            oor = out_of_range_values(S, SA, k, [300, n], [n + 1, 0xFFFFFFFF])
            yield "%s k%d duplicates and out of range" % (name, k), compose(dup, oor)
    elif family == "none":
        rng = np.random.default_rng(80)
        for n in GEOMETRY_SIZES:
            for kind in ("iid", "one_base"):
                S = rng.integers(0, 4, n, dtype=np.uint8) if kind == "iid" else np.full(n, 2, np.uint8)
                for k in (1, 8, 32, K_UNBOUNDED):
                    yield "%s n%d k%d" % (kind, n, k), Case(S, dna_sorter(S, k), k, (), {"ok": 1, "order_violations": 0,
                                                                                      "duplicates": 0, "out_of_range": 0,
                                                                                      "sa0_ok": 1, "first_violation": 0})
    else:
        raise KeyError(family)
