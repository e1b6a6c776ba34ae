"""Sequential restatement of the induction stage (kiss_amd/csrc/induce.hip, place.hip) in numpy / plain Python.  TEST ONLY.

  types(S)                   S/L types, ascending LMS positions, the twelve counts kiss_induce takes
  split_near(S, lms, k)      far / near-end LMS positions (classify.hip: far <=> p + D <= n)
  induce(S, lms_order)       the textbook induced sort from ANY order of the LMS suffixes -> (n + 1)-entry SA
  schedule(S, lms_order)     the same result walked segment by segment the way kiss_induce walks it: chain round sizes,
                             pass sizes, and who wrote every SA slot
  ctx_word(S, v, bases)      context word of position v (kiss_internal.hpp: kiss_load_ctx_n)

`induce` is one scan over SA, `schedule` is a sequence of segment passes: two independent forms of one result
(tests/test_induce_model.py holds them against each other, the oracle and a brute-force suffix array).
"""
import numpy as np

STRIDE = 125          # KISS_STRIDE
EMPTY_CTX = 1         # KISS_EMPTY_CTX
CTX_BASES = 15        # KISS_CTX_BASES
BASES = "ACGT"


def types(S):
    """-> (stype, lms, counts12).  stype[i] (i <= n) is True for S-type, the sentinel at n included; lms = ascending LMS
    positions without the sentinel; counts12 = bases | S-type per base | LMS per base (ctx->counts of kiss_induce)."""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    n = S.size
    stype = np.zeros(n + 1, dtype=bool)
    stype[n] = True
    if n:
        # a position has the type of the next position whose base differs from its successor's; the last base is L-type
        nxt = S[1:].astype(np.int16)
        cur = S[:-1].astype(np.int16)
        differs = np.ones(n, dtype=bool)
        differs[:-1] = cur != nxt
        idx = np.where(differs, np.arange(n), n)
        idx = np.minimum.accumulate(idx[::-1])[::-1]          # nearest deciding position at or after i
        decided = np.zeros(n, dtype=bool)
        decided[:-1] = cur < nxt                             # (position n - 1 precedes the sentinel: L-type)
        stype[:n] = decided[idx]
    lms = (np.nonzero(stype[1:n] & ~stype[:n - 1])[0] + 1).astype(np.int64) if n > 1 else np.zeros(0, np.int64)
    counts = np.zeros(12, dtype=np.int64)
    counts[0:4] = np.bincount(S, minlength=4)[:4]
    counts[4:8] = np.bincount(S[stype[:n]], minlength=4)[:4]
    counts[8:12] = np.bincount(S[lms], minlength=4)[:4]
    return stype, lms, [int(x) for x in counts]


def depth_of(n, k):
    """kiss_depth_of (stages.hip): 0 = unbounded"""
    k = int(k) & 0xFFFFFFFF
    return 0 if k >= n else STRIDE * (k // STRIDE + 1)


def split_near(S, lms_positions, k):
    """-> (far, near-end) positions, both in the order given.  A suffix is far when D bases fit behind its start
    (classify.hip: p + depth <= n); with D = 0 all are far, with D > n none is."""
    n = len(S)
    lms = np.asarray(lms_positions, dtype=np.int64)
    D = depth_of(n, k)
    far = np.ones(lms.size, dtype=bool) if D == 0 else lms + D <= n
    return lms[far], lms[~far]


def _layout(S):
    stype, lms, counts = types(S)
    cnt, cntS, cntLMS = counts[0:4], counts[4:8], counts[8:12]
    start = [1]
    for c in range(4):
        start.append(start[c] + cnt[c])
    cntL = [cnt[c] - cntS[c] for c in range(4)]
    return stype, lms, cnt, cntS, cntL, cntLMS, start


def _groups(S, lms_order):
    Sl = S.tolist() if hasattr(S, "tolist") else list(S)
    groups = [[], [], [], []]
    for p in (lms_order.tolist() if hasattr(lms_order, "tolist") else lms_order):
        groups[Sl[p]].append(int(p))
    return groups


def induce(S, lms_order):
    """Induced sort: the LMS suffixes at the tails of their buckets in the order given (stable per first base), one
    left-to-right L scan, the S parts cleared, one right-to-left S scan.  With the exactly (or k-) sorted LMS order the
    result is the (k-ordered) suffix array; with any other order it is the order that order induces."""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    n = S.size
    stype, lms, cnt, cntS, cntL, cntLMS, start = _layout(S)
    assert sorted(int(p) for p in lms_order) == lms.tolist(), "lms_order is not a permutation of the LMS positions"
    Sl, st = S.tolist(), stype.tolist()
    SA = [-1] * (n + 1)
    SA[0] = n
    for c, g in enumerate(_groups(S, lms_order)):
        e = start[c + 1]
        SA[e - len(g):e] = g
    head = start[:4]
    for i in range(n + 1):
        v = SA[i]
        if v > 0 and not st[v - 1]:
            c = Sl[v - 1]
            SA[head[c]] = v - 1
            head[c] += 1
    for c in range(4):
        for i in range(start[c] + cntL[c], start[c + 1]):
            SA[i] = -1
    tail = [start[c + 1] - 1 for c in range(4)]
    for i in range(n, -1, -1):
        v = SA[i]
        if v > 0 and st[v - 1]:
            c = Sl[v - 1]
            SA[tail[c]] = v - 1
            tail[c] -= 1
    out = np.asarray(SA, dtype=np.int64)
    assert out.min() >= 0, "a slot stayed empty"
    return out.astype(np.uint32)


class Schedule:
    """what `schedule` returns.
      chains[(sweep, c)]   round sizes of the self-feeding chain of bucket c in sweep 'L' / 'S' (round 1 = what other
                           segments appended, round t + 1 = what round t appended to its own bucket); [] = empty part
      lms_pass[c]          items of the LMS(c) pass of the L sweep
      l_to_s[c]            items of the L-part(c) pass of the S sweep (c > 0)
      begin[(sweep, c)]    SA index of the first item of the chain's round 1 (where the sweep starts reading the part)
      writer               per SA slot: (sweep, source segment, round of that segment), e.g. ('S', 'S-part(C)', 7)
      writes               per SA slot: how often it was written (once each, or the segments do not tile the array)
      SA                   the result (equal to induce(S, lms_order))"""

    def __init__(self):
        self.chains, self.lms_pass, self.l_to_s, self.begin, self.writer, self.SA = {}, {}, {}, {}, None, None
        self.start, self.cntL, self.cntS, self.cntLMS = None, None, None, None

    def segments(self):
        """non-empty source segments: the sentinel seed, every non-empty chain, every LMS pass, every L -> S pass"""
        return (1 + sum(1 for r in self.chains.values() if r) + sum(1 for v in self.lms_pass.values() if v)
                + sum(1 for v in self.l_to_s.values() if v))

    def part_of(self, slot):
        if slot == 0:
            return "sentinel slot"
        for c in range(4):
            if slot < self.start[c + 1]:
                return ("L-part(%s)" if slot < self.start[c] + self.cntL[c] else "S-part(%s)") % BASES[c]
        return "beyond SA"

    def describe(self, slot):
        w = self.writer[slot]
        if w is None:
            return "slot %d in %s: no writer" % (slot, self.part_of(slot))
        return "%s, slot %d, written in round %d of %s in the %s sweep" % (self.part_of(slot), slot, w[2], w[1], w[0])


def schedule(S, lms_order):
    """The induction as kiss_induce walks it: one pass per source segment, a self-feeding segment in rounds."""
    S = np.ascontiguousarray(S, dtype=np.uint8)
    n = S.size
    stype, lms, cnt, cntS, cntL, cntLMS, start = _layout(S)
    Sl = S.tolist()
    groups = _groups(S, lms_order)
    sch = Schedule()
    sch.start, sch.cntL, sch.cntS, sch.cntLMS = start, cntL, cntS, cntLMS
    SA = [-1] * (n + 1)
    writer = [None] * (n + 1)
    writes = [0] * (n + 1)
    SA[0] = n
    writer[0] = ("L", "start", 0)
    writes[0] = 1

    def emit(items, allowed, pos, step, tag):
        for v in items:
            if v > 0:
                c = Sl[v - 1]
                if allowed[c]:
                    p = pos[c]
                    SA[p] = v - 1
                    writer[p] = tag
                    writes[p] += 1
                    pos[c] = p + step

    # ---- L sweep: sentinel, then per base L-part(c) in rounds and LMS(c)
    pos = start[:4]
    emit([n], [True] * 4, pos, 1, ("L", "sentinel", 1))
    for c in range(4):
        a = start[c]
        sch.begin[("L", c)] = a
        rounds = []
        ge = [x >= c for x in range(4)]
        while pos[c] > a:
            N = pos[c] - a
            rounds.append(N)
            emit(SA[a:a + N], ge, pos, 1, ("L", "L-part(%s)" % BASES[c], len(rounds)))
            a += N
        sch.chains[("L", c)] = rounds
        assert pos[c] == start[c] + cntL[c], "L-part(%s): %d items, the types say %d" % (BASES[c], pos[c] - start[c], cntL[c])
        sch.lms_pass[c] = len(groups[c])
        assert len(groups[c]) == cntLMS[c]
        emit(groups[c], [x > c for x in range(4)], pos, 1, ("L", "LMS(%s)" % BASES[c], 1))
    # ---- S sweep: per base from T down, S-part(c) in rounds and L-part(c)
    pos = [start[c + 1] - 1 for c in range(4)]
    for c in range(3, -1, -1):
        hi = start[c + 1]
        sch.begin[("S", c)] = hi - 1
        rounds = []
        le = [x <= c for x in range(4)]
        while pos[c] + 1 < hi:
            N = hi - (pos[c] + 1)
            rounds.append(N)
            emit(SA[hi - N:hi][::-1], le, pos, -1, ("S", "S-part(%s)" % BASES[c], len(rounds)))
            hi -= N
        sch.chains[("S", c)] = rounds
        assert pos[c] + 1 == start[c] + cntL[c], "S-part(%s): tail %d, the types say %d" % (BASES[c], pos[c] + 1, start[c] + cntL[c])
        sch.l_to_s[c] = cntL[c] if c > 0 else 0
        if c > 0 and cntL[c]:
            emit(SA[start[c]:start[c] + cntL[c]][::-1], [x < c for x in range(4)], pos, -1, ("S", "L-part(%s)" % BASES[c], 1))
    sch.writer = writer
    sch.writes = writes
    sch.SA = np.asarray(SA, dtype=np.int64)
    assert sch.SA.min() >= 0, "a slot stayed empty"
    sch.SA = sch.SA.astype(np.uint32)
    return sch


def ctx_word(S, v, bases=CTX_BASES):
    """context word of position v with up to `bases` (<= 15) preceding bases: marker bit at 2 * b, base v - 1 in bits
    1:0, b = min(bases, v); no base at all = KISS_EMPTY_CTX (kiss_internal.hpp: kiss_load_ctx_n)"""
    assert 0 <= bases <= CTX_BASES
    b = min(int(bases), int(v))
    w = 1 << (2 * b)
    for j in range(b):
        w |= int(S[v - 1 - j]) << (2 * j)
    return w


def ctx_words(S, positions, bases=CTX_BASES):
    """ctx_word for many positions (vectorised); bases: one number or one per position"""
    S = np.asarray(S, dtype=np.uint8)
    v = np.asarray(positions, dtype=np.int64)
    b = np.minimum(np.broadcast_to(np.asarray(bases, dtype=np.int64), v.shape), v)
    w = np.left_shift(np.int64(1), 2 * b)
    for j in range(CTX_BASES):
        have = j < b
        w[have] |= S[v[have] - 1 - j].astype(np.int64) << (2 * j)
    return w.astype(np.uint32)


def run_lengths(S):
    """-> list of (start, length, base) of the maximal runs of one base"""
    S = np.asarray(S)
    if S.size == 0:
        return []
    cut = np.concatenate([[0], np.nonzero(S[1:] != S[:-1])[0] + 1, [S.size]])
    return [(int(a), int(b - a), int(S[a])) for a, b in zip(cut[:-1], cut[1:])]


COLLAPSE_RCAP, COLLAPSE_RCAP_WIDE = 65535, (1 << 22) - 1     # induce.hip: narrow and wide step fields of the closed form


def default_m_cap(max_n):
    """capacity of the per-LMS-suffix arrays of a fresh context (api.hip: default_m_cap); the tied-segment arrays of a
    context this small or this size hold as many, so it is also what bounds a round that may enter the closed form"""
    return min(int(0.32 * max_n) + 4096, max_n // 2 + 2)


def collapse_steps(rounds, t, m_cap, forced_cap=0):
    """step caps of the run_collapse calls for a chain that enters the closed form at round index t: a call on the N
    items of a round takes min(m_cap / N, field width) steps (the forced cap of the hooks build if smaller) and the items
    whose run reaches the cap -- the round that many steps on -- continue; after a call at the narrow width's limit the
    wide field is used"""
    steps, wide = [], False
    while t < len(rounds):
        cap = min(max(m_cap // rounds[t], 1), COLLAPSE_RCAP_WIDE if wide else COLLAPSE_RCAP)
        if 1 <= forced_cap < cap:
            cap = forced_cap
        steps.append(cap)
        t += cap
        wide = cap >= COLLAPSE_RCAP
    return steps


class Routing:
    """how run_pass / run_collapse (induce.hip) route a schedule's segments:
      tile     passes through the tile kernels (count, scan, scatter -- or the look-back form)
      small    segments or chain remainders through the one-workgroup kernel
      chased   chain rounds the one-workgroup kernel processes beyond its first
      steps    per chain that ends in the closed form: ((sweep, base), entry round size, rounds left at entry, step caps
               of its calls)
      closed   number of such chains;  calls = closed-form calls in all;  passes = what stats()["induce_passes"] counts"""

    def __init__(self):
        self.tile = self.small = self.chased = 0
        self.steps = []

    closed = property(lambda self: len(self.steps))
    calls = property(lambda self: sum(len(s[3]) for s in self.steps))
    passes = property(lambda self: self.tile + self.small + self.calls)


def expected_paths(sch, small_max, collapse_n, m_cap, forced_cap=0):
    r = Routing()
    collapse_max = min(collapse_n, m_cap)
    for N in [1] + [v for v in sch.lms_pass.values() if v] + [v for v in sch.l_to_s.values() if v]:
        if N > small_max:
            r.tile += 1
        else:
            r.small += 1
    for key, rounds in sch.chains.items():
        for t, N in enumerate(rounds):
            if N <= collapse_max:
                r.steps.append((key, N, len(rounds) - t, collapse_steps(rounds, t, m_cap, forced_cap)))
                break
            if N <= small_max:
                r.small += 1
                r.chased += len(rounds) - t - 1
                break
            r.tile += 1
    return r


def compare(got, want, sch, what):
    """None when the SAs agree, else a message: configuration, differing slots, the first one, its writer"""
    got = np.asarray(got).astype(np.int64).ravel()
    want = np.asarray(want).astype(np.int64).ravel()
    if got.size != want.size:
        return "%s: %d entries, expected %d" % (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return ("%s: SA differs in %d of %d slots; first difference in %s: library %d, model %d"
            % (what, bad.size, got.size, sch.describe(i) if sch is not None else "slot %d" % i, got[i], want[i]))


# ---- constructed texts (tests/test_induce_model.py checks what each claims; tests/test_induce_paths_gpu.py sorts them) ----
A_, C_, G_, T_ = 0, 1, 2, 3
RUNS_LONG = [15, 16, 17, 1023, 1024, 1025, 2048, 3071, 3072, 3073]
RUNS_SHORT = [15, 16, 17, 100, 255, 256, 257, 299, 300]   # for the forced step caps: cap 1 stays at a few hundred calls


def _full(ln, c):
    return np.full(ln, c, dtype=np.uint8)


def repeat_text(times, seed, n=50_000):
    """every base of an i.i.d. text `times` times: monotone stretches longer than a context word in both sweeps"""
    from tests import gen
    return np.repeat(gen.iid(n // times, seed), times)


def planted_runs(seed, lengths=RUNS_LONG, filler=60_000):
    """i.i.d. filler (60 000 bases in all) with one run of every base at every length planted between its pieces; the
    pieces never lengthen a run; one run starts at position 0, one ends at n"""
    rng = np.random.default_rng(seed)
    runs = [(ln, c) for ln in lengths for c in range(4)]
    order = rng.permutation(len(runs))
    piece = filler // (len(runs) - 1)
    out = []
    for j, r in enumerate(order.tolist()):
        ln, c = runs[r]
        out.append(_full(ln, c))
        if j + 1 < len(runs):
            nxt = runs[order[j + 1]][1]
            f = rng.integers(0, 4, piece, dtype=np.uint8)
            f[0] = (c + 1 + int(rng.integers(0, 3))) % 4          # differs from the run in front of it
            f[-1] = (nxt + 1 + int(rng.integers(0, 3))) % 4       # ... and from the one behind it
            out.append(f)
    return np.concatenate(out)


def staircase(first, run=1500, cycles=4):
    """(T^run G^run C^run A^run) x cycles with one-base separators that differ from both neighbours, beginning with the
    run of `first` (T_ or A_): almost nothing but runs, so rounds of a few items that last `run` steps"""
    cyc = [T_, G_, C_, A_] if first == T_ else [A_, T_, G_, C_]
    seq = cyc * cycles
    out = []
    for j, c in enumerate(seq):
        out.append(_full(run, c))
        if j + 1 < len(seq):
            sep = [x for x in range(4) if x != c and x != seq[j + 1]][j & 1]
            out.append(_full(1, sep))
    return np.concatenate(out)


GIANT = [65_535, 65_536, 70_000]


def giant_runs():
    """G C T^len (three times: L chains), then G C A^len (three times: S chains, each A run in front of a larger base and
    its start an LMS suffix), G.  No other T or A, so round 1 of either chain has three items and the closed form's first
    call is limited by the width of its step field (65 535), not by capacity: the runs that are longer continue wide."""
    out = []
    for c in (T_, A_):
        for ln in GIANT:
            out += [_full(1, G_), _full(1, C_), _full(ln, c)]
    out.append(_full(1, G_))
    return np.concatenate(out)


def four_blocks(reverse=False, ln=500):
    S = np.concatenate([_full(ln, c) for c in range(4)])
    return S[::-1].copy() if reverse else S


def two_letters(a, b, seed, n=20_000):
    return np.where(np.random.default_rng(seed).integers(0, 2, n) == 0, a, b).astype(np.uint8)


def alternating(a, b, times=10_000):
    return np.tile(np.array([a, b], dtype=np.uint8), times)


def tile_edge(x, prefix=0, prefix_base=T_):
    """prefix_base^prefix (CA)^x T^130: x LMS suffixes, all of A, none near the end at k = 32"""
    return np.concatenate([_full(prefix, prefix_base), np.tile(np.array([C_, A_], dtype=np.uint8), x), _full(130, T_)])


NEAR_E = [0, 1, 63, 64, 65, 128, 255, 256, 257, 300]
NEAR_K = 1000   # D = 1125


def near_end_text(E, seed=31, body=40_000):
    """i.i.d. body, T^1200, (CA)^E, G: at k = 1000 exactly the E LMS suffixes of the (CA) tail are near-end ones"""
    from tests import gen
    return np.concatenate([gen.iid(body, seed), _full(1200, T_), np.tile(np.array([C_, A_], dtype=np.uint8), E), _full(1, G_)])


def with_far_tail(S, k=256):
    """S followed by D + 5 T: no LMS suffix is a near-end one at this k"""
    return np.concatenate([np.asarray(S, dtype=np.uint8), _full(depth_of(len(S) + 10_000, k) + 5, T_)])


def shuffled_in_groups(S, lms_order, seed):
    """the LMS order shuffled inside each first-base group (still grouped A, C, G, T)"""
    rng = np.random.default_rng(seed)
    return np.asarray([p for g in _groups(S, lms_order) for p in rng.permutation(np.asarray(g, dtype=np.int64)).tolist()],
                      dtype=np.int64)


def texts():
    """name -> (builder, the k values its GPU cases use); every text of the GPU file"""
    from tests import gen
    t = {
        "iid40k": (lambda: gen.iid(40_000, 101), (32, 256)),
        "genome60k": (lambda: gen.genome_like(60_000, 102), (32, 256)),
        "repeat17": (lambda: repeat_text(17, 103), (256,)),
        "repeat40": (lambda: repeat_text(40, 104), (256,)),
        "planted": (lambda: planted_runs(105), (256,)),
        "planted_short": (lambda: planted_runs(106, RUNS_SHORT), (256,)),
        "stairs_T": (lambda: staircase(T_), (256,)),
        "stairs_A": (lambda: staircase(A_), (256,)),
        "giant": (giant_runs, (256,)),
        "blocks": (four_blocks, (256,)),
        "blocks_rev": (lambda: four_blocks(True), (256,)),
        "AT": (lambda: two_letters(A_, T_, 107), (256,)),
        "CG": (lambda: two_letters(C_, G_, 108), (256,)),
        "AC": (lambda: two_letters(A_, C_, 109), (256,)),
        "ACAC": (lambda: alternating(A_, C_), (256,)),
        "TATA": (lambda: alternating(T_, A_), (256,)),
    }
    for x in (64, 65, 2047, 2048, 2049, 8191, 8192, 8193):
        t["edge%d" % x] = ((lambda x=x: tile_edge(x)), (32,))
    for j in range(16):
        t["edge2049_T%d" % j] = ((lambda j=j: tile_edge(2049, j, T_)), (32,))
        t["edge2049_A%d" % j] = ((lambda j=j: tile_edge(2049, j, A_)), (32,))
    for E in NEAR_E:
        t["near%d" % E] = ((lambda E=E: near_end_text(E)), (NEAR_K,))
    return t
