"""What kiss_classify (kiss_amd/csrc/classify.hip) has to deliver, stated over the RUNS of the text in numpy, so that it can be
evaluated at 10^8 bases: suffix types, LMS positions, the 13 window counters and the emitted keys.  The definitions are those of
tests/stage_model.py (plain Python, a few 10^5 bases at the most), written a second time and held against it by
tests/test_classify_big_model.py; nothing here follows the kernel's bit arithmetic.

A run is a maximal stretch of one base.  Every base of a run has the type of the run: S when the next run's base is greater,
L otherwise, and L for the last run (the sentinel behind the text is smaller than every base).  An LMS position is the start of
an S-type run that follows an L-type run; position 0 has nothing in front of it and is never one.

The second half restates how the carry fold of the classification is SPLIT (not what it computes): which form runs for a
number of tiles, which tiles or chunks each thread of k_tile_cin folds, and the fold itself over (generate, propagate)
summaries in that split, with the three ways of getting it wrong that tests/classify_big_cases.py plants its runs against."""
import numpy as np

TILE = 8192          # bases per classification tile (256 packed words)
WORD = 32
KEY_BASES = 20
KEY_CTX_BASES = 11
STRIDE = 125


def depth(n, k):
    return 0 if k >= n else STRIDE * (k // STRIDE + 1)


def tiles_of(n):
    return (n + TILE - 1) // TILE


# ---- the definitions over runs ------------------------------------------------------------------------------------------
class Model:
    def __init__(self, S):
        S = np.asarray(S, dtype=np.uint8)
        self.S, self.n = S, S.size
        self.starts = np.concatenate([np.zeros(1, np.int64), np.flatnonzero(S[1:] != S[:-1]) + 1])  # first base of every run
        self.bases = S[self.starts]
        self.s_run = np.zeros(self.starts.size, dtype=bool)
        self.s_run[:-1] = self.bases[1:] > self.bases[:-1]
        new = np.zeros(self.starts.size, dtype=bool)
        new[1:] = self.s_run[1:] & ~self.s_run[:-1]
        self.lms = self.starts[new]
        self._types = self._pad = None

    def types(self):
        """True = S-type, one entry per base"""
        if self._types is None:
            self._types = np.repeat(self.s_run, np.diff(np.append(self.starts, self.n)))
        return self._types

    def window(self, lo, hi):
        """the LMS positions p with lo <= p < hi"""
        a, b = np.searchsorted(self.lms, [lo, hi])
        return self.lms[a:b]

    def far_count(self, k, pos):
        """pos ascends: the far ones (p + D <= n; all when D = 0) are a prefix of it"""
        D = depth(self.n, k)
        return int(pos.size if D == 0 else np.searchsorted(pos, self.n - D, side="right"))

    def counts13(self, k, lo, hi):
        """count[c], s_count[c], lms_count[c] (c = A C G T) and the number of far LMS positions of the window [lo, hi)"""
        seg = self.S[lo:hi]
        pos = self.window(lo, hi)
        out = [np.bincount(seg, minlength=4), np.bincount(seg[self.types()[lo:hi]], minlength=4),
               np.bincount(self.S[pos], minlength=4)]
        return [int(x) for part in out for x in part] + [self.far_count(k, pos)]

    def keys(self, pos):
        """the emitted key of every position: 20 bases from p on (A behind the end) in bits 63..24, below them the context
        word -- a marker bit above j = min(p, 11) two-bit fields, base p - i in bits 2i-1 : 2i-2"""
        p = np.asarray(pos, dtype=np.int64)
        if self._pad is None:
            self._pad = np.concatenate([self.S, np.zeros(KEY_BASES, np.uint8)])
        key = np.zeros(p.size, dtype=np.uint64)
        for i in range(KEY_BASES):
            key = (key << np.uint64(2)) | self._pad[p + i].astype(np.uint64)
        word = np.uint64(1) << (2 * np.minimum(p, KEY_CTX_BASES)).astype(np.uint64)
        for i in range(1, KEY_CTX_BASES + 1):
            base = np.where(p >= i, self.S[np.maximum(p - i, 0)], 0).astype(np.uint64)
            word |= base << np.uint64(2 * i - 2)
        return (key << np.uint64(24)) | word


# ---- single positions, without the run table (a text of 10^8 bases costs nothing here) -------------------------------------
def run_end(S, q):
    """the last base of the run that holds q (vectorised over q): windows of growing width until the base changes"""
    n = S.size
    e = np.array(q, dtype=np.int64).reshape(-1)
    todo, w = np.arange(e.size), 64
    while todo.size:
        blk = S[np.minimum(e[todo][:, None] + np.arange(w + 1), n - 1)]
        d = blk[:, 1:] != blk[:, :-1]
        hit = d.any(axis=1)
        e[todo] = np.minimum(e[todo] + np.where(hit, d.argmax(axis=1), w), n - 1)
        todo = todo[~(hit | (e[todo] == n - 1))]
        w = min(2 * w, 1 << 16)
    return e


def run_start(S, q):
    return S.size - 1 - run_end(S[::-1], S.size - 1 - np.asarray(q, dtype=np.int64))


def types_at(S, q):
    e = run_end(S, q)
    return (e < S.size - 1) & (S[np.minimum(e + 1, S.size - 1)] > S[e])


def tile_summaries(S):
    """-> (g, p, cin) per tile.  p: the tile hands its carry-in on unchanged -- its bases and the first base of the next tile
    are one run.  g: what it hands on otherwise, the type of its first base.  cin: what it has to receive, the type of the
    first base of the next tile (nothing behind the last tile: 0)"""
    first = np.arange(tiles_of(S.size), dtype=np.int64) * TILE
    p = run_end(S, first) >= first + TILE
    t = types_at(S, first)
    return t & ~p, p, np.append(t[1:], False)


def s_count_change(S, cin, wrong):
    """the change of s_count[c] when the tiles are classified with the carry-ins `wrong`: a tile takes its carry-in as the
    type of the stretch at its end that is one run with the first base of the next tile (no such stretch: it ignores it)"""
    delta = [0, 0, 0, 0]
    for t in np.flatnonzero(np.asarray(wrong, bool)[:-1] != np.asarray(cin, bool)[:-1]).tolist():
        nxt = (t + 1) * TILE
        if S[nxt - 1] == S[nxt]:
            a = max(int(run_start(S, nxt - 1)[0]), t * TILE)
            delta[int(S[nxt])] += (nxt - a) * (1 if wrong[t] else -1)
    return delta


# ---- how the fold is split (classify.hip: k_tile_cin, k_tile_cin_chunks, k_tile_cin_apply, kiss_classify) --------------------
FOLD_THREADS = 1024      # k_tile_cin: one workgroup, each thread folds ceil(items / 1024) consecutive items
TWO_LEVEL_ABOVE = 4096   # more tiles than this: the items of k_tile_cin are chunks of TC_CHUNK tiles
TC_CHUNK = 16
COUNT_GRID = 2048        # workgroups of the count pass; more tiles: a workgroup loops
EMIT_GRID = 8192         # workgroups of the emit pass


class Fold:
    def __init__(self, tiles, propagate=()):
        self.tiles = tiles
        self.two_level = tiles > TWO_LEVEL_ABOVE
        self.chunks = (tiles + TC_CHUNK - 1) // TC_CHUNK
        self.items = self.chunks if self.two_level else tiles  # what a thread of k_tile_cin folds
        self.per = (self.items + FOLD_THREADS - 1) // FOLD_THREADS
        self.ranges = [(min(t * self.per, self.items), min((t + 1) * self.per, self.items)) for t in range(FOLD_THREADS)]
        self.propagate = np.zeros(tiles, dtype=bool)
        self.propagate[list(propagate)] = True

    def chunk_of(self, tile):
        return tile // TC_CHUNK

    def item_of(self, tile):
        return tile // TC_CHUNK if self.two_level else tile

    def thread_of(self, tile):
        return self.item_of(tile) // self.per

    def tiles_of_thread(self, t):
        a, b = self.ranges[t]
        return (a * TC_CHUNK, min(b * TC_CHUNK, self.tiles)) if self.two_level else (a, b)

    def empty_threads(self):
        return [t for t, (a, b) in enumerate(self.ranges) if a == b]

    def whole(self, bounds):
        """of the given (first, behind) tile ranges, those whose tiles all propagate"""
        return [i for i, (a, b) in enumerate(bounds) if b > a and bool(self.propagate[a:b].all())]

    def whole_chunks(self):
        return self.whole([(c * TC_CHUNK, min((c + 1) * TC_CHUNK, self.tiles)) for c in range(self.chunks)])

    def whole_threads(self):
        return self.whole([self.tiles_of_thread(t) for t in range(FOLD_THREADS)])


BROKEN = ("summary_propagate_as_0", "stops_at_thread_ranges", "empty_threads_generate")


def _summarise(g, p, bounds):
    """(g, p) of every range of items: folded from its last item to its first"""
    G, P = np.zeros(len(bounds), dtype=bool), np.zeros(len(bounds), dtype=bool)
    for i, (a, b) in enumerate(bounds):
        c0, c1 = False, True
        for t in range(b - 1, a - 1, -1):
            c0, c1 = bool(g[t] or (p[t] and c0)), bool(g[t] or (p[t] and c1))
        G[i], P[i] = c0, c1 and not c0
    return G, P


def _apply(g, p, bounds, cins):
    """carry-in of every item, from the carry-in of its range"""
    out = np.zeros(len(g), dtype=bool)
    for (a, b), c in zip(bounds, cins):
        c = bool(c)
        for t in range(b - 1, a - 1, -1):
            out[t] = c
            c = bool(g[t] or (p[t] and c))
    return out


def _threads(g, p, fold, broken, first_summary):
    """k_tile_cin over the items g, p: a summary per thread, one thread folds the summaries, every thread its items"""
    G, P = _summarise(g, p, fold.ranges)
    if broken == "summary_propagate_as_0" and first_summary:
        P[:] = False
    if broken == "empty_threads_generate":
        for t in fold.empty_threads():
            G[t], P[t] = True, False
    cin = _apply(G, P, [(0, FOLD_THREADS)], [False])
    if broken == "stops_at_thread_ranges":
        cin[:] = False
    return _apply(g, p, fold.ranges, cin)


def fold_cin(g, p, broken=None):
    """the carry-in of every tile from the tile summaries, folded in the split that kiss_classify uses for this many tiles.
    broken: one of BROKEN -- the first summary above the tiles (chunks at two levels, thread ranges at one) loses its
    propagate bit; no carry crosses from one thread's range into the next; a thread with no items hands on 1, not its
    carry-in"""
    assert broken is None or broken in BROKEN
    fold = Fold(len(g))
    if not fold.two_level:
        return _threads(g, p, fold, broken, True)
    bounds = [(c * TC_CHUNK, min((c + 1) * TC_CHUNK, fold.tiles)) for c in range(fold.chunks)]
    G, P = _summarise(g, p, bounds)
    if broken == "summary_propagate_as_0":
        P[:] = False
    return _apply(g, p, bounds, _threads(G, P, fold, broken, False))
