"""Texts for the classification at the sizes where its carry fold changes form (kiss_amd/csrc/classify.hip, kiss_classify),
shared by tests/test_classify_big_model.py (CPU) and tests/test_classify_big_gpu.py.  Every text is an i.i.d. base layer with
planted runs of one base; where a run lies follows from the split of the fold (classify_big_model.Fold), and every run has a
name and a claim() that asserts from that split that it is what the name says.

A run is S-type when the base behind it is greater and L-type when it is smaller.  An S-type run is planted behind a greater
base, so it starts with an LMS position; an L-type run is followed by a smaller base and then a greater one, so the base behind
it is an LMS position.  A fold that drops a carry turns an S-type run into an L-type one, a fold that makes one up does the
opposite: either way s_count moves by the length of the stretch and an LMS position comes or goes."""
import collections
import functools
import os
import re

import numpy as np

from tests import gen
from tests import classify_big_model as bm

T = bm.TILE
CHUNK = bm.TC_CHUNK * T
K_EXACT = 0xFFFFFFFF
KS = (32, 256, K_EXACT)
SIZES = {"fold2": 1030 * T + 37,          # one level, 2 tiles per thread, threads 516..1023 empty
         "fold4_last": 4096 * T,          # the last one-level size: 4 tiles per thread; the count pass loops twice
         "two_level_first": 4096 * T + 1,  # the first two-level size; the last tile holds one base
         "emit_loop": 8195 * T + 77,      # two levels, 513 chunks; the emit pass loops
         "two_level_deep": 16_424 * T + 5}  # 1027 chunks: 2 chunks per thread at the chunk level
TEXTS = tuple(SIZES)
SEEDS = dict(zip(TEXTS, (41, 42, 43, 44, 45)))
LENGTHS = (1, 15, 16, 17, 33)  # tiles: one, and around one and two chunks
HIGH = bm.EMIT_GRID            # a tile from here on is the second tile of its workgroup in the emit pass

Planted = collections.namedtuple("Planted", "name kind lo hi base s_type")
Plan = collections.namedtuple("Plan", "name n tiles fold runs points")


def source_constants():
    """the values this file and the model restate, as they stand in classify.hip"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kiss_amd", "csrc", "classify.hip")).read()

    def one(pattern):
        found = re.findall(pattern, src)
        assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
        return int(found[0])
    return {"CL_THREADS": one(r"constexpr int CL_THREADS = (\d+);"), "TC_CHUNK": one(r"constexpr int TC_CHUNK = (\d+);"),
            "FOLD_THREADS": one(r"const uint64_t chunk = \(tiles \+ \d+\) / (\d+);"),
            "FOLD_THREADS_LAUNCHED": one(r"k_tile_cin, dim3\(1\), dim3\((\d+)\)"),
            "TWO_LEVEL_ABOVE": one(r"if \(tiles > (\d+)\) \{ // two levels"),
            "COUNT_GRID": one(r"wtiles < (\d+) \? wtiles : \1\);\s*hipLaunchKernelGGL\(k_classify<false>"),
            "EMIT_GRID": one(r"wtiles < (\d+) \? wtiles : \1\);\s*hipLaunchKernelGGL\(k_classify<true>")}


assert source_constants() == {"CL_THREADS": T // bm.WORD, "TC_CHUNK": bm.TC_CHUNK, "FOLD_THREADS": bm.FOLD_THREADS,
                              "FOLD_THREADS_LAUNCHED": bm.FOLD_THREADS, "TWO_LEVEL_ABOVE": bm.TWO_LEVEL_ABOVE,
                              "COUNT_GRID": bm.COUNT_GRID, "EMIT_GRID": bm.EMIT_GRID}, source_constants()


def propagate_tiles(lo, hi):
    """the tiles a run [lo, hi) turns into propagate tiles: wholly inside it, and the first base of the next tile too"""
    return range((lo + T - 1) // T, (hi - 1) // T)


@functools.lru_cache(maxsize=None)
def plan(name):
    n = SIZES[name]
    tiles = bm.tiles_of(n)
    shape = bm.Fold(tiles)
    runs = []

    def add(rname, kind, lo, hi, s_type):
        assert 0 <= lo < hi <= n and all(hi + 4 <= r.lo or r.hi + 4 <= lo for r in runs), (name, rname)  # their edges apart
        runs.append(Planted(rname, kind, lo, hi, (0 if lo == 0 or kind == "pair" else 1) if s_type else 2, s_type))

    add("start", "start", 0, 2 * T + T // 2, True)
    cur = 4
    for L in LENGTHS:
        for s in (True, False):
            add("aligned%d%s" % (L, "SL"[not s]), "aligned", cur * T, (cur + L) * T, s)
            cur += L + 1
    for i, L in enumerate(LENGTHS):
        for s in (True, False):
            lo = cur * T + 1000 + 517 * i
            add("offset%d%s" % (L, "SL"[not s]), "offset", lo, lo + L * T, s)
            cur = (lo + L * T) // T + 2
    c = (cur + bm.TC_CHUNK - 1) // bm.TC_CHUNK + 1
    add("chunk_starts", "chunk_starts", c * CHUNK, c * CHUNK + 5 * T + 300, True)
    add("chunk_ends", "chunk_ends", (c + 1) * CHUNK - 4 * T - 700, (c + 1) * CHUNK, False)
    add("chunk_straddles", "chunk_straddles", (c + 2) * CHUNK - 2 * T - 500, (c + 2) * CHUNK + 3 * T + 500, True)
    cur = (c + 2) * bm.TC_CHUNK + 6
    unit = shape.per * (bm.TC_CHUNK if shape.two_level else 1)  # tiles of one thread's range
    L = 100 if name == "two_level_deep" else 2 * unit + 2
    for s in (True, False):
        b = (cur + unit) // unit * unit + unit  # a tile on which a thread's range begins
        lo = b * T - (unit // 2) * T - T // 3
        add("thread_range" + "SL"[not s], "thread_range", lo, lo + L * T, s)
        cur = (lo + L * T) // T + 2
    lo = cur * T + 777
    add("pair_A", "pair", lo, lo + 20 * T, True)    # A then C then A: S-type, L-type, nothing between them
    runs.append(Planted("pair_C", "pair", lo + 20 * T, lo + 40 * T, 1, False))
    cur = (lo + 40 * T) // T + 2
    points = []
    if tiles > HIGH:
        assert cur < HIGH - 40
        add("across_high", "across_high", (HIGH - 1) * T + T // 2, HIGH * T + 3, False)  # (the base behind it: an LMS position)
        add("high_in_tile", "high", HIGH * T + 3000, HIGH * T + 7000, True)
        points += [("first_word", HIGH * T + 20), ("last_base", (HIGH + 1) * T - 1)]
    if name == "two_level_deep":
        add("high_whole", "high", 8300 * T + 99, 8317 * T + 1234, True)
        points += [("first_base", 16_000 * T), ("last_base_2", 16_001 * T - 1), ("end_of_first_word", 16_400 * T + 31),
                   ("start_of_last_word", 16_401 * T - 32)]
    add("end", "end", (tiles - 3) * T + 4000, n, False)
    covered = [t for r in runs for t in propagate_tiles(r.lo, r.hi)]
    assert len(covered) == len(set(covered))
    return Plan(name, n, tiles, bm.Fold(tiles, covered), tuple(runs), tuple(points))


def text(name):
    """the text (not kept: the caller holds the largest one only as long as it needs it)"""
    p = plan(name)
    S = gen.iid(p.n, SEEDS[name])
    for r in p.runs:
        S[r.lo:r.hi] = r.base
        if r.lo > 0 and r.name != "pair_C":
            S[r.lo - 1] = r.base + 2 if r.s_type else 0  # S-type: behind a greater base; L-type: behind another base
        if r.hi < p.n and r.name != "pair_A":
            S[r.hi] = r.base + 1 if r.s_type else r.base - 1
            if not r.s_type and r.name != "pair_C":
                S[r.hi + 1] = 3
        if r.name == "pair_C":
            S[r.hi + 1] = 1  # ... C A C: the A behind the pair is an LMS position
    for _, q in p.points:
        S[q - 1:q + 2] = (3, 0, 1)
    S.setflags(write=False)
    return S


def run_of(p, pos):
    """the planted run that holds pos, or None"""
    return next((r for r in p.runs if r.lo <= pos < r.hi), None)


def where(p, pos):
    """for a failure message: the tile and chunk of a position and the planted run it lies in"""
    r = run_of(p, int(pos))
    return "position %d, tile %d, chunk %d, thread %d of the fold, %s" % (
        pos, pos // T, pos // CHUNK, p.fold.thread_of(int(pos) // T), "in run " + r.name if r else "in no planted run")


def claim(p, r):
    """the run is what its name says: the tiles it turns into propagate tiles and the boundaries it crosses (from the split)"""
    f = p.fold
    prop = list(propagate_tiles(r.lo, r.hi))
    assert all(f.propagate[t] for t in prop)
    chunks_crossed = [c for c in range(1, f.chunks) if r.lo < c * CHUNK < r.hi]
    threads = sorted({f.thread_of(t) for t in prop})
    if r.kind == "aligned":
        L = (r.hi - r.lo) // T
        assert r.lo % T == 0 and r.hi % T == 0 and L in LENGTHS and len(prop) == L - 1
    elif r.kind == "offset":
        assert r.lo % T and r.hi % T and (r.hi - r.lo) // T in LENGTHS and (r.hi - r.lo) % T == 0
        assert len(prop) == (r.hi - r.lo) // T - 1  # its whole tiles
    elif r.kind == "chunk_starts":
        assert r.lo % CHUNK == 0 and r.hi % T and not chunks_crossed and len(prop) == 5
    elif r.kind == "chunk_ends":
        assert r.hi % CHUNK == 0 and r.lo % T and not chunks_crossed and len(prop) == 3
        assert f.chunk_of(prop[-1]) == r.hi // CHUNK - 1 and prop[-1] % bm.TC_CHUNK == bm.TC_CHUNK - 2
    elif r.kind == "chunk_straddles":
        assert len(chunks_crossed) == 1 and r.lo % T and r.hi % T
        assert {f.chunk_of(t) for t in prop} == {chunks_crossed[0] - 1, chunks_crossed[0]}
    elif r.kind == "thread_range":
        assert r.lo % T and r.hi % T
        if p.name == "two_level_deep":  # several chunks per thread: whole ranges of threads in the middle of it
            assert r.hi - r.lo == 100 * T and len(threads) >= 4 and f.per == 2 and len(chunks_crossed) >= 6
            assert sum(1 for t in f.whole_threads() if t in threads) >= 2
        else:
            assert len(threads) >= 3 and any(t in f.whole_threads() for t in threads)
    elif r.kind == "pair":
        other = next(o for o in p.runs if o.kind == "pair" and o is not r)
        first, second = sorted((r, other), key=lambda x: x.lo)
        assert first.hi == second.lo and (first.base, second.base) == (0, 1) and first.s_type and not second.s_type
        assert first.hi - first.lo == second.hi - second.lo == 20 * T and len(prop) == 19
        # the two meet inside a tile: that tile stops the carry of the second run, and nothing else lies between them
        assert not f.propagate[first.hi // T] and f.propagate[first.hi // T - 1] and f.propagate[first.hi // T + 1]
    elif r.kind == "end":
        assert r.hi == p.n and not r.s_type and (p.n - 1) // T - r.lo // T + 1 >= 3 and len(prop) >= 1
        assert prop[-1] == p.tiles - 2 and (p.n % T != 0 or p.name == "fold4_last")  # the last tile: partial where n allows
    elif r.kind == "start":
        assert r.lo == 0 and r.hi >= 2 * T and prop[0] == 0 and len(prop) >= 2
    elif r.kind == "high":
        assert r.lo >= HIGH * T
    else:
        assert r.kind == "across_high" and r.lo < HIGH * T < r.hi and r.lo // T == HIGH - 1
    return prop


def covers(p):
    """what the text as a whole has to reach in the form its size runs (asserted by the CPU tests)"""
    f = p.fold
    return {"two_level": f.two_level, "per": f.per, "empty_threads": len(f.empty_threads()),
            "whole_chunks": len(f.whole_chunks()), "whole_threads": len(f.whole_threads()),
            "count_loops": -(-p.tiles // bm.COUNT_GRID), "emit_loops": -(-p.tiles // bm.EMIT_GRID)}


def windows(p):
    """-> {name: (lo, hi)}"""
    n = p.n
    r = next((x for x in p.runs if x.name == "high_in_tile"), None) or next(x for x in p.runs if x.name == "thread_rangeS")
    mid = (r.lo + r.hi) // 2
    w = {"lo_inside_run": (mid, min(n, r.hi + 3 * T + 5)), "hi_inside_run": (r.lo - 2 * T - 7, mid + 1),
         "long_from_tile_1": (T + 11, n - 7), "chunk_to_chunk": (3 * CHUNK, (p.fold.chunks - 2) * CHUNK)}
    assert r.lo < w["lo_inside_run"][0] < r.hi - 1 and r.lo < w["hi_inside_run"][1] - 1 < r.hi - 1
    assert (r.lo // T >= HIGH) == (p.tiles > HIGH)  # beyond tile 8192 wherever the text has such tiles
    lo, hi = w["long_from_tile_1"]
    assert lo // T == 1 and ((hi - 1) // T - lo // T + 1 > bm.EMIT_GRID) == (p.tiles > HIGH)
    assert all(x % CHUNK == 0 for x in w["chunk_to_chunk"])
    return w


def key_sample(p, pos):
    """indices into the ascending LMS list `pos` whose keys are compared on the larger texts: within 64 bases of an edge of a
    planted run, in the first or last word of a tile, and every 64th"""
    pos = np.asarray(pos, dtype=np.int64)
    pick = np.zeros(pos.size, dtype=bool)
    pick[::64] = True
    word = (pos % T) // bm.WORD
    pick |= (word == 0) | (word == T // bm.WORD - 1)
    for r in p.runs:
        for edge in (r.lo, r.hi):
            a, b = np.searchsorted(pos, [edge - 64, edge + 65])
            pick[a:b] = True
    return np.flatnonzero(pick)
