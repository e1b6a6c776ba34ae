"""(no GPU) tests/classify_big_model.py against tests/stage_model.py and the CPU oracle, the claims of
tests/classify_big_cases.py, and that the planted runs can catch a fold that is wrong: this is what makes the model the
reference of tests/test_classify_big_gpu.py and its texts worth their size."""
import collections

import numpy as np
import pytest

from tests import classify_big_cases as bc
from tests import classify_big_model as bm
from tests import stage_cases as sc
from tests import stage_model as sm

T = bm.TILE
STAGE_TEXTS = sc.BIG_TEXTS + sc.TINY_TEXTS + ("tandem", "deep", "genome120k")


def same_as_stage_model(S, windows, ks):
    M = bm.Model(S)
    assert np.array_equal(M.types(), sm._types(S).astype(bool))
    assert np.array_equal(M.lms, sm.lms(S))
    for k in ks:
        assert bm.depth(S.size, k) == sm.depth_of(S.size, k)
        for lo, hi in windows:
            assert M.counts13(k, lo, hi) == sm.counts13(S, k, lo, hi), (k, lo, hi)
            keys, pos, m_far = sm.local_list(S, k, lo, hi)
            mine = M.window(lo, hi)
            assert np.array_equal(mine, pos) and M.far_count(k, mine) == m_far, (k, lo, hi)
            assert np.array_equal(M.keys(mine), keys), (k, lo, hi)
    # the single-position forms
    ends = np.append(M.starts[1:], S.size) - 1
    q = np.arange(S.size)
    if S.size > 20_000:  # a sample, and both ends of every run
        q = np.unique(np.concatenate([np.random.default_rng(S.size).integers(0, S.size, 3000), M.starts[::7], ends[::7]]))
    assert np.array_equal(bm.types_at(S, q), M.types()[q])
    run = np.searchsorted(M.starts, q, side="right") - 1
    assert np.array_equal(bm.run_end(S, q), ends[run]) and np.array_equal(bm.run_start(S, q), M.starts[run])


@pytest.mark.parametrize("name", STAGE_TEXTS)
def test_model_equals_the_stage_model_on_its_texts(name):
    S = sc.text(name)
    n = S.size
    rng = np.random.default_rng(n)
    cuts = sorted(rng.integers(0, n + 1, 4).tolist())
    wins = {(0, n), (cuts[0], cuts[1]), (cuts[1], cuts[3]), (cuts[2], cuts[2])}
    if name.startswith("runs"):
        wins |= {sc.windows(name, 256)[w] for w in ("lo_inside_long_run", "hi_inside_long_run", "both_inside_long_run", "tail_run")}
    same_as_stage_model(S, sorted(wins), (32, 256, sc.K_EXACT, n - 1, n))


def test_model_equals_the_stage_model_on_random_short_texts():
    rng = np.random.default_rng(2024)
    for i in range(300):
        n = int(rng.integers(1, 201))
        S = rng.integers(0, int(rng.integers(1, 5)), n).astype(np.uint8)
        if i % 3 == 0:  # runs: every base repeated a random number of times
            S = np.repeat(S, rng.integers(1, 9, n))[:n]
        S.setflags(write=False)
        wins = {(0, n)} | {tuple(sorted(rng.integers(0, n + 1, 2).tolist())) for _ in range(3)}
        same_as_stage_model(S, sorted(wins), (32, 124, n - 1, n, sc.K_EXACT))


def test_model_equals_the_oracle_on_a_text_with_a_run_over_a_tile(oracle):
    for name in ("runs_G", "runs_A"):
        S = sc.text(name)
        got, _ = oracle.get_lms(S)
        M = bm.Model(S)
        assert got[-1] == S.size and np.array_equal(got[:-1], M.lms)
        assert bool(M.types()[sc.RUN_LO + 5]) == (name == "runs_G") and sc.RUN_HI - sc.RUN_LO > T


# ---- the split of the fold -----------------------------------------------------------------------------------------------
def test_split_of_the_fold_at_the_thresholds():
    f = bm.Fold(1024)
    assert not f.two_level and f.per == 1 and f.ranges[1023] == (1023, 1024) and not f.empty_threads()
    f = bm.Fold(1025)
    assert f.per == 2 and f.ranges[512] == (1024, 1025) and f.empty_threads() == list(range(513, 1024))
    f = bm.Fold(4096)
    assert not f.two_level and f.per == 4 and not f.empty_threads() and f.thread_of(4095) == 1023
    f = bm.Fold(4097)
    assert f.two_level and f.chunks == 257 and f.per == 1 and f.tiles_of_thread(256) == (4096, 4097) and f.thread_of(4096) == 256
    f = bm.Fold(16 * 1024)
    assert f.two_level and f.chunks == 1024 and f.per == 1
    f = bm.Fold(16 * 1024 + 1)
    assert f.chunks == 1025 and f.per == 2 and f.tiles_of_thread(512) == (16_384, 16_385) and len(f.empty_threads()) == 511


def plain_types_with_cin(S, cin):
    """types tile by tile, each tile from its own bases and its carry-in alone (plain loop)"""
    n, s = S.size, S.tolist()
    t = [0] * n
    for tile in range(bm.tiles_of(n)):
        hi = min((tile + 1) * T, n)
        for i in range(hi - 1, tile * T - 1, -1):
            if i == n - 1:
                t[i] = 0
            elif s[i] != s[i + 1]:
                t[i] = int(s[i] < s[i + 1])
            else:
                t[i] = int(cin[tile]) if i + 1 == hi else t[i + 1]
    return t


@pytest.mark.parametrize("name", ("runs_G", "runs_A", "iid"))
def test_tile_summaries_and_the_change_of_s_count_on_a_small_text(name):
    S = sc.text(name)
    g, p, cin = bm.tile_summaries(S)
    types = sm.types(S)
    assert cin.tolist() == [int(types[(t + 1) * T]) for t in range(cin.size - 1)] + [0]
    assert p.tolist() == [name != "iid" and t == 1 for t in range(p.size)]  # the run of C over tile 1
    assert plain_types_with_cin(S, cin) == types.tolist()
    assert np.array_equal(bm.fold_cin(g, p), cin)
    rng = np.random.default_rng(3)
    for wrong in [~cin, np.zeros_like(cin), np.ones_like(cin)] + [rng.random(cin.size) < 0.5 for _ in range(3)]:
        t = np.array(plain_types_with_cin(S, wrong))
        want = [int(np.count_nonzero((t == 1) & (S == c))) - int(np.count_nonzero((types == 1) & (S == c))) for c in range(4)]
        assert bm.s_count_change(S, cin, wrong) == want


# ---- the five texts ----------------------------------------------------------------------------------------------------
COVERS = {"fold2": dict(two_level=False, per=2, empty_threads=508, count_loops=1, emit_loops=1),
          "fold4_last": dict(two_level=False, per=4, empty_threads=0, count_loops=2, emit_loops=1),
          "two_level_first": dict(two_level=True, per=1, empty_threads=767, count_loops=3, emit_loops=1),
          "emit_loop": dict(two_level=True, per=1, empty_threads=511, count_loops=5, emit_loops=2),
          "two_level_deep": dict(two_level=True, per=2, empty_threads=510, count_loops=9, emit_loops=3)}


@pytest.mark.parametrize("name", bc.TEXTS)
def test_claims(name):
    p = bc.plan(name)
    assert p.n == bc.SIZES[name] and p.tiles == -(-p.n // T)
    got = bc.covers(p)
    assert {k: got[k] for k in COVERS[name]} == COVERS[name], got
    assert got["whole_chunks"] >= 4 and got["whole_threads"] >= (4 if name != "two_level_deep" else 2), got
    assert (p.fold.empty_threads() or [1024])[0] == {"fold2": 516, "fold4_last": 1024, "two_level_first": 257, "emit_loop": 513,
                                                      "two_level_deep": 514}[name]
    for r in p.runs:
        bc.claim(p, r)
    kinds = dict(collections.Counter(r.kind for r in p.runs))
    want = dict(start=1, aligned=10, offset=10, chunk_starts=1, chunk_ends=1, chunk_straddles=1, thread_range=2, pair=2, end=1)
    if p.tiles > bc.HIGH:
        want.update(across_high=1, high=2 if name == "two_level_deep" else 1)
        assert {(q // T >= bc.HIGH, (q % T) // 32 in (0, 255)) for _, q in p.points} == {(True, True)} and len(p.points) >= 2
    assert kinds == want
    for kind in ("aligned", "offset", "thread_range"):
        assert {r.s_type for r in p.runs if r.kind == kind} == {True, False}
    for kind in ("aligned", "offset"):
        assert sorted((r.hi - r.lo) // T for r in p.runs if r.kind == kind) == sorted(bc.LENGTHS * 2)
    for wname, (lo, hi) in bc.windows(p).items():
        assert 0 <= lo < hi <= p.n, wname


@pytest.mark.parametrize("name", bc.TEXTS)
def test_planted_runs_are_what_the_plan_says_and_catch_a_broken_fold(name):
    """on the text at its full size, through the single-position forms of the model (no run table of 10^8 runs)"""
    p = bc.plan(name)
    S = bc.text(name)
    g, prop, cin = bm.tile_summaries(S)
    assert np.array_equal(prop, p.fold.propagate)  # the planted runs' tiles propagate, and no other tile of the text does
    for r in p.runs:
        assert bool(bm.types_at(S, [r.lo])[0]) == r.s_type and bm.run_end(S, [r.lo])[0] == r.hi - 1, r
        assert r.lo == 0 or bm.run_start(S, [r.hi - 1])[0] == r.lo
        if r.s_type and r.lo > 0:
            assert not bm.types_at(S, [r.lo - 1])[0], r   # it starts with an LMS position
        if not r.s_type and r.hi < p.n:
            assert bm.types_at(S, [r.hi])[0], r           # the base behind it is one
    for _, q in p.points:
        assert bm.types_at(S, [q])[0] and not bm.types_at(S, [q - 1])[0]
    assert np.array_equal(bm.fold_cin(g, prop), cin)
    assert bm.s_count_change(S, cin, cin) == [0, 0, 0, 0]
    for broken in ("summary_propagate_as_0", "stops_at_thread_ranges"):
        wrong = bm.fold_cin(g, prop, broken)
        change = bm.s_count_change(S, cin, wrong)
        # both drop carries and make none up: S-type stretches come out L-type, the planted runs of C among them
        assert change[1] <= -T and all(c <= 0 for c in change) and change[3] == 0, (name, broken, change)
        assert not np.any(wrong & ~cin)
    # A thread without tiles that handed on 1: it changes the carry-in of the last tile alone, and the last tile holds base
    # n - 1, which is L-type whatever comes in.  Such threads stand behind the end only, so NO input can show this error
    # (and the `beg >= end` line of k_tile_cin changes nothing that is read: its loops do not run for such a thread).
    wrong = bm.fold_cin(g, prop, "empty_threads_generate")
    differs = np.flatnonzero(wrong != cin).tolist()
    assert differs == ([p.tiles - 1] if p.fold.empty_threads() else []), (name, differs)
    assert (p.n - 1) // T == p.tiles - 1 and bm.s_count_change(S, cin, wrong) == [0, 0, 0, 0]
