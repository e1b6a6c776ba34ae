"""kiss_hip_stage_classify with a window [lo, hi) and kiss_hip_stage_local_lms against tests/stage_model.py, window by window:
the 13 counters, the sizes, the emitted (key, position) list in its copy form and through the ctx's views.  The windows are
chosen (tests/stage_cases.py: windows, claim), not what an even split of the text happens to give: edges on and next to word
and tile boundaries, inside runs, on LMS positions, around the far/near cut, empty and one-base windows, uneven tilings."""
import numpy as np
import pytest

from tests import gen
from tests import stage_cases as sc
from tests import stage_model as sm
from tests.stage_dev import E_INVALID, VIEW_LOCAL_KEYS, VIEW_LOCAL_POS, Stage

pytestmark = pytest.mark.gpu

MAX_N = 70_001


@pytest.fixture(scope="module")
def st():
    import kiss_amd
    ctx = kiss_amd.Context(max_n=MAX_N, device=0)
    yield Stage(ctx)
    ctx.close()


def check_window(st, S, k, lo, hi, what, model=None, offset=0):
    """one stage_classify call and everything it left behind against the model -> (counters, keys, positions, m_far).
    model / offset: a cut-out of a text too large for the model, (model text, position of its first base)"""
    M = S if model is None else model
    rc, got = st.classify(S, k, lo, hi)
    assert rc == 0, (what, rc)
    want = sm.counts13(M, k if model is None else sc.K_EXACT, lo - offset, hi - offset)
    assert got == want, "%s: counters %s, model %s" % (what, got, want)
    keys, pos, m_far = sm.local_list(M, k if model is None else sc.K_EXACT, lo - offset, hi - offset)
    pos = pos + np.uint32(offset)
    assert st.sizes() == (pos.size, m_far), "%s: sizes %s, model %s" % (what, st.sizes(), (pos.size, m_far))
    got_keys, got_pos = st.copy_list()
    assert np.array_equal(got_pos, pos), what + ": copied positions"
    bad = np.flatnonzero(got_keys != keys)
    assert bad.size == 0, "%s: %d keys differ, first at position %d: %016x, model %016x" % (
        what, bad.size, pos[bad[0]], got_keys[bad[0]], keys[bad[0]])
    assert np.array_equal(st.view(VIEW_LOCAL_POS, pos.size), pos), what + ": positions through the view"
    assert np.array_equal(st.view(VIEW_LOCAL_KEYS, pos.size), keys), what + ": keys through the view"
    return got, keys, pos, m_far


def k_id(k):
    return {sc.K_EXACT: "exact", -1: "n-1", 0: "n"}.get(k, "k%d" % k)


def k_of(S, k):
    return len(S) + k if k <= 0 else k


@pytest.mark.parametrize("k", [32, 256, sc.K_EXACT, -1, 0], ids=k_id)
@pytest.mark.parametrize("name", sc.BIG_TEXTS)
def test_windows(st, name, k):
    S = sc.text(name)
    k = k_of(S, k)
    D = sm.depth_of(S.size, k)
    assert (D == 0) == (k >= S.size) and (k != S.size - 1 or D >= S.size)  # k = n - 1: nothing is far, k = n: everything
    wins = sc.windows(name, k)
    assert ("cut_inside" in wins) == (k in (32, 256))
    for wname, (lo, hi) in wins.items():
        sc.claim(name, k, wname, lo, hi)
        got, keys, pos, m_far = check_window(st, S, k, lo, hi, "%s k=%d %s [%d, %d)" % (name, k, wname, lo, hi))
        if k == S.size - 1:
            assert m_far == 0
        if k >= S.size:
            assert m_far == pos.size


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
@pytest.mark.parametrize("name", sc.BIG_TEXTS)
def test_tilings_add_up_to_the_whole_text(st, name, k):
    S = sc.text(name)
    n = S.size
    whole, wkeys, wpos, wfar = check_window(st, S, k, 0, n, "%s k=%d whole" % (name, k))
    for tname, tiling in sc.tilings(n).items():
        assert tiling[0][0] == 0 and tiling[-1][1] == n and all(a[1] == b[0] for a, b in zip(tiling, tiling[1:]))
        assert any(lo == hi for lo, hi in tiling) and any(hi - lo == 1 for lo, hi in tiling)
        total, keys, pos = [0] * 13, [], []
        for lo, hi in tiling:
            got, gk, gp, gf = check_window(st, S, k, lo, hi, "%s k=%d %s [%d, %d)" % (name, k, tname, lo, hi))
            total = [a + b for a, b in zip(total, got)]
            keys.append(gk)
            pos.append(gp)
        assert total == whole, (name, k, tname)
        # window by window the far ones come first; over the whole text that is one list, the near-end positions at its end
        assert np.array_equal(np.concatenate(pos), wpos) and np.array_equal(np.concatenate(keys), wkeys), (name, k, tname)


@pytest.mark.parametrize("name", sc.TINY_TEXTS)
def test_tiny_texts(st, name):
    S = sc.text(name)
    n = S.size
    assert name != "no_lms" or sm.lms(S).size == 0
    for k in (32, n - 1, n, sc.K_EXACT):
        if k < 1:
            continue
        for lo, hi in sc.tiny_windows(n):
            check_window(st, S, k, lo, hi, "%s k=%d [%d, %d)" % (name, k, lo, hi))


def test_far_cut_on_every_field_of_a_word(st):
    """k = 32: the cut n - 125 on every field of a packed word, the last far or the first near LMS position planted on it"""
    for S, cut, q in sc.far_cut_texts():
        n = S.size
        for lo, hi in ((0, n), (cut - 40, cut + 40), (q, q + 1)):
            got, keys, pos, m_far = check_window(st, S, 32, lo, hi, "cut on field %d, LMS at %d, [%d, %d)" % (cut % 32, q, lo, hi))
            assert q in pos.tolist() and (m_far == pos.tolist().index(q) + (1 if q == cut else 0))


def test_every_second_base_an_lms_position_regrows_the_arrays():
    """(CA)^m: 16 LMS positions in every word, 4096 in a tile, more than a ctx sized for DNA-typical density holds"""
    import kiss_amd
    S = sc.text("CA")
    ctx = kiss_amd.Context(max_n=S.size, device=0, lms_capacity=1000)
    try:
        small = Stage(ctx)
        before = small.capacity()
        m = sm.lms(S).size
        assert m == sc.TILE and before < m
        for lo, hi in ((0, S.size), (31, sc.TILE + 33)):
            check_window(small, S, 256, lo, hi, "(CA)^m on a small ctx [%d, %d)" % (lo, hi))  # (the views are asked for anew)
        assert small.capacity() >= m
    finally:
        ctx.close()


def test_argument_checks(st):
    S = sc.text("iid")
    n = S.size
    assert st.classify(S, 256, 0, n)[0] == 0
    assert st.classify(S, 256, 11, 10)[0] == E_INVALID          # lo > hi
    assert st.classify(S, 256, 0, n + 1)[0] == E_INVALID        # hi > n
    assert st.classify(S, 256, 0, 0, n=0)[0] == E_INVALID       # n = 0
    assert st.classify(S, 256, 0, n, n=MAX_N + 1)[0] == E_INVALID  # n > max_n (refused before anything is read)
    assert st.classify(S, 256, 0, n, counts=False)[0] == E_INVALID
    check_window(st, S, 256, 100, 5000, "after the refused calls")


# ---- the two-level carry: more than 4096 tiles ----------------------------------------------------------------------------
BIG_N = 4096 * sc.TILE + 2 * sc.TILE + 77
CHUNK = 16 * sc.TILE
BIG_RUN = (100 * CHUNK - 20_000, 100 * CHUNK - 20_000 + 300_000)


def cut_out(S, lo, hi):
    """-> (the bases from 12 in front of lo to where the types of [lo, hi) are decided, position of the first one): the next
    base that differs from its successor at or behind hi - 1, and 21 bases behind hi for the keys.  Only the search for that
    base is vectorised; the model then runs its plain loops on the cut-out, 300 000 bases at the most here."""
    ahead = S[hi - 1:hi + 400_000]
    e = hi - 1 + int(np.flatnonzero(ahead[:-1] != ahead[1:])[0])
    a, b = lo - 12, max(e + 2, hi + 21)
    sub = S[a:b].copy()
    sub.setflags(write=False)
    return sub, a


@pytest.mark.parametrize("after", [2, 0], ids=["run_then_G", "run_then_A"])
def test_two_level_carry_across_chunk_boundaries(after):
    import kiss_amd
    lo_run, hi_run = BIG_RUN
    S = gen.iid(BIG_N, 77)
    S[lo_run - 1] = 3
    S[lo_run:hi_run] = 1
    S[hi_run] = after
    S.setflags(write=False)
    assert (BIG_N + 31) // 32 > 4096 * 256  # more than 4096 tiles
    assert sum(1 for c in range(1, BIG_N // CHUNK + 1) if lo_run < c * CHUNK < hi_run) == 3
    ctx = kiss_amd.Context(max_n=BIG_N, device=0)
    try:
        big = Stage(ctx)
        wins = {"left_of_the_run": (lo_run - 3000, lo_run), "across_its_left_end": (lo_run - 2000, lo_run + 2000),
                "inside_the_run": (lo_run + 100_000, lo_run + 103_000), "across_its_right_end": (hi_run - 2000, hi_run + 2000)}
        for wname, (lo, hi) in wins.items():
            sub, a = cut_out(S, lo, hi)
            got, keys, pos, m_far = check_window(big, S, 256, lo, hi, "%s [%d, %d)" % (wname, lo, hi), model=sub, offset=a)
            if wname == "inside_the_run":  # the type of the whole run comes from the base behind it, three chunks away
                assert got[:4] == [0, 3000, 0, 0] and got[4:8] == [0, 3000 if after == 2 else 0, 0, 0] and pos.size == 0
            else:
                assert pos.size > 100
    finally:
        ctx.close()
