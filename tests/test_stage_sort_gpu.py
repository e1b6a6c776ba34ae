"""kiss_hip_stage_sort on lists as the exchange of the sharded sort delivers them, against tests/stage_model.py:
(a) the list stage_classify emitted, in place through the ctx's views, (b) the same list through the caller's tensors (copied
in), (c) key-range subsets cut by choose_splitters, (d) a subset put together from the lists of a window tiling, also delivered
into the ctx's buffers, (e) nothing and a single item.  Checked: the order, the returned context words, the taint bits of tied
suffixes, and that stage_induce makes the oracle's suffix array of it.

The digit counts of the classification's emit pass are reused by (a) only for a list of two radix tiles or more, 16 385 items
(radix.hip: `one` and `counted` in kiss_radix_sort, RX_TILE = 16 384); below that (a) and (b) differ by two copies.  The one text
above that size is "genome120k" (25 900 far LMS positions and more): there (a) sorts on the emit pass's counts, (b), the subsets
and the list in the ctx's buffers that is not the counted one sort on counts of their own, and all must give one order.

The taint rule tested (kiss_internal.hpp:90, KISS_CTX_TAINT): a far suffix whose first D bases equal another list member's comes
back from stage_sort with bit 31 set -- the sort compares through D, so it sees every such tie itself (lms_sort.hip:67, "both
suffixes are tainted").  What the placement step adds (place.hip:313, "taint of the far suffixes that TIE with a near-end
suffix") concerns ties with a NEAR-end suffix, which no stage_sort list holds."""
import numpy as np
import pytest

from tests import stage_cases as sc
from tests import stage_model as sm
from tests.stage_dev import (E_DEEP, E_INVALID, VIEW_LOCAL_KEYS, VIEW_LOCAL_POS, VIEW_SORTED, VIEW_SORTED_CTX, Stage)

pytestmark = pytest.mark.gpu

MAX_N = 120_001
BITS = sm.HIST_BITS


@pytest.fixture(scope="module")
def st():
    import kiss_amd
    ctx = kiss_amd.Context(max_n=MAX_N, device=0)
    yield Stage(ctx)
    ctx.close()


def k_id(k):
    return "exact" if k == sc.K_EXACT else "k%d" % k


def classify_whole(st, S, k):
    """stage_classify(0, n), held against the model -> (far keys, far positions, near-end positions, counts12)"""
    rc, got = st.classify(S, k, 0, S.size)
    want = sm.counts13(S, k, 0, S.size)
    assert rc == 0 and got == want
    keys, pos, m_far = sm.local_list(S, k, 0, S.size)
    assert st.sizes() == (pos.size, m_far)
    return keys[:m_far], pos[:m_far], pos[m_far:], want[:12]


def sort_in_place(st, S, k, count):
    """(a): the ctx's own views in and out, as multi_gpu.GpuBackend passes them"""
    keys, pos = st.view_tensor(VIEW_LOCAL_KEYS, count), st.view_tensor(VIEW_LOCAL_POS, count)
    out, words = st.view_tensor(VIEW_SORTED, count), st.view_tensor(VIEW_SORTED_CTX, count)
    rc = st.sort(keys, pos, count, S.size, k, out, words)
    return rc, st.view(VIEW_SORTED, count), st.view(VIEW_SORTED_CTX, count)


def sort_copied(st, S, k, keys, pos):
    """(b): the caller's tensors; the inputs stay as they are, nothing is written behind `count` entries of the outputs"""
    count = pos.size
    d_keys_all, d_keys = st.to_dev(keys, room=8)
    d_pos_all, d_pos = st.to_dev(pos, room=8)
    out, words = st.guarded(count, 4), st.guarded(count, 4)
    rc = st.sort(d_keys, d_pos, count, S.size, k, out, words)
    assert np.array_equal(st.host(d_keys_all, count, np.uint64, "input keys"), keys), "input keys changed"
    assert np.array_equal(st.host(d_pos_all, count, np.uint32, "input positions"), pos), "input positions changed"
    return rc, st.host(out, count, np.uint32, "sorted positions"), st.host(words, count, np.uint32, "context words")


DEEP = 32_768  # KISS_EXACT_MSD_MAX_DEPTH: exact order gives up on list members that tie through this many bases (32 a round)


def check_sorted(S, k, listed, rc, got, words, what, want=None):
    """order, context words and taint bits of one stage_sort result -> number of tied members; None: the list has ties too
    deep for exact order (the model's longest common prefix of two members says so) and KISS_HIP_E_DEEP came back, as it must"""
    if sm.depth_of(S.size, k) == 0:
        deepest = sm.max_common_prefix(S, listed)
        assert not DEEP - 64 <= deepest < DEEP + 64, what + ": a case on the edge of the give-up depth decides nothing"
        if deepest >= DEEP:
            assert rc == E_DEEP, "%s: rc %d for members equal on %d bases" % (what, rc, deepest)
            return None
    assert rc != E_DEEP, what + ": KISS_HIP_E_DEEP on a list without ties 32768 bases deep"
    assert rc == 0, (what, rc)
    want = sm.sort_list(S, k, listed) if want is None else want
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d places differ, the first is %d: %d, model %d" % (
        what, bad.size, want.size, bad[0] if bad.size else -1, got[bad[0]] if bad.size else 0, want[bad[0]] if bad.size else 0)
    wrong = [(int(p), hex(int(w))) for p, w in zip(got, words) if not sm.valid_ctx_word(S, p, w)]
    assert not wrong, "%s: %d context words are neither 0 nor the word of their position, e.g. %s" % (what, len(wrong), wrong[:3])
    if sm.depth_of(S.size, k) == 0:
        return 0
    tied = sm.tied(S, k, listed)
    clean = [int(p) for p, w in zip(got, words) if int(p) in tied and not (int(w) & sm.TAINT)]
    assert not clean, "%s: %d of %d tied suffixes came back without the taint bit, e.g. %s" % (what, len(clean), len(tied), clean[:5])
    return len(tied)


def check_induce(st, oracle, S, k, got, words, near, counts12, what):
    """the sorted far list with the sort's words, without words and with nothing but taint bits: the oracle's SA each time"""
    want = oracle.suffix_sort(S, k)
    if k == sc.K_EXACT:
        assert np.array_equal(want, sm.suffix_array(S)), what + ": the oracle's exact SA is not the plain sort of the suffixes"
    _, d_far = st.to_dev(got)
    _, d_near = st.to_dev(near)
    forms = {"the sort's words": st.to_dev(words)[1], "no words": None,
             "taint bits only": st.to_dev(np.full(got.size, sm.TAINT, dtype=np.uint32))[1]}
    for form, d_words in forms.items():
        rc, sa = st.induce(S.size, k, d_far, d_words, d_near, counts12)
        assert rc == 0, (what, form, rc)
        bad = np.flatnonzero(sa != want)
        assert bad.size == 0, "%s, %s: %d SA entries differ, the first at %d" % (what, form, bad.size, bad[0] if bad.size else -1)


def groups_of(keys, splitters):
    top = (keys >> np.uint64(64 - BITS)).astype(np.int64)
    return (top[:, None] >= np.asarray(splitters, dtype=np.int64)[None, :]).sum(1) if len(splitters) else np.zeros(keys.size, np.int64)


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
@pytest.mark.parametrize("name", sc.SORT_TEXTS)
def test_whole_list_in_place_and_copied(st, oracle, name, k):
    S = sc.text(name)
    keys, pos, near, counts12 = classify_whole(st, S, k)
    want = sm.sort_list(S, k, pos)
    assert pos.size > (sc.RADIX_TILE if name == "genome120k" else 1000)          # (genome120k: the emit pass's counts are used)
    rc, got_a, words_a = sort_in_place(st, S, k, pos.size)                       # (a) right behind the classification
    n_tied = check_sorted(S, k, pos, rc, got_a, words_a, "%s k=%d in place" % (name, k), want)
    if name == "tandem" and k != sc.K_EXACT:
        assert n_tied > 100, "the tandem text has no ties through D"
    # the generated "genome" of 70 001 bases is covered by its 24 telomere arrays (3000 bases each, 2916 apart): one deep tie
    assert (n_tied is None) == (name == "genome" and k == sc.K_EXACT)
    classify_whole(st, S, k)                                                      # (digit counts of this list at hand: to be dropped)
    rc, got_b, words_b = sort_copied(st, S, k, keys, pos)                         # (b)
    assert (check_sorted(S, k, pos, rc, got_b, words_b, "%s k=%d copied" % (name, k), want) is None) == (n_tied is None)
    if n_tied is None:
        return
    assert np.array_equal(got_a, got_b)
    assert np.array_equal(words_a >> 31, words_b >> 31), "in place and copied: different taint bits"
    check_induce(st, oracle, S, k, got_a, words_a, near, counts12, "%s k=%d" % (name, k))


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
@pytest.mark.parametrize("name", sc.SORT_TEXTS)
def test_key_range_subsets(st, oracle, name, k):
    """(c): group g of 2, 3 and 7 key ranges; the pieces in group order are the order of the whole list"""
    from kiss_amd.multi_gpu import choose_splitters
    S = sc.text(name)
    keys, pos, near, counts12 = classify_whole(st, S, k)
    want = sm.sort_list(S, k, pos)
    hist = sm.key_hist(keys)
    sizes = set()
    tied_whole = sm.tied(S, k, pos) if k != sc.K_EXACT else set()
    tied_pieces = {}  # (number of groups, group) -> tied members of that piece
    for G in (2, 3, 7):
        sp = choose_splitters(hist, G)
        g = groups_of(keys, sp)
        pieces, words = [], []
        for q in range(G):
            sub = g == q
            sizes.add(int(sub.sum()))
            rc, got, cw = sort_copied(st, S, k, keys[sub], pos[sub])
            n_tied = check_sorted(S, k, pos[sub], rc, got, cw, "%s k=%d group %d of %d" % (name, k, q, G))
            deep = n_tied is None
            if k != sc.K_EXACT:  # equal on D bases = in one key range: a piece holds its tie groups whole
                assert n_tied == len(tied_whole & set(pos[sub].tolist())), "%s k=%d group %d of %d: tied members" % (name, k, q, G)
                tied_pieces[(G, q)] = n_tied
            pieces.append(got[:0] if deep else got)
            words.append(cw)
        if any(p.size == 0 and (g == q).sum() > 0 for q, p in enumerate(pieces)):
            assert name == "genome" and k == sc.K_EXACT  # (a key range with the telomere arrays: refused, nothing to put together)
            continue
        assert np.array_equal(np.concatenate(pieces), want), "%s k=%d: %d pieces in group order" % (name, k, G)
        if name == "tandem" and k != sc.K_EXACT:  # the pieces that hold the arrays have tied members, and there are such pieces
            assert sum(v for (G_, q), v in tied_pieces.items() if G_ == G) == len(tied_whole) > 100
            assert any(v > 0 for (G_, q), v in tied_pieces.items() if G_ == G)
    if name == "genome120k":
        assert max(sizes) > sc.RADIX_TILE  # (a key range of more than one radix tile, sorted on counts of its own)
    if name == "CA":
        assert 0 in sizes  # one 14-bit bin holds nearly everything: key ranges stay empty
    if name == "tandem":
        check_induce(st, oracle, S, k, np.concatenate(pieces), np.concatenate(words), near, counts12, "%s k=%d, 7 pieces" % (name, k))


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
def test_key_range_of_a_single_item_and_empty_lists(st, k):
    """(c) with splitters around a bin that holds one item, (e) count 0 and count 1"""
    S = sc.text("iid")
    keys, pos, near, counts12 = classify_whole(st, S, k)
    hist = sm.key_hist(keys)
    ones = np.flatnonzero(hist == 1)
    b = int(ones[ones.size // 2])
    g = groups_of(keys, [b, b + 1, b + 1])
    assert int((g == 1).sum()) == 1 and int((g == 2).sum()) == 0 and (g == 0).any() and (g == 3).any()
    pieces = []
    for q in range(4):
        rc, got, cw = sort_copied(st, S, k, keys[g == q], pos[g == q])
        check_sorted(S, k, pos[g == q], rc, got, cw, "iid k=%d group %d around a bin of one" % (k, q))
        pieces.append(got)
    assert pieces[1].tolist() == pos[g == 1].tolist() and pieces[2].size == 0
    assert np.array_equal(np.concatenate(pieces), sm.sort_list(S, k, pos))
    for q in (0, pos.size // 2, pos.size - 1):  # one item from the front, the middle and the end of the list
        rc, got, cw = sort_copied(st, S, k, keys[q:q + 1], pos[q:q + 1])
        assert rc == 0 and got.tolist() == [pos[q]] and sm.valid_ctx_word(S, pos[q], cw[0])
    assert st.sort(None, None, 0, S.size, k, None, None) == 0
    # in place with one item: what the views hold at their front
    classify_whole(st, S, k)
    rc, got, cw = sort_in_place(st, S, k, 1)
    assert rc == 0 and got.tolist() == [pos[0]] and sm.valid_ctx_word(S, pos[0], cw[0])


@pytest.mark.parametrize("k", sc.KS, ids=k_id)
@pytest.mark.parametrize("name", ["runs_G", "tandem", "genome", "genome120k"])
def test_list_put_together_from_a_window_tiling(st, name, k):
    """(d): what a receiver holds -- the far lists of five windows, as stage_classify emitted them, filtered by one of three key
    ranges and concatenated in window order"""
    from kiss_amd.multi_gpu import choose_splitters
    S = sc.text(name)
    n = S.size
    wkeys, wpos, _, _ = classify_whole(st, S, k)
    sp = choose_splitters(sm.key_hist(wkeys), 3)
    g3 = groups_of(wkeys, sp)
    mine_is = int(np.argmax(np.bincount(g3, minlength=3)))  # the fullest of three key ranges (on the "genome" texts the one with
    if name == "tandem" and k != sc.K_EXACT:                # the end arrays); on the tandem text the one with the most ties
        mine_is = int(np.argmax([len(sm.tied(S, k, wpos[g3 == q])) for q in range(3)]))
    got_keys, got_pos = [], []
    for lo, hi in sc.tilings(n)["tiling5"]:
        rc, _ = st.classify(S, k, lo, hi)
        assert rc == 0
        m, m_far = st.sizes()
        ck, cp = st.copy_list()
        mine = groups_of(ck[:m_far], sp) == mine_is
        got_keys.append(ck[:m_far][mine])
        got_pos.append(cp[:m_far][mine])
    keys, pos = np.concatenate(got_keys), np.concatenate(got_pos)
    sel = groups_of(wkeys, sp) == mine_is
    assert np.array_equal(pos, wpos[sel]) and np.array_equal(keys, wkeys[sel]) and 0 < pos.size < wpos.size
    assert np.all(np.diff(pos.astype(np.int64)) > 0)  # the received list ascends by position
    classify_whole(st, S, k)  # the state of the rank that sorts: the whole text classified, stale digit counts of ITS list
    rc, got, cw = sort_copied(st, S, k, keys, pos)
    n_tied = check_sorted(S, k, pos, rc, got, cw, "%s k=%d, key range %d of 3 from five windows" % (name, k, mine_is))
    if n_tied is None:
        assert name == "genome" and k == sc.K_EXACT
        return
    if name == "tandem" and k != sc.K_EXACT:
        assert n_tied > 0, "the list from the tiling holds no tied members"
    if name == "genome120k":  # more than one radix tile: sorted in place below while the ctx holds counts of ANOTHER list
        assert sc.RADIX_TILE < pos.size < wpos.size
    # ... and delivered into the ctx's own buffers, as the all-to-all does: sorted in place, but not the list that was counted
    st.view_tensor(VIEW_LOCAL_KEYS, pos.size).copy_(st.to_dev(keys)[1])
    st.view_tensor(VIEW_LOCAL_POS, pos.size).copy_(st.to_dev(pos)[1])
    rc, got2, cw2 = sort_in_place(st, S, k, pos.size)
    check_sorted(S, k, pos, rc, got2, cw2, "%s k=%d, the same in the ctx's buffers" % (name, k))
    assert np.array_equal(got, got2)


TINY_KS = {"k32": lambda n: 32, "n-1": lambda n: n - 1, "n": lambda n: n, "exact": lambda n: sc.K_EXACT}


@pytest.mark.parametrize("kname", list(TINY_KS))
@pytest.mark.parametrize("name", sc.TINY_TEXTS)
def test_tiny_texts_in_place_and_copied(st, oracle, name, kname):
    """n = 1, 2, 33 and the text without an LMS position: an empty far list beside near-end positions, no list at all, a text
    shorter than a packed word -- sorted in place and copied, then induced three ways"""
    S = sc.text(name)
    k = TINY_KS[kname](S.size)
    keys, pos, near, counts12 = classify_whole(st, S, k)
    assert pos.size + near.size == sm.lms(S).size and (name != "no_lms" and name != "n1" or pos.size + near.size == 0)
    if name == "n33":
        assert (pos.size, near.size > 0) == {"k32": (0, True), "n-1": (0, True)}.get(kname, (sm.lms(S).size, False))
    rc, got_a, words_a = sort_in_place(st, S, k, pos.size)
    check_sorted(S, k, pos, rc, got_a, words_a, "%s k=%d in place" % (name, k))
    classify_whole(st, S, k)
    rc, got_b, words_b = sort_copied(st, S, k, keys, pos)
    check_sorted(S, k, pos, rc, got_b, words_b, "%s k=%d copied" % (name, k))
    assert np.array_equal(got_a, got_b) and np.array_equal(words_a >> 31, words_b >> 31)
    check_induce(st, oracle, S, k, got_a, words_a, near, counts12, "%s k=%d" % (name, k))


def test_deep_ties_are_reported_and_the_ctx_works_on(st, oracle):
    """one (TTAGGG) array of 65 541 bases in exact order: ties deeper than KISS_EXACT_MSD_MAX_DEPTH = 32 768 bases"""
    S = sc.text("deep")
    keys, pos, near, counts12 = classify_whole(st, S, sc.K_EXACT)
    assert pos.size > 10_000 and near.size == 0
    p, q = int(pos[0]), int(pos[1])
    assert q - p == 6 and np.array_equal(S[p:p + 40_000], S[q:q + 40_000])  # (two list members equal on 40 000 bases)
    rc, _, _ = sort_in_place(st, S, sc.K_EXACT, pos.size)
    assert rc == E_DEEP, rc
    T = sc.text("tandem")
    for k in (256, sc.K_EXACT):
        keys, pos, near, counts12 = classify_whole(st, T, k)
        rc, got, cw = sort_in_place(st, T, k, pos.size)
        check_sorted(T, k, pos, rc, got, cw, "tandem k=%d behind the refused sort" % k)
        check_induce(st, oracle, T, k, got, cw, near, counts12, "tandem k=%d behind the refused sort" % k)


def test_argument_checks(st):
    S = sc.text("iid")
    keys, pos, near, counts12 = classify_whole(st, S, 256)
    n = S.size
    _, d_keys = st.to_dev(keys)
    _, d_pos = st.to_dev(pos)
    out, words = st.guarded(pos.size, 4), st.guarded(pos.size, 4)
    assert st.sort(d_keys, d_pos, pos.size, n + 1, 256, out, words) == E_INVALID  # not the text stage_classify packed
    assert st.sort(d_keys, d_pos, pos.size, 0, 256, out, words) == E_INVALID
    assert st.sort(None, d_pos, pos.size, n, 256, out, words) == E_INVALID
    assert st.sort(d_keys, None, pos.size, n, 256, out, words) == E_INVALID
    assert st.sort(d_keys, d_pos, pos.size, n, 256, None, words) == E_INVALID
    assert st.host(out, 0, np.uint32).size == 0 and st.host(words, 0, np.uint32).size == 0  # (nothing written by the refused calls)
    assert st.sort(d_keys, d_pos, pos.size, n, 256, out, None) == 0  # the context words are optional
    assert np.array_equal(st.host(out, pos.size, np.uint32), sm.sort_list(S, 256, pos))
