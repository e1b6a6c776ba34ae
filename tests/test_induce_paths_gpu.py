"""The induction sweeps (kiss_amd/csrc/induce.hip) path by path against the sequential model (tests/induce_model.py).

Route: the stage calls, so that only placement and induction run between the model's input and the result --
GpuBackend.classify packs the text (its counts, far count and near-end list are held against the model), then
GpuBackend.induce gets the oracle's k-ordered LMS list filtered to the far positions plus the model's near-end positions.
The SA that comes back is compared bit for bit with induce_model.induce (and the oracle's SA); a difference is reported
with the configuration, the number of differing slots, the first one and the segment and round that wrote it.

Every case sets switches of the hooks build that force one path at test size (CONFIGS), asserts through the model that
the text has what the case is about (tests/induce_cases.py: plan) and through the kernel-class launch counts that the path ran (prove).
"""
import contextlib

import numpy as np
import pytest

from tests import gen
from tests import induce_model as im
from tests.induce_cases import (CONFIGS, FORM_TEXTS, GRID, K_EXACT, MAIN, ROOMY_N, SWITCHES, TIGHT, case_of, forget, plan,
                                thresholds)

pytestmark = pytest.mark.gpu

# ---- the GPU side -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def roomy():
    import kiss_amd
    c = kiss_amd.Context(max_n=ROOMY_N, device=0, hooks=True)
    c.set_profiling(True, classes=["induce_count", "induce_scatter", "induce_small"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def tight():
    """contexts of exactly a text's size (one per size, made on demand): capacity m_cap / N limits the collapse step"""
    import kiss_amd
    made = {}

    def get(n):
        if n not in made:
            made[n] = kiss_amd.Context(max_n=n, device=0, hooks=True)
            made[n].set_profiling(True, classes=["induce_count", "induce_scatter", "induce_small"])
        return made[n]
    yield get
    for c in made.values():
        c.close()


@contextlib.contextmanager
def device_errors_end_the_run():
    """a HIP error (not a wrong answer) ends the whole run: nothing more is started on a device that has just faulted"""
    import kiss_amd
    try:
        yield
    except kiss_amd._lib.KissHipError as e:
        if e.status in (kiss_amd._lib.KISS_HIP_E_HIP, kiss_amd._lib.KISS_HIP_E_NOMEM):
            pytest.exit("device error, stopping: %s" % e, returncode=3)
        raise


def set_config(monkeypatch, config, **extra):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(CONFIGS[config], **extra).items():
        monkeypatch.setenv(name, str(value))


def _dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).to(torch.device("cuda", 0))


SLACK = 4096


def sa_buffer(n, torch):
    """-> (SA, the whole buffer): a zeroed SA with zeroed room behind it -- a slot the sweeps never write reads 0, and
    nothing may be written behind"""
    whole = torch.zeros(n + 1 + SLACK, dtype=torch.int32, device=torch.device("cuda", 0))
    return whole[:n + 1], whole


def sa_result(whole, n, what):
    whole = whole.cpu().numpy().view(np.uint32)
    assert not whole[n + 1:].any(), what + ": written behind the end of SA"
    return whole[:n + 1].copy()


def classify_checked(ctx, case):
    """packs the text (stage_classify) and holds what the library found against the model -> backend"""
    import torch
    from kiss_amd import multi_gpu
    be = multi_gpu.GpuBackend(ctx, torch.from_numpy(case.S).to(torch.device("cuda", 0)), case.k)
    counts13 = be.classify(0, case.n)
    assert counts13[:12] == case.counts12, "%s: counts %s, model %s" % (case.name, counts13[:12], case.counts12)
    keys, pos, m_far = be.local_lms()
    assert m_far == counts13[12] == case.far_asc.size, "%s: m_far %d / %d, model %d" % (case.name, m_far, counts13[12], case.far_asc.size)
    got = pos.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got[:m_far], case.far_asc), case.name + ": ascending far list"
    assert np.array_equal(got[m_far:], case.near), case.name + ": near-end list"
    return be


def run_induce(ctx, case, far, ctx_words=None):
    """stage_classify + stage_induce -> (SA, stats)"""
    import torch
    import kiss_amd
    with device_errors_end_the_run():
        be = classify_checked(ctx, case)
        cw = None if ctx_words is None else _dev(ctx_words, torch)
        SA, whole = sa_buffer(case.n, torch)
        try:
            be.induce(_dev(far, torch), _dev(case.near, torch), case.counts12, SA=SA, far_ctx=cw)
        except kiss_amd.KissHipError as e:
            if e.status != kiss_amd._lib.KISS_HIP_E_INTERNAL:
                raise
            # the sweeps check every bucket's fill themselves and stop: what they had written by then says where it went wrong
            return sa_result(whole, case.n, case.name), str(e)
        return sa_result(whole, case.n, case.name), ctx.stats()


def prove(st, config, r, what):
    """the launch counts of the kernel classes and the pass count say which path ran, and how often"""
    k = st["kernels"]
    ic, isc, ism = (int(k[x]["launches"]) for x in ("induce_count", "induce_scatter", "induce_small"))
    got = "%s: launches count %d scatter %d small %d, %d passes; model: %d tile passes, %d one-workgroup, %d closed-form calls %s" % (
        what, ic, isc, ism, st["induce_passes"], r.tile, r.small, r.calls, [s[3][:4] for s in r.steps])
    if "KISS_HIP_INDUCE_ONE_PASS" in CONFIGS[config]:
        assert ic == 0 and isc == r.tile, got
    else:
        assert ic == r.tile and isc == r.tile, got
    assert ism >= r.small + r.calls and (ism > 0) == (r.small + r.calls > 0), got
    # one pass per tile pass, per one-workgroup launch and per closed-form call: a chain that continues from its last block
    # after every `cap` steps shows here
    assert st["induce_passes"] == r.passes, got
    return ic, isc, ism


def check(ctx, oracle, name, k, config, monkeypatch, claim=None, far=None, want=None, sch=None, words="full", **extra):
    case = case_of(oracle, name, k)
    expected = plan(case, config, claim, max_n=ctx.max_n)
    set_config(monkeypatch, config, **extra)
    what = "%s k=%d under %s (%s words)" % (name, k, config, words)
    cw = make_words(case, case.far if far is None else far, words)
    sa, st = run_induce(ctx, case, case.far if far is None else far, cw)
    msg = im.compare(sa, case.want if want is None else want, case.sch if sch is None else sch, what)
    assert not isinstance(st, str), "%s; the sweeps stopped at their own bucket check; until then: %s" % (st, msg)
    assert msg is None, msg
    if want is None:
        assert np.array_equal(sa, case.sa_oracle), what + ": equals the model but not the oracle"
    return prove(st, config, expected, what)


def make_words(case, far, form, seed=7):
    """the four forms the context words of the far list may come in"""
    if form == "none":
        return None                                       # all gathered, all tainted
    if form == "zero":
        return np.zeros(len(far), dtype=np.uint32)        # 0 = gather
    if form == "full":
        return im.ctx_words(case.S, far)
    assert form == "cut"                                  # 0 .. 15 bases each: the children inherit the short words
    return im.ctx_words(case.S, far, np.random.default_rng(seed).integers(0, 16, len(far)))


@pytest.mark.parametrize("name,k,config,claim", GRID, ids=["%s-k%d-%s" % g[:3] for g in GRID])
def test_paths(roomy, oracle, monkeypatch, name, k, config, claim):
    ic, isc, ism = check(roomy, oracle, name, k, config, monkeypatch, claim)
    small_max = thresholds(config)[0]
    if name.startswith("edge"):  # x LMS suffixes of A and x items of L-part(C): at the threshold the one-workgroup kernel alone
        x = int(name[4:])
        others = 1 if 130 > small_max else 0  # (the L-part of T, 130 items, feeds nothing but is a pass)
        assert (ic - others > 0) == (x > small_max), "%s under %s: %d count launches" % (name, config, ic)
    if name.startswith("near") and config != "shipped":
        E = int(name[4:])
        assert case_of(oracle, name, k).near.size == E and roomy.stats()["near_end"] == E
        assert case_of(oracle, name, k).sch.lms_pass[0] > 3 * 2048, "LMS(A) has tiles with and without a near-end suffix"


# 5: giant runs -- rounds of three items, so the first closed-form call of either sweep runs into the 16-bit step field
# (65 535 steps, plan: "wide") and the runs of 65 536 and 70 000 continue with the wide field (the only text above 120 000 bases)
def test_giant_runs(roomy, oracle, monkeypatch):
    check(roomy, oracle, "giant", 256, "shipped", monkeypatch, claim="wide")


# a context of the text's own size: under the shipped thresholds m_cap / N limits the closed form's steps by itself and the
# chain continues (plan: "capacity"); under `tiles` the large rounds take the tile path with that context's small arrays
@pytest.mark.parametrize("name,config", TIGHT, ids=["%s-%s" % t for t in TIGHT])
def test_paths_tight_context(tight, oracle, monkeypatch, name, config):
    case = case_of(oracle, name, 256)
    ic, isc, ism = check(tight(case.n), oracle, name, 256, config, monkeypatch, claim="capacity" if config == "shipped" else None)
    if config == "tiles":
        assert ic > 0 and isc > 0, "%s under tiles on a tight context: no tile launch" % name


# 8: (CA)^2049 T^130 behind 0 .. 15 more bases.  Extra A move the start of bucket C through every residue mod 16, so the
# class-byte stretch of L-part(C) (one full tile and one item) is read at all 16 alignments in both sweeps; extra T leave
# the bucket starts of A and C where they are and move the text under the packed words instead.
@pytest.mark.parametrize("base", ["A", "T"])
@pytest.mark.parametrize("config", ["tiles", "tiles_words"])
def test_class_byte_alignments(roomy, oracle, monkeypatch, base, config):
    begins = set()
    for j in range(16):
        name = "edge2049_%s%d" % (base, j)
        case = case_of(oracle, name, 32)
        assert case.sch.lms_pass[0] == 2049 and case.near.size == 0 and case.sch.chains[("L", 1)] == [2049]
        begins.add(case.sch.begin[("L", 1)] % 16)
        ic, isc, ism = check(roomy, oracle, name, 32, config, monkeypatch)
        assert ic >= 3, name  # LMS(A), L-part(C) left to right, L-part(C) right to left
    assert base == "T" or begins == set(range(16))


# 10: tiny texts
@pytest.mark.parametrize("config", ["shipped", "tiles"])
def test_tiny_texts(roomy, oracle, monkeypatch, config):
    from tests.test_suffix_sort_gpu import _random_text
    rng = np.random.default_rng(4242)
    ks = [1, 32, 125, 256, K_EXACT]
    for t in range(200):
        n = int(rng.integers(1, 401))
        S = _random_text(rng, n)
        name = "tiny%d" % t
        case_of(oracle, name, ks[t % len(ks)], S=S)
        check(roomy, oracle, name, ks[t % len(ks)], config, monkeypatch, words=("full", "none", "cut")[t % 3])
        forget(name, ks[t % len(ks)])


# ---- forms of the input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["shipped", "tiles", "cap3"])
@pytest.mark.parametrize("idx", range(7))
def test_context_word_forms(roomy, oracle, monkeypatch, config, idx):
    """no words at all, all zero, full 15-base words, words cut to 0 .. 15 bases (refresh paths of count, scatter and the
    one-workgroup kernel all over both sweeps, a lone empty word in an otherwise full tile included): the same SA"""
    name, k = FORM_TEXTS[config][idx]
    for words in ("none", "zero", "full", "cut"):
        check(roomy, oracle, name, k, config, monkeypatch, words=words)


@pytest.mark.parametrize("config", ["shipped", "tiles", "cap3", "tiles_merged"])
@pytest.mark.parametrize("idx", range(5))
def test_order_is_preserved(roomy, oracle, monkeypatch, config, idx):
    """A segment is a stable partition of its items in source order: the sweeps may not depend on the LMS
    list being sorted.  No near-end suffix (the text ends in D + 5 T), so placement consumes no order either; the far list
    shuffled inside each first-base group must give exactly what the model induces from that order."""
    base, k = FORM_TEXTS.get(config, MAIN)[idx]
    name = base + "_tail"
    case = case_of(oracle, name, k, S=im.with_far_tail(im.texts()[base][0](), k))
    assert case.near.size == 0 and case.far.size == case.lms.size
    shuffled = im.shuffled_in_groups(case.S, case.order, 11 + idx)
    assert not np.array_equal(shuffled, case.order)
    sch = im.schedule(case.S, shuffled)
    want = im.induce(case.S, shuffled)
    assert np.array_equal(sch.SA, want) and not np.array_equal(want, case.want)
    check(roomy, oracle, name, k, config, monkeypatch, far=shuffled, want=want, sch=sch, words=("full", "cut")[idx % 2])


TAINT_TEXTS = {"periodic": lambda: gen.periodic(30_000, 171, 12, mutations=40), "planted": None}


@pytest.mark.parametrize("config", ["shipped", "tiles", "small_chain", "cap1", "cap3"])
@pytest.mark.parametrize("text", ["periodic", "planted"])
def test_taint_reaches_the_exact_finish(roomy, oracle, monkeypatch, text, config):
    """The taint bits are the sort's: far list and context words from the library's own stage_sort, then stage_induce and
    the suffix-array form of the exact finish, which looks for tie groups among tainted neighbours only.  A path that
    drops the bit puts a tie group's member down as a head and the exact SA comes out wrong."""
    import torch
    if text == "planted":
        name = "planted"  # (runs of 3073: about 3000 closed-form calls per chain under cap1, a second or two)
        case = case_of(oracle, name, 256)
    else:
        name = "periodic171"
        case = case_of(oracle, name, 256, S=TAINT_TEXTS[text]())
    exact = oracle.suffix_sort(case.S, K_EXACT)
    plan(case, config)
    set_config(monkeypatch, config, KISS_HIP_NO_LMS_EXACT=1)
    with device_errors_end_the_run():
        be = classify_checked(roomy, case)
        keys, pos, m_far = be.local_lms()
        srt, cw = be.sort(keys[:m_far], pos[:m_far])
    assert np.array_equal(srt.cpu().numpy().view(np.uint32), case.far), name + ": the library's sorted far list"
    tainted = int((cw.cpu().numpy().view(np.uint32) >> 31).sum())
    assert tainted > 0, name + ": no far suffix left the sort tainted"
    with device_errors_end_the_run():
        SA, whole = sa_buffer(case.n, torch)
        be.induce(srt, pos[m_far:].clone(), case.counts12, SA=SA, far_ctx=cw)
    what = "%s k=256 under %s (the sort's words)" % (name, config)
    msg = im.compare(sa_result(whole, case.n, what), case.want, case.sch, what)
    assert msg is None, msg
    with device_errors_end_the_run():
        be.refine_exact(SA, 256)
        torch.cuda.synchronize()
    msg = im.compare(sa_result(whole, case.n, what), exact, None, what + ", after the exact finish (taint bits)")
    assert msg is None, msg
