"""The count pass of the induction (k_induce_count, kiss_amd/csrc/induce.hip) where its forms meet: items whose context word
has no bases inside tiles that are otherwise counted in straight-line code (the refresh loop of the word form and of the
class-byte form), and full tiles, a one-item tail and misaligned byte stretches side by side.

Route and yardstick are those of tests/test_induce_paths_gpu.py: the stage calls, the SA compared bit for bit with the
sequential model (tests/induce_model.py) and the oracle, and the launch counts of the kernel classes proving that the tile
kernels ran.  A count that is off by one item shifts everything the scatter pass writes behind it, so the SA shows it.
The premises of every case are asserted from the model (tests/induce_count_model.py; tests/test_induce_count_model.py holds
them without a GPU)."""
import numpy as np
import pytest

from tests import induce_count_model as cm
from tests import induce_model as im
from tests.induce_cases import ROOMY_N, case_of, plan, thresholds
from tests.test_induce_paths_gpu import check, prove, run_induce, set_config

pytestmark = pytest.mark.gpu

CONFIGS = ("tiles", "tiles_words")  # class bytes beside SA, or context words everywhere; the far list is always words
PLANTED_TEXTS = [("genome60k", 256), ("genome60k", 32), ("near300", 256), ("near300", 32)]
CUT_TEXTS = [("genome60k", 256), ("iid40k", 32)]
CUT_SEED = 7  # (test_induce_paths_gpu.make_words: the seed of its "cut" words)


@pytest.fixture(scope="module")
def roomy():
    import kiss_amd
    c = kiss_amd.Context(max_n=ROOMY_N, device=0, hooks=True)
    c.set_profiling(True, classes=["induce_count", "induce_scatter", "induce_small"])
    yield c
    c.close()


def near_case(oracle, name, k):
    """near300 is written for k = 1000; at k = 256 and 32 fewer of its tail's suffixes are near-end ones, but some are"""
    case = case_of(oracle, name, k)
    if name.startswith("near"):
        assert case.near.size > 0, "%s k=%d: no near-end suffix" % (name, k)
    assert case.sch.lms_pass[0] > 3 * cm.TILE, "%s: LMS(A) has %d items" % (name, case.sch.lms_pass[0])
    return case


# ---- zeros planted in the far list: the refresh loop of the word form -----------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("placement", sorted(cm.PLACEMENTS))
@pytest.mark.parametrize("name,k", PLANTED_TEXTS, ids=["%s-k%d" % t for t in PLANTED_TEXTS])
def test_planted_empties_in_the_far_list(roomy, oracle, monkeypatch, name, k, placement, config):
    case = near_case(oracle, name, k)
    cw, zeros = cm.planted(case, placement)
    assert zeros > 0 and int((cw == 0).sum()) == zeros
    expected = plan(case, config, None, max_n=roomy.max_n)
    assert case.sch.lms_pass[0] > thresholds(config)[0], "LMS(A) is a tile pass"
    set_config(monkeypatch, config)
    what = "%s k=%d under %s, %d zero words (%s)" % (name, k, config, zeros, placement)
    sa, st = run_induce(roomy, case, case.far, cw)
    msg = im.compare(sa, case.want, case.sch, what)
    assert not isinstance(st, str), "%s; the sweeps stopped at their own bucket check; until then: %s" % (st, msg)
    assert msg is None, msg
    assert np.array_equal(sa, case.sa_oracle), what + ": equals the model but not the oracle"
    ic, isc, ism = prove(st, config, expected, what)
    assert ic >= 1, what


# ---- words that run out beside SA: the refresh loop of the class-byte form (tiles) and of the word form (tiles_words) -----
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name,k", CUT_TEXTS, ids=["%s-k%d" % t for t in CUT_TEXTS])
def test_words_that_run_out_beside_sa(roomy, oracle, monkeypatch, name, k, config):
    case = case_of(oracle, name, k)
    bases = np.random.default_rng(CUT_SEED).integers(0, 16, len(case.far))
    small_max, collapse_n, cap = thresholds(config)
    passes = cm.run_outs(case, bases, small_max, collapse_n, roomy.max_n)
    for sweep in "LS":
        found = cm.tile_passes_with_run_out(passes, sweep)
        assert found, "%s k=%d: no full tile of a pass beside SA in the %s sweep holds an item whose word has run out" % (name, k, sweep)
    ic, isc, ism = check(roomy, oracle, name, k, config, monkeypatch, words="cut")
    assert ic >= sum(1 for p in passes if p.kind == "tile" and not p.name.startswith("LMS"))


# ---- the tiles of one wave: full tiles, a one-item tail, misaligned byte stretches ----------------------------------------
# x = 2049, 4097, G 2048 + 1 and (G + 1) 2048 + 1 with G the tiles a wave takes: with the one tile per wave that was kept
# the last two are the first two.  A workgroup is four waves, so 4097 also has full tiles and the tail in one workgroup.
G = cm.KEPT_TILES_PER_WAVE
EDGES = sorted({2049, 4097, G * 2048 + 1, (G + 1) * 2048 + 1})


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("j", [0, 5, 15])
@pytest.mark.parametrize("x", EDGES)
def test_tile_grouping(roomy, oracle, monkeypatch, x, j, config):
    """(CA)^x T^130 behind j more A: LMS(A) and L-part(C) have x items -- full tiles and a tail of one item, under `tiles`
    read as class bytes from a bucket start that j moves off the 16-byte grid, in both sweeps"""
    name = "edge%d_A%d" % (x, j)
    case = case_of(oracle, name, 32, S=im.tile_edge(x, j, im.A_))
    assert case.sch.lms_pass[0] == x and case.near.size == 0 and case.sch.chains[("L", 1)] == [x]
    assert x % cm.TILE == 1 and x // cm.TILE in (1, 2, G, G + 1)
    for words in ("full", "cut"):
        ic, isc, ism = check(roomy, oracle, name, 32, config, monkeypatch, words=words)
        assert ic >= 3, name  # LMS(A), L-part(C) left to right, L-part(C) right to left
