"""The premises of tests/test_induce_count_gpu.py on the CPU (tests/induce_count_model.py): the texts have the tiles the
cases are about, the planted zeros lie where the cases say, and the walk that finds the words running out beside SA gives
the model's suffix array."""
import numpy as np
import pytest

from tests import induce_count_model as cm
from tests import induce_model as im
from tests.induce_cases import ROOMY_N, case_of, thresholds

PLANTED_TEXTS = [("genome60k", 256), ("genome60k", 32), ("near300", 256), ("near300", 32)]
CUT_TEXTS = [("genome60k", 256), ("iid40k", 32)]


@pytest.mark.parametrize("name,k", PLANTED_TEXTS, ids=["%s-k%d" % t for t in PLANTED_TEXTS])
def test_planted_zeros_lie_where_the_cases_say(oracle, name, k):
    case = case_of(oracle, name, k)
    far_in_order, far_index, passes = cm.lms_layout(case)
    assert np.array_equal(case.order[far_in_order], case.far)
    a, N = passes[0]
    assert a == 0 and N > 3 * cm.TILE
    t, shift = cm.block_tile(case)
    assert t >= 1
    if name.startswith("near"):
        assert case.near.size > 0
        # tiles with a near-end suffix inside exist too (counted item by item), and the block tile lies behind some of them
        assert shift > 0, "%s k=%d: no near-end suffix in front of tile %d of LMS(A)" % (name, k, t)
    full = im.ctx_words(case.S, case.far)
    tiles_in_all = sum((n + cm.TILE - 1) // cm.TILE for a_, n in passes)
    for placement, offsets in cm.PLACEMENTS.items():
        cw, zeros = cm.planted(case, placement)
        changed = np.nonzero(cw != full)[0]
        assert changed.size == zeros and not cw[changed].any(), placement
        if offsets is not None:
            merged = np.nonzero(far_in_order)[0][changed]
            assert (merged - t * cm.TILE).tolist() == sorted(offsets), placement
            lanes = {(int(o) % 256) // 4 for o in offsets}
            assert len(lanes) == 1 or placement in ("first_of_tile", "last_of_tile")
        elif placement == "one_per_tile":
            assert tiles_in_all - 4 <= zeros <= tiles_in_all  # (a tail of near-end suffixes only has no far word to zero)
        else:
            assert zeros == case.far.size


def test_lane_of_a_placement():
    """the placements name lanes of count_word_tile: item 256 q + 4 lane + e"""
    assert cm.PLACEMENTS["item3_of_lane63"] == [255]
    assert {(o % 256) // 4 for o in cm.PLACEMENTS["two_in_one_lane"]} == {17} and len(cm.PLACEMENTS["two_in_one_lane"]) == 2
    assert {(o % 256) // 4 for o in cm.PLACEMENTS["whole_lane"]} == {40} and len(set(cm.PLACEMENTS["whole_lane"])) == 32


@pytest.mark.parametrize("config", ["tiles", "tiles_words"])
@pytest.mark.parametrize("name,k", CUT_TEXTS, ids=["%s-k%d" % t for t in CUT_TEXTS])
def test_cut_words_run_out_in_full_tiles_of_both_sweeps(oracle, name, k, config):
    case = case_of(oracle, name, k)
    bases = np.random.default_rng(7).integers(0, 16, len(case.far))
    small_max, collapse_n, cap = thresholds(config)
    passes = cm.run_outs(case, bases, small_max, collapse_n, ROOMY_N)  # (asserts that the walk gives the model's SA)
    for sweep in "LS":
        found = cm.tile_passes_with_run_out(passes, sweep)
        print(sweep, found)
        assert found, (name, k, sweep)
    # with full words nothing runs out in a pass beside SA before 15 bases are used up, and the LMS passes meet no empty word
    passes = cm.run_outs(case, np.full(len(case.far), 15), small_max, collapse_n, ROOMY_N)
    assert not any(p.empties for p in passes if p.name.startswith("LMS"))

