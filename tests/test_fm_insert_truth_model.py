"""The truth conditions that tests/test_fm_insert_gpu.py asserts for insert_truth_case(), confirmed without a GPU on the same
seed: the seed, chain, align, select, insert and pair models composed (tests/fm_seed_model.py, fm_chain_model.py,
fm_align_model.py, fm_select_model.py, fm_insert_model.py, fm_pair_model.py), default parameters, both strands.  If this fails
after a change of TRUTH_SEED or of insert_truth_case(), choose another seed; the assertions of the GPU test stay."""
import functools

import numpy as np

from tests import fm_align_model as am, fm_chain_model as cm, fm_insert_model as im, fm_pair_model as pm, fm_seed_model as sd
from tests import fm_select_model as sm
from tests.test_fm_insert_gpu import assert_insert_truth, insert_truth_case


@functools.lru_cache(maxsize=None)
def first_pass(damaged):
    S, m1, m2, truth = insert_truth_case(200, damaged)
    reads = [r for pr in zip(m1, m2) for r in pr]
    seeds = sd.Batch(S, reads, True, 0).seeds(19, 500)
    ch = cm.chain(seeds["start"], seeds["len"], seeds["seed_index"], seeds["positions"], seeds["pos_index"])
    al = am.align(S, reads, ch["chains"][:, 2:6], ch["chain_index"], True)
    sel = sm.select(al["alignments"], ch["chain_index"], [100] * len(reads), both_strands=True)
    return sel, al, truth


def test_the_truth_conditions_hold_in_the_composed_models():
    sel, al, truth = first_pass(0)
    est = im.estimate(sel["hits"], sel["hit_index"], al["alignments"])
    assert est["report"]["flags"] == im.OK and est["report"]["samples"] == 200
    plain = pm.pair(sel["hits"], sel["hit_index"], al["alignments"])
    used = {k: est["report"][k] for k in ("ins_min", "ins_max", "ins_mean")}
    auto = pm.pair(sel["hits"], sel["hit_index"], al["alignments"], **used)
    assert plain["report"]["proper"] == 0 and auto["report"]["proper"] == 200
    assert_insert_truth(plain["pairs"], auto["pairs"], est, truth)
    # the first 24 pairs alone: every one a sample, and too few of them
    hidx = np.asarray(sel["hit_index"])[:49]
    few = im.estimate(sel["hits"], hidx, al["alignments"])
    assert few["report"]["samples"] == 24 and few["report"]["flags"] == 0
    assert pm.pair(sel["hits"], hidx, al["alignments"])["report"]["proper"] == 0


def test_the_damaged_pairs_are_left_to_the_rescue_and_do_not_move_the_estimate():
    sel, al, truth = first_pass(10)
    est = im.estimate(sel["hits"], sel["hit_index"], al["alignments"])
    assert est["report"]["samples"] == 200 and est["report"]["unmapped"] == 10 and est["report"]["flags"] == im.OK
    used = {k: est["report"][k] for k in ("ins_min", "ins_max", "ins_mean")}
    assert pm.pair(sel["hits"], sel["hit_index"], al["alignments"], **used)["report"]["proper"] == 200
    # a window laid with the estimated bounds holds the mate; the default ins_max of 1000 ends short of every fragment
    assert used["ins_min"] <= 1400 and used["ins_max"] >= 1600
