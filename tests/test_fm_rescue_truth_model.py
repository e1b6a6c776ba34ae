"""The truth conditions that tests/test_fm_rescue_gpu.py asserts for EVERY pair of rescue_truth_case(), confirmed without a GPU
on the same seed: the seed, chain, align, select, pair and rescue models composed (tests/fm_rescue_model.py: pipeline()),
default parameters but for ins_max.  If this fails after a change of TRUTH_SEED or of rescue_truth_case(), choose another seed;
the assertions of the GPU test stay."""
from tests import fm_pair_model as pm, fm_rescue_model as rm
from tests.test_fm_rescue_gpu import TRUTH_PAIR, assert_rescue_truth, rescue_truth_case


def test_the_truth_conditions_hold_in_the_composed_models():
    S, m1, m2, truth = rescue_truth_case()
    reads = [r for pr in zip(m1, m2) for r in pr]
    out = rm.pipeline(S, reads, pair_params=TRUTH_PAIR)
    assert out["pair"]["report"]["proper"] == 0
    assert_rescue_truth(out["pair"]["pairs"], out["pair2"]["pairs"], out["select"]["hits"], out["select2"]["hits"], out["merge"]["alignments"],
                        out["merge"]["source"], out["align"]["alignments"].shape[0], truth)
    assert out["pair2"]["report"]["proper"] == 30 and out["rescued"] == 30 and out["plan"]["report"]["pairs_planned"] == 35
    assert not (out["pair2"]["pairs"][30:, 2] & pm.PROPER).any()
