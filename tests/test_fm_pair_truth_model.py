"""The truth conditions that tests/test_fm_pair_gpu.py asserts for EVERY pair of pair_truth_case(), confirmed without a GPU on
the same seed: the seed, chain, align, select and pair models composed (tests/fm_seed_model.py, fm_chain_model.py,
fm_align_model.py, fm_select_model.py, fm_pair_model.py), default parameters, both strands.  If this fails after a change of
TRUTH_SEED or of pair_truth_case(), choose another seed; the assertions of the GPU test stay."""
from tests import fm_align_model as am, fm_chain_model as cm, fm_pair_model as pm, fm_seed_model as sd, fm_select_model as sm
from tests.test_fm_pair_gpu import assert_truth, pair_truth_case


def test_the_truth_conditions_hold_in_the_composed_models():
    S, m1, m2, truth = pair_truth_case()
    reads = [r for pr in zip(m1, m2) for r in pr]
    seeds = sd.Batch(S, reads, True, 0).seeds(19, 500)
    ch = cm.chain(seeds["start"], seeds["len"], seeds["seed_index"], seeds["positions"], seeds["pos_index"])
    al = am.align(S, reads, ch["chains"][:, 2:6], ch["chain_index"], True)
    sel = sm.select(al["alignments"], ch["chain_index"], [150] * len(reads), both_strands=True)
    res = pm.pair(sel["hits"], sel["hit_index"], al["alignments"])
    hits = [tuple(int(v) for v in h) for h in sel["hits"]]
    for p in range(len(truth)):  # select alone: mate 1 has MAPQ 0 and a secondary, mate 2 MAPQ 60
        first1, first2 = hits[int(sel["hit_index"][2 * p])], hits[int(sel["hit_index"][2 * p + 1])]
        assert first1[2] == 0 and first1[5] >= 1 and first2[2] == 60, (p, first1, first2)
    assert_truth((res["pairs"], hits, sel["hit_index"]), truth, lambda h: int(al["alignments"][h[0]][4]))
    assert res["report"]["promoted"] == 10 and res["report"]["lifted"] == 20 and res["report"]["proper"] == 20
