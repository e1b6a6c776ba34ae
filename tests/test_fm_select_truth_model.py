"""The truth conditions that tests/test_fm_select_gpu.py asserts for EVERY read of its two cases, confirmed without a GPU on the
same seed: the seed, chain, align and select models composed (tests/fm_seed_model.py, fm_chain_model.py, fm_align_model.py,
fm_select_model.py), default parameters, both strands.  If this fails after a change of TRUTH_SEED or of truth_case(), choose
another seed or text; the assertions of the GPU test stay."""
import pytest

from tests import fm_align_model as am, fm_chain_model as cm, fm_seed_model as sd, fm_select_model as sm
from tests.test_fm_select_gpu import truth_case


@pytest.mark.parametrize("kind", ("unique", "repeat"))
def test_the_truth_conditions_hold_in_the_composed_models(kind):
    S, reads, starts = truth_case(kind)
    seeds = sd.Batch(S, reads, True, 0).seeds(19, 500)
    ch = cm.chain(seeds["start"], seeds["len"], seeds["seed_index"], seeds["positions"], seeds["pos_index"])
    al = am.align(S, reads, ch["chains"][:, 2:6], ch["chain_index"], True)
    res = sm.select(al["alignments"], ch["chain_index"], [150] * len(reads), both_strands=True)
    for q, p in enumerate(starts):
        mine = res["hits"][res["hit_index"][q]:res["hit_index"][q + 1]]
        assert len(mine) >= 1, (kind, q)
        aln, flags, mapq, _, _, n_sec = (int(x) for x in mine[0][:6])
        tbeg = int(al["alignments"][aln][4])
        assert flags & ~sm.HIT_REVERSE == 0 and bool(flags & sm.HIT_REVERSE) == bool(q % 2), (kind, q)
        if kind == "unique":
            assert abs(tbeg - p) <= 32 and mapq == 60 and n_sec == 0, (kind, q, tbeg, p)
        else:
            assert min(abs(tbeg - p), abs(tbeg - p - 10000)) <= 32 and mapq == 0 and n_sec >= 1, (kind, q, tbeg, p)
