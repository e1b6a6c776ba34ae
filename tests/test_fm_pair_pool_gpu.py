"""The pooled scratch of the pair call (kiss_amd/csrc/kiss_internal.hpp: FM_SLOT_PAIR_CTL) beside the other FM-index calls on
ONE context: map_pairs after and before each of query_batch, seeds, align and map.  A slot that two roles share by mistake, or
a buffer that one call leaves in a state the next one trips over, shows as a result that depends on what ran before; the
result is also held against a fresh context and against the _host entry, which runs on a context of its own.  The new slots'
part of what tests/test_fm_pool_slots_gpu.py checks for the others."""
import numpy as np
import pytest

from tests.test_fm_pool_slots_gpu import L, Q, _inputs, _run, _same

pytestmark = pytest.mark.gpu

OTHERS = ("query_batch", "seeds", "align", "map")


def _pairs(f, text, pats):
    """the reads of the pool test as mates: read p and the reverse complement of read p + Q / 2"""
    half = Q // 2
    m1 = list(pats[:half])
    m2 = [(3 - r[::-1]).astype(np.uint8) for r in pats[half:]]
    return f.map_pairs(m1, m2, text, ins_max=4096)


@pytest.fixture(scope="module")
def passes():
    import kiss_amd.fm_index as fm
    text, pats, _ = _inputs()
    f = fm.FMIndex(sa_intv=4).build(text, exact=True)
    fresh = _pairs(f, text, pats)
    f.close()
    f = fm.FMIndex(sa_intv=4).build(text, exact=True)
    others, between = {}, {}
    for name in OTHERS:  # other, pairs, other: the pair call after and before each
        others[name] = [_run(f, name, text, pats)]
        between[name] = _pairs(f, text, pats)
        others[name].append(_run(f, name, text, pats))
    f.close()
    return {"text": text, "pats": pats, "fresh": fresh, "others": others, "between": between}


def test_the_pairs_reach_the_pair_call(passes):
    rep = passes["fresh"]["pair_report"]
    assert rep["P"] == Q // 2 and rep["eligible"] > Q // 2 and rep["proper"] >= 4 and rep["combinations"] > rep["proper"]
    assert passes["fresh"]["pairs"].shape == (Q // 2,) and passes["fresh"]["hit_index"].size == Q + 1


def test_map_pairs_after_and_before_every_other_call_equals_a_fresh_context(passes):
    for name in OTHERS:
        _same(passes["fresh"], passes["between"][name], name)
        _same(passes["others"][name][0], passes["others"][name][1], name + " around map_pairs")


def test_the_result_equals_the_host_entry_on_a_context_of_its_own(passes):
    import kiss_amd
    want = passes["fresh"]
    got = kiss_amd.pair_hits(want["hits"], want["hit_index"], want["alignments"], ins_max=4096)
    _same({"pairs": want["pairs"], "report": want["pair_report"]}, got, "pair_host")
    sel = kiss_amd.select_alignments(want["alignments"], want["chain_index"], np.full(Q, L), both_strands=True)
    _same({"hits": want["hits"], "hit_index": want["hit_index"], "report": want["select_report"]}, sel, "select_host")
