"""The pooled scratch of the rescue plan and the merge call (kiss_amd/csrc/kiss_internal.hpp: FM_SLOT_RESCUE_CTL,
FM_SLOT_RESCUE_SLAB) beside the other FM-index calls on ONE context: map_pairs(rescue=True) after and before each of
query_batch, seeds, align, map and map_pairs without rescue, held against a fresh context and against the _host entries,
which run on a context of their own -- as tests/test_fm_pair_pool_gpu.py does for the pair call."""
import numpy as np
import pytest

from tests.test_fm_pool_slots_gpu import L, Q, _inputs, _run, _same

pytestmark = pytest.mark.gpu

OTHERS = ("query_batch", "seeds", "align", "map", "map_pairs")


def _mates(pats):
    """the reads of the pool test as mates: read p and the reverse complement of read p + Q / 2 (far apart: nearly no pair is
    proper at ins_max 400, so nearly every pair is planned)"""
    half = Q // 2
    return list(pats[:half]), [(3 - r[::-1]).astype(np.uint8) for r in pats[half:]]


def _rescued(f, text, pats):
    m1, m2 = _mates(pats)
    return f.map_pairs(m1, m2, text, ins_max=400, rescue=True)


def _other(f, name, text, pats):
    if name == "map_pairs":
        m1, m2 = _mates(pats)
        return f.map_pairs(m1, m2, text, ins_max=4096)
    return _run(f, name, text, pats)


@pytest.fixture(scope="module")
def passes():
    import kiss_amd.fm_index as fm
    text, pats, _ = _inputs()
    f = fm.FMIndex(sa_intv=4).build(text, exact=True)
    fresh = _rescued(f, text, pats)
    f.close()
    f = fm.FMIndex(sa_intv=4).build(text, exact=True)
    others, between = {}, {}
    for name in OTHERS:  # other, rescue, other: the rescue calls after and before each
        others[name] = [_other(f, name, text, pats)]
        between[name] = _rescued(f, text, pats)
        others[name].append(_other(f, name, text, pats))
    f.close()
    return {"text": text, "pats": pats, "fresh": fresh, "others": others, "between": between}


def _flat(res):
    """a result with the two nested dicts laid out, for _same"""
    out = {k: v for k, v in res.items() if k not in ("first_pass", "rescue")}
    for name in ("first_pass", "rescue"):
        for k, v in res[name].items():
            out[name + "." + k] = v
    return out


def test_the_pairs_reach_the_rescue_calls(passes):
    r = passes["fresh"]
    rep = r["rescue"]["report"]
    assert rep["P"] == Q // 2 and rep["pairs_planned"] >= Q // 4 and rep["chains"] == r["rescue"]["chains"].size >= rep["pairs_planned"]
    assert r["rescue"]["merge_report"]["alignments_b"] == rep["chains"] and r["rescue"]["align_report"]["cells"] > 0
    assert r["alignments"].size == r["first_pass"]["alignments"] + rep["chains"] == r["aln_source"].size


def test_rescue_after_and_before_every_other_call_equals_a_fresh_context(passes):
    for name in OTHERS:
        _same(_flat(passes["fresh"]), _flat(passes["between"][name]), name)
        _same(passes["others"][name][0], passes["others"][name][1], name + " around map_pairs(rescue=True)")


def test_the_result_equals_the_host_entries_on_a_context_of_their_own(passes):
    import kiss_amd
    want = passes["fresh"]
    CA = want["first_pass"]["alignments"]
    a = want["aln_source"] < CA
    alns_a, alns_b = want["alignments"][a], want["alignments"][~a]  # (a read's own come first and in order, so do the rescued)
    assert np.array_equal(want["aln_source"][a], np.arange(CA)) and np.array_equal(want["aln_source"][~a], CA + np.arange(alns_b.size))
    first_hits = kiss_amd.select_alignments(alns_a, _first_index(want), np.full(Q, L), both_strands=True)
    assert np.array_equal(first_hits["hit_index"], want["first_pass"]["hit_index"])
    plan = kiss_amd.plan_rescue(want["first_pass"]["pairs"], first_hits["hits"], first_hits["hit_index"], alns_a, np.full(Q, L),
                                passes["text"].size, ins_max=400)
    _same({k: want["rescue"][k] for k in ("chains", "chain_index", "origin", "report")}, plan, "rescue_host")
    mg = kiss_amd.merge_alignments(alns_a, _first_index(want), alns_b, plan["chain_index"])
    assert mg["alignments"].tobytes() == want["alignments"].tobytes() and np.array_equal(mg["chain_index"], want["chain_index"])
    assert np.array_equal(mg["source"], want["aln_source"])
    for k in ("V", "alignments_a", "alignments_b", "alignments"):  # (no ops asked for here: cigar_ops is 0)
        assert mg["report"][k] == want["rescue"]["merge_report"][k], k


def _first_index(res):
    """the chain index of the first pass: what is left of the merged one without the rescue chains"""
    return res["chain_index"] - res["rescue"]["chain_index"]
