"""kiss_hip_fmi_rescue_dev / _host and kiss_hip_fmi_aln_merge_dev / _host against tests/fm_rescue_model.py: (a) the plan on
synthetic pair, hit and alignment arrays, every chain, chain_index, origin and report count; (b) the capacity protocol and
the error contract of the raw device calls; (c) the merge; (d) FMIndex.map_pairs(rescue=True) on the texts of the FM tests,
every stage compared with its model run on what the device gave the stage before; (e) against the truth: mates without a
seed found next to their partners."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_align_model as am, fm_pair_model as pm, fm_rescue_model as rm, fm_select_model as sm
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 300)
MAX_N = 4294963200
TOP = (1 << 32) - 4097


def check_plan(res, want):
    got = np.stack([res["chains"][k].astype(np.int64) for k in rm.CHAIN_FIELDS], axis=1).reshape(-1, 6)
    rep = res["report"]
    print({k: rep[k] for k in rm.REPORT_COUNTS})
    assert {k: rep[k] for k in rm.REPORT_COUNTS} == want["report"]
    assert np.array_equal(res["chain_index"].astype(np.int64), want["chain_index"])
    assert got.shape == want["chains"].shape, (got.shape, want["chains"].shape)
    for c in np.flatnonzero((got != want["chains"]).any(axis=1))[:3]:
        raise AssertionError("chain %d: %s, the model says %s" % (c, got[c], want["chains"][c]))
    assert np.array_equal(res["origin"].astype(np.int64), want["origin"])


def run_plan(pairs, hits, hidx, alns, lens, n, bounds=None, **params):
    """model and device on the same arrays -> what the model says"""
    import kiss_amd
    want = rm.plan(pairs, hits, hidx, alns, lens, n, bounds, **params)
    res = kiss_amd.plan_rescue(np.asarray(pairs, np.int64).reshape(-1, 10), np.asarray(hits, np.int64).reshape(-1, 8), hidx,
                               np.asarray(alns, np.int64).reshape(-1, 12), lens, n, bounds=bounds, **params)
    check_plan(res, want)
    return want


def flagged(npairs, flags=0):
    """pair records of which only flags matters"""
    out = np.zeros((npairs, 10), np.int64)
    out[:, 2] = flags
    return out


# ---- (a) the plan on synthetic arrays -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crossed_case():
    """the other mate with 0 .. 300 hits on either side, hits that are no anchors mixed in; some pairs proper or bad input"""
    rng = np.random.default_rng(51)
    counts = [(c1, c2) for c1 in COUNTS for c2 in (0, 2, 65, 300)]
    case = rm.random_case(rng, counts, 3000, nrefs=2, extra=3, ins_max=150)
    pairs = case["pairs"].copy()
    pairs[:, 2] &= ~pm.PROPER  # (with so many hits nearly every pair has a concordant combination: all but three are planned here)
    pairs[5, 2] |= pm.PROPER
    pairs[20, 2] |= pm.BAD_INPUT
    pairs[33, 2] = pm.PROPER | pm.BAD_INPUT
    return pairs, case["hits"], case["hit_index"], case["alns"], case["lens"]


@pytest.mark.parametrize("max_anchors", (1, 4, 64, 100))
def test_hit_counts_around_the_chunk_of_64_and_max_anchors(max_anchors):
    pairs, hits, hidx, alns, lens = crossed_case()
    want = run_plan(pairs, hits, hidx, alns, lens, 5000, bounds=[0, 2500, 5000], max_anchors=max_anchors, min_anchor_score=40,
                    ins_max=400, max_width=100)
    rep = want["report"]
    assert rep["anchors"] > 30 * min(max_anchors, 60) and rep["split"] > 20 and rep["empty"] > 0 and rep["pairs_planned"] >= 25
    per_v = np.diff(want["chain_index"])
    assert not per_v[4 * 5:4 * 6].any() and not per_v[4 * 20:4 * 21].any() and not per_v[4 * 33:4 * 34].any()
    if max_anchors == 100:  # anchors from a chunk after the first, on either side
        first = np.asarray(hidx)[np.searchsorted(hidx, want["origin"], side="right") - 1]
        assert (want["origin"] - first >= 128).any()


def test_the_same_batch_behind_a_hit_index_that_does_not_start_at_0_without_bounds():
    pairs, hits, hidx, alns, lens = crossed_case()
    lead = 7
    moved = [[0xFFFFFFFF, 0, 0, 500, 0, 0, 0, 0]] * lead + [list(h) for h in hits]
    want = run_plan(pairs, moved, [h + lead for h in hidx], alns, lens, 5000, min_anchor_score=40, ins_max=300)
    assert want["origin"].min() >= lead and want["report"]["bad_input"] == 0


def test_windows_at_the_edges_of_the_text_of_records_and_of_the_number_formats():
    fw, rv = 0, 1
    mates = [
        ([(30, 80, fw, 50)], []),                                       # 0: forward anchor near 0: the mate lies behind it, nothing to clip
        ([(30, 80, rv, 50)], []),                                       # 1: reverse anchor near 0: clipped at 0
        ([(4900, 4950, fw, 50, 1)], []),                                # 2: forward anchor near n: clipped at n
        ([(2300, 2350, fw, 50, 0)], []),                                # 3: clipped at the end of record 0
        ([(2520, 2570, rv, 50, 1)], []),                                # 4: clipped at the start of record 1
        ([(10, 60, fw, 50, 2)], []),                                    # 5: a ref past the last record: bad input
        ([(1000, 1301, fw, 50)], []),                                   # 6: W = max_width (an anchor longer than the mate)
        ([(1000, 1300, fw, 50)], []),                                   # 7: W = max_width + 1
        ([(1000, 1101, fw, 50)], []),                                   # 8: W = 3 max_width
        ([], [(1000, 1101, rv, 50)]),                                   # 9: the same from mate 2, reverse
        ([(1000, 1050, fw, 50), (1050, 1000, fw, 50), (1200, 1250, rv, 50, 0, 1)], []),  # 10: an empty interval and a supplementary head
    ]
    hits, hidx, alns = pm.batch_of(mates, first_aln=2)
    lens = [50] * (2 * len(mates))
    want = run_plan(flagged(len(mates)), hits, hidx, alns, lens, 5000, bounds=[0, 2500, 5000], ins_max=400, max_width=100)
    per_v = np.diff(want["chain_index"]).reshape(-1, 4)  # (mate 1 forward, mate 1 reverse, mate 2 forward, mate 2 reverse)
    ch = want["chains"]
    at = lambda p, v: ch[want["chain_index"][4 * p + v]:want["chain_index"][4 * p + v + 1]]  # noqa: E731
    assert list(per_v[0]) == [0, 0, 0, 4] and at(0, 3)[0][4] == 30 and at(0, 3)[-1][5] == 430
    assert list(per_v[1]) == [0, 0, 1, 0] and list(at(1, 2)[0]) == [50, 0, 0, 50, 0, 80]
    assert at(2, 3)[0][4] == 4900 and at(2, 3)[-1][5] == 5000
    assert at(3, 3)[-1][5] == 2500 and at(4, 2)[0][4] == 2500
    assert not per_v[5].any() and want["report"]["bad_input"] == 1
    assert [int(per_v[p].sum()) for p in (6, 7, 8, 9)] == [1, 2, 3, 3] and want["report"]["split"] == 6
    assert list(per_v[9]) == [3, 0, 0, 0] and list(per_v[10]) == [0, 0, 0, 4]
    # a read longer than its record, ins_min == ins_max, the largest text
    mates = [([(100, 150, fw, 50, 0)], []), ([(1000, 1050, fw, 50, 1)], []), ([(1300, 1350, rv, 50, 1)], [])]
    hits, hidx, alns = pm.batch_of(mates)
    want = run_plan(flagged(3), hits, hidx, alns, [50, 301, 50, 80, 50, 80], 5000, bounds=[0, 300, 5000], ins_min=250, ins_max=250)
    assert want["report"]["empty"] == 1 and want["report"]["chains"] == 2
    assert [list(c) for c in want["chains"]] == [[50, 0, 0, 80, 1170, 1250], [50, 0, 0, 80, 1100, 1180]]
    mates = [([(TOP - 400, TOP - 250, fw, 100)], []), ([(MAX_N - 60, MAX_N, fw, 100)], []), ([(0, MAX_N, fw, 100)], []),
             ([], [(TOP - 150, TOP, rv, 100)]), ([(MAX_N - 1, MAX_N, rv, 100)], [])]
    hits, hidx, alns = pm.batch_of(mates)
    want = run_plan(flagged(5)[:3], hits[:3], hidx[:7], alns, [150] * 6, MAX_N, ins_max=0xFFFFFFFF, max_width=1024)
    assert want["report"]["chains"] == 2 and want["chains"][:, 5].max() == MAX_N and want["report"]["empty"] == 1
    want = run_plan(flagged(5), hits, hidx, alns, [150] * 10, MAX_N, ins_max=1000, max_width=400)
    assert want["report"]["chains"] == 1 + 3 + 3 and want["chains"][:, 5].max() == MAX_N and want["chains"][:, 4].min() == TOP - 1000


def test_anchors_with_aln_out_of_range_are_skipped_and_counted():
    rng = np.random.default_rng(52)
    case = rm.random_case(rng, [(3, 3), (70, 2), (2, 70), (1, 1), (3, 3)], 2000, ins_max=50)
    hits = [list(h) for h in case["hits"]]
    hidx = case["hit_index"]
    hits[hidx[2] + 1][0] = len(case["alns"])      # pair 1, mate 1: one past the end
    hits[hidx[5] + 2][0] = 0xFFFFFFFF             # pair 2, mate 2: far out
    hits[hidx[6]][0] = len(case["alns"]) + 5      # pair 3
    want = run_plan(flagged(5), hits, hidx, case["alns"], case["lens"], 3000, max_anchors=4, ins_max=400)
    assert want["report"]["bad_input"] == 3 and want["report"]["anchors"] >= 15
    assert not np.isin(want["origin"], [hidx[2] + 1, hidx[5] + 2, hidx[6]]).any()


def test_ten_thousand_light_pairs_beside_one_of_300_by_300():
    rng = np.random.default_rng(53)
    counts = [(300, 300) if p == 7000 else (int(rng.integers(0, 4)), int(rng.integers(0, 4))) for p in range(10001)]
    case = rm.random_case(rng, counts, 3000, ins_max=100)
    case["pairs"][7000, 2] &= ~pm.PROPER  # (300 x 300 hits have a concordant combination: planned all the same)
    want = run_plan(case["pairs"], case["hits"], case["hit_index"], case["alns"], case["lens"], 4000, max_anchors=100, ins_max=300, max_width=64)
    rep = want["report"]
    assert rep["P"] == 10001 and rep["pairs_planned"] > 5000 and rep["max_chains"] > 400 and rep["chains"] > 20000


# ---- (b) the raw device calls: capacity, errors, _dev against _host -----------------------------------------------------------------------
def raw_plan(pairs, hits, hidx, alns, lens, n, Q, cap, params=None, null=(), bounds=None, R=None, ridx=None, want_origin=True, **kw):
    """kiss_hip_fmi_rescue_dev itself -> rc, report, chains (cap x 6), chain_index, origin: -1 where nothing was written"""
    import torch
    import kiss_amd
    from kiss_amd import _lib, fm_rescue
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p

    def up(a, width, dtype=np.uint32):
        a = np.asarray(a, np.int64).reshape(-1, width).astype(dtype)
        return torch.from_numpy((a if a.size else np.zeros((1, width), dtype)).view(np.int32 if dtype == np.uint32 else np.int64)).to(dev)

    d_pairs, d_hits, d_alns = up(pairs, 10), up(hits, 8), up(alns, 12)
    d_hidx = torch.from_numpy(np.asarray(hidx, np.int64)).to(dev)
    if ridx is None:
        ridx = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])
    d_ridx = torch.from_numpy(np.asarray(ridx, np.int64)).to(dev)
    d_bounds = torch.from_numpy(np.asarray(bounds, np.int64)).to(dev) if bounds is not None else None
    d_chains = torch.full((max(cap, 1), 6), -1, dtype=torch.int32, device=dev)
    d_cidx = torch.full((2 * Q + 1,), -1, dtype=torch.int64, device=dev)
    d_origin = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    rep = _lib.RescueReport()
    p = params if params is not None else fm_rescue.rescue_params(**kw)
    ptr = dict(pairs=vp(d_pairs.data_ptr()), hits=vp(d_hits.data_ptr()), hidx=vp(d_hidx.data_ptr()), alns=vp(d_alns.data_ptr()),
               ridx=vp(d_ridx.data_ptr()), chains=vp(d_chains.data_ptr()), cidx=vp(d_cidx.data_ptr()))
    for k in null:
        ptr[k] = None
    n_aln = np.asarray(alns).reshape(-1, 12).shape[0]
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        rc = lib.kiss_hip_fmi_rescue_dev(ctx._ctx, ptr["pairs"], ptr["hits"], ptr["hidx"], Q, ptr["alns"], n_aln, ptr["ridx"], n,
                                         vp(d_bounds.data_ptr()) if d_bounds is not None else None,
                                         (len(bounds) - 1 if bounds is not None else 0) if R is None else R,
                                         ctypes.byref(p) if "params" not in null else None, ptr["chains"], ptr["cidx"],
                                         vp(d_origin.data_ptr()) if want_origin else None, cap, ctypes.byref(rep), None)
    return rc, rep, d_chains.cpu().numpy(), d_cidx.cpu().numpy(), d_origin.cpu().numpy()


def test_capacity_protocol_and_error_contract_of_the_plan_call():
    import kiss_amd
    from kiss_amd import _lib, fm_rescue
    rng = np.random.default_rng(54)
    case = rm.random_case(rng, [(3, 2), (0, 4), (70, 5), (2, 2)], 2000, extra=1, ins_max=50)
    pairs, hits, hidx, alns, lens = flagged(4), case["hits"], case["hit_index"], case["alns"], case["lens"]
    kw = dict(ins_max=400, max_width=100)
    want = rm.plan(pairs, hits, hidx, alns, lens, 3000, **kw)
    C = want["report"]["chains"]
    assert C >= 20
    # room for all: the model's chains, the report, the times; the header's bound suffices; the host entry gives the same
    room = fm_rescue.chain_room(8, len(hits), fm_rescue.rescue_params(**kw))
    assert room >= C
    for cap in (C, room):
        rc, rep, ch, cidx, org = raw_plan(pairs, hits, hidx, alns, lens, 3000, 8, cap, **kw)
        assert rc == 0 and np.array_equal(ch[:C].view(np.uint32).astype(np.int64), want["chains"]) and (ch[C:] == -1).all()
        assert np.array_equal(cidx, want["chain_index"]) and np.array_equal(org[:C], want["origin"])
        assert {k: getattr(rep, k) for k in rm.REPORT_COUNTS} == want["report"] and rep.ms_total > 0 and rep.ms_count > 0
    rc, rep, ch, cidx, org = raw_plan(pairs, hits, hidx, alns, lens, 3000, 8, C, want_origin=False, **kw)
    assert rc == 0 and np.array_equal(ch[:C].view(np.uint32).astype(np.int64), want["chains"]) and (org == -1).all()
    check_plan(kiss_amd.plan_rescue(pairs, np.array(hits, np.int64), hidx, np.array(alns, np.int64), lens, 3000, **kw), want)
    # ... and the host entry without origin
    pr, ht, al = (fm_rescue._records(x, d, "a record") for x, d in ((pairs, fm_rescue.PAIR_DTYPE), (np.array(hits, np.int64), fm_rescue.HIT_DTYPE),
                                                                    (np.array(alns, np.int64), fm_rescue.ALN_DTYPE)))
    hi, ri = np.array(hidx, np.uint64), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ch, ci, rep, p = np.zeros(C, fm_rescue.CHAIN_DTYPE), np.zeros(17, np.uint64), _lib.RescueReport(), fm_rescue.rescue_params(**kw)
    assert _lib.load().kiss_hip_fmi_rescue_host(pr.ctypes.data, ht.ctypes.data, hi.ctypes.data, 8, al.ctypes.data, al.size, ri.ctypes.data, 3000,
                                                None, 0, ctypes.byref(p), ch.ctypes.data, ci.ctypes.data, None, C, ctypes.byref(rep), 0) == 0
    assert np.array_equal(ch.view(np.uint32).reshape(C, 6).astype(np.int64), want["chains"]) and np.array_equal(ci, want["chain_index"])
    assert {k: getattr(rep, k) for k in rm.REPORT_COUNTS} == want["report"]
    # too little room: the totals, nothing written
    for cap in (0, C - 1):
        rc, rep, ch, cidx, org = raw_plan(pairs, hits, hidx, alns, lens, 3000, 8, cap, **kw)
        assert rc == _lib.KISS_HIP_E_INVALID and rep.chains == C and rep.anchors == want["report"]["anchors"]
        assert (ch == -1).all() and (cidx == -1).all() and (org == -1).all()
    # Q odd, an index that decreases, a zero-length read, bad bounds: nothing written
    ridx = np.concatenate([[0], np.cumsum(lens)])
    bad_ridx = ridx.copy()
    bad_ridx[3] = bad_ridx[2]
    for args in (dict(Q=7, hidx=hidx[:8]), dict(hidx=hidx[:3] + [hidx[3] - 1] + hidx[4:]), dict(ridx=bad_ridx),
                 dict(bounds=[1, 3000]), dict(bounds=[0, 1500, 1500, 3000]), dict(bounds=[0, 3001]), dict(bounds=[0, 3000], R=0)):
        a = dict(Q=8, hidx=hidx)
        a.update(args)
        Q = a.pop("Q")
        hi = a.pop("hidx")
        rc, rep, ch, cidx, org = raw_plan(pairs, hits, hi, alns, lens[:Q], 3000, Q, C, **a, **kw)
        assert rc == _lib.KISS_HIP_E_INVALID and (ch == -1).all() and (cidx == -1).all(), args
    with pytest.raises(kiss_amd.KissHipError) as e:
        kiss_amd.plan_rescue(pairs, np.array(hits, np.int64), hidx[:3] + [hidx[3] - 1] + hidx[4:], np.array(alns, np.int64), lens, 3000)
    assert e.value.status == _lib.KISS_HIP_E_INVALID
    with pytest.raises(ValueError):
        kiss_amd.plan_rescue(pairs, np.array(hits, np.int64), hidx[:8], np.array(alns, np.int64), lens[:7], 3000)
    # a required pointer NULL, a parameter out of range, the limits
    for k in ("pairs", "hits", "hidx", "alns", "ridx", "chains", "cidx", "params"):
        assert raw_plan(pairs, hits, hidx, alns, lens, 3000, 8, C, null=(k,), **kw)[0] == _lib.KISS_HIP_E_INVALID, k
    for p in (_lib.RescueParams(10, 9, 4, 0, 960), _lib.RescueParams(0, 9, 0, 0, 960), _lib.RescueParams(0, 9, 4, 0, 0),
              _lib.RescueParams(0, 9, 4, 0, 1025)):
        rc, rep, ch, cidx, org = raw_plan(pairs, hits, hidx, alns, lens, 3000, 8, C, params=p)
        assert rc == _lib.KISS_HIP_E_INVALID and (ch == -1).all() and (cidx == -1).all()
    assert raw_plan(pairs, hits, hidx, alns, lens, MAX_N + 1, 8, C, **kw)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    # no reads; reads without hits
    rc, rep, ch, cidx, org = raw_plan([], [], [0], [], [], 3000, 0, 0)
    assert rc == 0 and list(cidx) == [0] and rep.P == 0
    rc, rep, ch, cidx, org = raw_plan(flagged(2), [], [0] * 5, [], [50] * 4, 3000, 4, 0)
    assert rc == 0 and list(cidx) == [0] * 9 and rep.chains == 0 and rep.P == 2
    res = kiss_amd.plan_rescue(np.zeros((0, 10), np.int64), np.zeros((0, 8), np.int64), [0], np.zeros((0, 12), np.int64), [], 3000)
    assert res["chains"].shape == (0,) and list(res["chain_index"]) == [0]


# ---- (c) the merge ----------------------------------------------------------------------------------------------------------------------------
def merge_case(seed, sizes_a, sizes_b, first_a=0, first_b=0):
    rng = np.random.default_rng(seed)
    ia = np.concatenate([[first_a], first_a + np.cumsum(sizes_a)]).astype(np.int64)
    ib = np.concatenate([[first_b], first_b + np.cumsum(sizes_b)]).astype(np.int64)
    A = rng.integers(0, 1 << 32, (int(np.sum(sizes_a)), 12), dtype=np.int64)
    B = rng.integers(0, 1 << 32, (int(np.sum(sizes_b)), 12), dtype=np.int64)
    oa = np.concatenate([[0], np.cumsum(rng.integers(0, 5, A.shape[0]))]).astype(np.int64)
    ob = np.concatenate([[0], np.cumsum(rng.integers(0, 5, B.shape[0]))]).astype(np.int64)
    ca = rng.integers(0, 1 << 32, int(oa[-1]), dtype=np.int64).astype(np.uint32)
    cb = rng.integers(0, 1 << 32, int(ob[-1]), dtype=np.int64).astype(np.uint32)
    return A, ia, B, ib, ca, oa, cb, ob


def check_merge(res, want, cigar):
    got = np.stack([res["alignments"][k].astype(np.int64) for k in sm.ALN_FIELDS], axis=1).reshape(-1, 12)
    assert np.array_equal(got, want["alignments"]) and np.array_equal(res["chain_index"].astype(np.int64), want["chain_index"])
    assert np.array_equal(res["source"].astype(np.int64), want["source"])
    assert res["report"]["alignments"] == want["alignments"].shape[0]
    if cigar:
        assert np.array_equal(res["cigar"], want["cigar"]) and np.array_equal(res["cigar_index"], want["cigar_index"])
        assert res["report"]["cigar_ops"] == want["cigar"].size
    else:
        assert "cigar" not in res


SIZES = (0, 1, 63, 64, 65)


@pytest.mark.parametrize("cigar", (False, True))
def test_merge_segment_sizes_around_64_on_either_side(cigar):
    import kiss_amd
    sa = [a for a in SIZES for _ in SIZES] + [0, 3]
    sb = [b for _ in SIZES for b in SIZES] + [0, 0]
    for first_a, first_b in ((0, 0), (5, 11)):
        A, ia, B, ib, ca, oa, cb, ob = merge_case(61, sa, sb, first_a, first_b)
        ops = (ca, oa, cb, ob) if cigar else ()
        check_merge(kiss_amd.merge_alignments(A, ia, B, ib, *ops), rm.merge(A, ia, B, ib, *ops), cigar)
    # ops that do not start at 0 in their array: the index says where
    if cigar:
        want = rm.merge(A, ia, B, ib, ca, oa, cb, ob)
        lead = np.arange(9, dtype=np.uint32)
        check_merge(kiss_amd.merge_alignments(A, ia, B, ib, np.concatenate([lead, ca]), oa + 9, cb, ob), want, True)


@pytest.mark.parametrize("cigar", (False, True))
def test_merge_with_either_set_empty_and_with_both(cigar):
    import kiss_amd
    for sa, sb in (([2, 0, 65, 1], [0, 0, 0, 0]), ([0, 0, 0, 0], [2, 0, 65, 1]), ([0, 0], [0, 0]), ([], [])):
        A, ia, B, ib, ca, oa, cb, ob = merge_case(62, sa, sb, 3, 4)
        ops = (ca, oa, cb, ob) if cigar else ()
        res = kiss_amd.merge_alignments(A, ia, B, ib, *ops)
        check_merge(res, rm.merge(A, ia, B, ib, *ops), cigar)
        assert res["report"]["alignments_a"] == sum(sa) and res["report"]["alignments_b"] == sum(sb)


def test_capacity_protocol_and_error_contract_of_the_merge_call():
    import torch
    import kiss_amd
    from kiss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p
    A, ia, B, ib, ca, oa, cb, ob = merge_case(63, [3, 0, 70, 2], [1, 66, 0, 2], 2, 0)
    want = rm.merge(A, ia, B, ib, ca, oa, cb, ob)
    C, O = want["alignments"].shape[0], want["cigar"].size
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(A=A.astype(np.uint32).view(np.int32), B=B.astype(np.uint32).view(np.int32), ia=ia, ib=ib,
                                                          ca=ca.view(np.int32), cb=cb.view(np.int32), oa=oa, ob=ob).items()}

    def call(acap, ocap, cigar=True, ia_=None, oa_=None, null=()):
        d = dict(alns=torch.full((max(acap, 1), 12), -1, dtype=torch.int32, device=dev), cidx=torch.full((5,), -1, dtype=torch.int64, device=dev),
                 src=torch.full((max(acap, 1),), -1, dtype=torch.int32, device=dev), cig=torch.full((max(ocap, 1),), -1, dtype=torch.int32, device=dev),
                 oidx=torch.full((C + 1,), -1, dtype=torch.int64, device=dev))
        tia = torch.from_numpy(np.asarray(ia_, np.int64)).to(dev) if ia_ is not None else t["ia"]
        toa = torch.from_numpy(np.asarray(oa_, np.int64)).to(dev) if oa_ is not None else t["oa"]
        ptr = dict(A=t["A"], ia=tia, B=t["B"], ib=t["ib"], alns=d["alns"], cidx=d["cidx"])
        p = {k: (None if k in null else vp(v.data_ptr())) for k, v in ptr.items()}
        rep = _lib.MergeReport()
        with kiss_amd.Context(max_n=1 << 20) as ctx:
            rc = lib.kiss_hip_fmi_aln_merge_dev(ctx._ctx, p["A"], p["ia"], vp(t["ca"].data_ptr()) if cigar else None,
                                                vp(toa.data_ptr()) if cigar else None, p["B"], p["ib"], vp(t["cb"].data_ptr()) if cigar else None,
                                                vp(t["ob"].data_ptr()) if cigar else None, 4, p["alns"], acap, p["cidx"], vp(d["src"].data_ptr()),
                                                vp(d["cig"].data_ptr()) if cigar else None, vp(d["oidx"].data_ptr()) if cigar else None,
                                                ocap if cigar else 0, ctypes.byref(rep), None)
        return rc, rep, {k: v.cpu().numpy() for k, v in d.items()}

    rc, rep, d = call(C, O)
    assert rc == 0 and rep.alignments == C and rep.cigar_ops == O and rep.ms_total > 0
    assert np.array_equal(d["alns"].view(np.uint32).astype(np.int64), want["alignments"]) and np.array_equal(d["cidx"], want["chain_index"])
    assert np.array_equal(d["src"], want["source"]) and np.array_equal(d["cig"].view(np.uint32), want["cigar"])
    assert np.array_equal(d["oidx"].view(np.uint64), want["cigar_index"])
    for acap, ocap in ((C - 1, O), (C, O - 1), (0, 0)):
        rc, rep, d = call(acap, ocap)
        assert rc == _lib.KISS_HIP_E_INVALID and rep.alignments == C and rep.cigar_ops == O
        assert all((v == -1).all() for v in d.values()), (acap, ocap)
    rc, rep, d = call(C, 0, cigar=False)
    assert rc == 0 and np.array_equal(d["alns"].view(np.uint32).astype(np.int64), want["alignments"]) and (d["cig"] == -1).all()
    # the host entry: short capacities give the totals, then the call with room, with and without source
    from kiss_amd import fm_rescue
    h = {k: np.ascontiguousarray(v, np.uint64) for k, v in dict(ia=ia, ib=ib, oa=oa, ob=ob).items()}
    h.update(A=fm_rescue._records(A, fm_rescue.ALN_DTYPE, "an alignment record"), B=fm_rescue._records(B, fm_rescue.ALN_DTYPE, "an alignment record"),
             ca=np.ascontiguousarray(ca, np.uint32), cb=np.ascontiguousarray(cb, np.uint32))

    def host(acap, ocap, source=True):
        o = dict(alns=np.zeros((max(acap, 1), 12), np.uint32), cidx=np.full(5, 7, np.uint64), src=np.full(max(acap, 1), 7, np.uint32),
                 cig=np.zeros(max(ocap, 1), np.uint32), oidx=np.full(C + 1, 7, np.uint64))
        rep = _lib.MergeReport()
        rc = lib.kiss_hip_fmi_aln_merge_host(h["A"].ctypes.data, h["ia"].ctypes.data, h["ca"].ctypes.data, h["oa"].ctypes.data, h["B"].ctypes.data,
                                             h["ib"].ctypes.data, h["cb"].ctypes.data, h["ob"].ctypes.data, 4, o["alns"].ctypes.data, acap,
                                             o["cidx"].ctypes.data, o["src"].ctypes.data if source else None, o["cig"].ctypes.data,
                                             o["oidx"].ctypes.data, ocap, ctypes.byref(rep), 0)
        return rc, rep, o

    rc, rep, o = host(0, 0)
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.alignments, rep.cigar_ops) == (C, O)
    for source in (True, False):
        rc, rep, o = host(C, O, source)
        assert rc == 0 and np.array_equal(o["alns"].astype(np.int64), want["alignments"]) and np.array_equal(o["cidx"], want["chain_index"])
        assert np.array_equal(o["cig"], want["cigar"]) and np.array_equal(o["oidx"], want["cigar_index"])
        assert np.array_equal(o["src"], want["source"]) if source else (o["src"] == 7).all()
    # an index that decreases, a required pointer NULL
    bad = ia.copy()
    bad[2] = bad[1] - 1
    rc, rep, d = call(C, O, ia_=bad)
    assert rc == _lib.KISS_HIP_E_INVALID and all((v == -1).all() for v in d.values())
    bad = oa.copy()
    bad[4] = bad[3] - 1
    rc, rep, d = call(C, O, oa_=bad)
    assert rc == _lib.KISS_HIP_E_INVALID and all((v == -1).all() for v in d.values())
    for k in ("A", "ia", "B", "ib", "alns", "cidx"):
        assert call(C, O, null=(k,))[0] == _lib.KISS_HIP_E_INVALID, k
    with pytest.raises(ValueError):
        kiss_amd.merge_alignments(A, ia, B, ib, ca, oa)


# ---- (d) FMIndex.map_pairs(rescue=...) stage by stage --------------------------------------------------------------------------------------
RESCUE_SETS = ((dict(ins_max=400), True), (dict(ins_min=100, ins_max=350, ins_mean=250), dict(max_anchors=2, min_anchor_score=30, max_width=128)))


def rows(arr, fields):
    return np.stack([arr[k].astype(np.int64) for k in fields], axis=1).reshape(-1, len(fields))


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_every_stage_of_a_rescue_equals_its_model_on_the_output_of_the_stage_before(name, which):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import check as check_pairs, mates_of
    f = index_of(name, 4)
    S = text(name)
    m1, m2 = mates_of(name)
    reads = [r for pr in zip(m1, m2) for r in pr]
    lens = [len(r) for r in reads]
    pp, rescue = RESCUE_SETS[which]
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20))
    res = f.map_pairs(m1, m2, S, 15, 0, 200, rescue=rescue, **common, **pp)
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, **common, **pp)
    first, rs = res["first_pass"], res["rescue"]
    CA = first["alignments"]
    src = res["aln_source"].astype(np.int64)
    # pass 1 is what map_pairs gives without rescue
    assert CA == plain["alignments"].size and res["chains"].tobytes() == plain["chains"].tobytes()
    for k in ("pairs", "hits", "hit_index"):
        assert first[k].tobytes() == plain[k].tobytes(), k
    assert res["alignments"][src < CA].tobytes() == plain["alignments"].tobytes()
    # the plan on pass 1
    rp = dict(ins_min=pp.get("ins_min", 0), ins_max=pp["ins_max"])
    rp.update(rescue if isinstance(rescue, dict) else {})
    want = rm.plan(first["pairs"], first["hits"], first["hit_index"], plain["alignments"], lens, S.size, **rp)
    check_plan(rs, want)
    # the rescue chains aligned
    alns_b = res["alignments"][src >= CA]
    al = am.align(S, reads, want["chains"][:, 2:6], want["chain_index"], True)
    assert np.array_equal(rows(alns_b, am.FIELDS), al["alignments"])
    assert {k: rs["align_report"][k] for k in ("cells", "aligned", "too_wide", "max_band")} == {k: al[k] for k in ("cells", "aligned", "too_wide", "max_band")}
    # merged
    mg = rm.merge(plain["alignments"], plain["chain_index"], alns_b, want["chain_index"], plain["cigar"], plain["cigar_index"], al["cigar"],
                  al["cigar_index"])
    assert np.array_equal(rows(res["alignments"], am.FIELDS), mg["alignments"]) and np.array_equal(src, mg["source"])
    assert np.array_equal(res["chain_index"].astype(np.int64), mg["chain_index"])
    assert np.array_equal(res["cigar"], mg["cigar"]) and np.array_equal(res["cigar_index"], mg["cigar_index"])
    assert rs["merge_report"]["alignments"] == src.size and rs["merge_report"]["cigar_ops"] == mg["cigar"].size
    # pass 2
    sel = sm.select(res["alignments"], res["chain_index"], lens, both_strands=True, min_score=20)
    assert np.array_equal(rows(res["hits"], sm.HIT_FIELDS), sel["hits"]) and np.array_equal(res["hit_index"].astype(np.int64), sel["hit_index"])
    assert {k: res["select_report"][k] for k in sm.REPORT_COUNTS} == sel["report"]
    check_pairs(res, pm.pair(res["hits"], res["hit_index"], res["alignments"], **pp), key="pair_report")
    # a pair that was proper keeps its record, up to the numbers of its hits and their alignments
    p1, p2 = rows(first["pairs"], pm.PAIR_FIELDS), rows(res["pairs"], pm.PAIR_FIELDS)
    was = (p1[:, 2] & pm.PROPER) != 0
    assert np.array_equal(p1[was, 2:], p2[was, 2:])
    for p in np.flatnonzero(was):
        for k in (0, 1):
            h1, h2 = first["hits"][p1[p, k]], res["hits"][p2[p, k]]
            assert src[h2["aln"]] == h1["aln"] and [h1[x] for x in sm.HIT_FIELDS[1:]] == [h2[x] for x in sm.HIT_FIELDS[1:]]
            assert p2[p, k] - res["hit_index"][2 * p + k] == p1[p, k] - first["hit_index"][2 * p + k]
    assert rs["rescued"] == int((((p2[:, 2] & pm.PROPER) != 0) & ~was).sum())
    if name in ("genome", "iid"):
        assert rs["report"]["pairs_planned"] >= 2 and rs["report"]["chains"] >= 2
    assert f.map_pairs(m1, m2, S, 15, 0, 200, rescue=None, **common, **pp).keys() == plain.keys()
    with pytest.raises(TypeError):
        f.map_pairs(m1, m2, S, rescue=dict(overlap=3))


# ---- (e) against the truth ------------------------------------------------------------------------------------------------------------------
TRUTH_SEED = 71
TRUTH_PAIR = dict(ins_max=400)


def revcomp(R):
    return (3 - np.asarray(R, np.uint8)[::-1]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rescue_truth_case():
    """A random text of 20 000 bases that holds a 500-base block twice, 10 000 bases apart; mates of 100 bases, fragments of
    250..380.  A damaged mate carries a substitution every 12th base (bases 5, 17, ..., 89: its longest exact match is 11
    bases, so it has no seed; 92 matches and 8 mismatches score 60).
    (A) 20 pairs anywhere outside the blocks: the damaged mate is the reverse one in even pairs and the forward one in odd
    pairs, the mates swapped in every second pair of pairs.  (B) 10 pairs whose damaged mate lies wholly inside the block -- its
    true copy alternating -- and whose partner lies wholly in the unique flank.  (C) 5 pairs whose second mate is random bases.
    -> text, mates 1, mates 2, truth: [(kind, the damaged mate (0 / 1), its true tbeg, its true tend)]"""
    rng = np.random.default_rng(TRUTH_SEED)
    S = rng.integers(0, 4, 20000, dtype=np.uint8)
    S[12000:12500] = S[2000:2500]

    def damaged(R):
        R = R.copy()
        for j in range(5, 100, 12):
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        return R

    def fragment(a, frag, hurt_reverse, swap):
        fwd, rev = S[a:a + 100], S[a + frag - 100:a + frag]
        fwd, rev = (fwd, damaged(rev)) if hurt_reverse else (damaged(fwd), rev)
        mates = (revcomp(rev), fwd) if swap else (fwd, revcomp(rev))
        which = (0 if swap else 1) if hurt_reverse else (1 if swap else 0)
        at = a + frag - 100 if hurt_reverse else a
        return mates, (which, at, at + 100)

    m1, m2, truth = [], [], []
    for p in range(20):
        frag = int(rng.integers(250, 381))
        a = int(rng.integers(3000, 11000 - frag))
        (x, y), t = fragment(a, frag, p % 2 == 0, (p // 2) % 2 == 1)
        m1.append(x), m2.append(y), truth.append(("A",) + t)
    for p in range(10):
        B = 12000 if p % 2 else 2000
        if (p // 2) % 2 == 0:  # the forward mate damaged, at the end of the block; its partner behind the block
            a = int(rng.integers(B + 320, B + 401))
            frag = int(rng.integers(max(250, B + 600 - a), 381))
            (x, y), t = fragment(a, frag, False, p % 3 == 0)
            assert B <= a and a + 100 <= B + 500 <= a + frag - 100
        else:                  # the reverse mate damaged, at the start of the block; its partner in front of the block
            e = int(rng.integers(B + 100, B + 181))
            frag = int(rng.integers(max(250, e - B + 100), 381))
            (x, y), t = fragment(e - frag, frag, True, p % 3 == 0)
            assert B <= e - 100 and e <= B + 500 and e - frag + 100 <= B
        m1.append(x), m2.append(y), truth.append(("B",) + t)
    for p in range(5):
        a = int(rng.integers(13000, 19000))
        m1.append(S[a:a + 100].copy()), m2.append(rng.integers(0, 4, 100, dtype=np.uint8)), truth.append(("C", 1, 0, 0))
    return S, m1, m2, truth


def assert_rescue_truth(pairs1, pairs2, hits1, hits2, alns2, source, CA, truth):
    """the conditions of the issue, for EVERY pair.  pairs1 / pairs2: rows of PAIR_FIELDS of pass 1 and pass 2; hits1 / hits2: rows
    of HIT_FIELDS; alns2: rows of the merged alignment records; source: per merged alignment"""
    for p, (kind, which, tbeg, tend) in enumerate(truth):
        r1 = dict(zip(pm.PAIR_FIELDS, (int(v) for v in pairs1[p])))
        r2 = dict(zip(pm.PAIR_FIELDS, (int(v) for v in pairs2[p])))
        assert not r1["flags"] & pm.PROPER, (p, r1)          # without rescue no pair is proper
        if kind == "C":                                     # stays as pass 1 left it
            assert {k: r1[k] for k in pm.PAIR_FIELDS[2:]} == {k: r2[k] for k in pm.PAIR_FIELDS[2:]}, (p, r1, r2)
            assert r2["hit2"] == pm.NONE and int(source[hits2[r2["hit1"]][0]]) == hits1[r1["hit1"]][0]
            continue
        assert r2["flags"] & pm.PROPER, (p, kind, r2)        # with rescue every pair is proper
        h = hits2[r2["hit2" if which else "hit1"]]
        a = alns2[h[0]]
        assert int(a[5]) == tend, (p, kind, int(a[4]), int(a[5]), tbeg, tend)  # the damaged mate ends at its true end
        assert int(source[h[0]]) >= CA, (p, kind)           # its SAM line would carry YR:i:1
        assert int(a[0]) == 60 and abs(int(a[4]) - tbeg) <= 5, (p, kind, a)
        other = hits2[r2["hit1" if which else "hit2"]]
        assert int(source[other[0]]) < CA
        if kind == "B":                                     # the true copy, at MAPQ 60
            assert r2["mapq2" if which else "mapq1"] == 60 and r2["mapq1" if which else "mapq2"] == 60, (p, r2)


def test_against_the_truth_a_mate_without_a_seed_is_found_next_to_its_partner():
    """(A) 20 pairs, one mate with a substitution every 12th base, mates swapped in every second pair of pairs: without rescue no
    pair is proper, with rescue every pair is, the damaged mate ends at its true end and comes from a rescue chain (YR:i:1).
    (B) 10 pairs whose damaged mate lies in a block that occurs twice: the true copy, at MAPQ 60.  (C) 5 pairs whose second mate
    is random bases stay as pass 1 left them.  The conditions hold on this seed in the composed CPU models:
    tests/test_fm_rescue_truth_model.py."""
    import kiss_amd
    import kiss_amd.fm_index as fm
    S, m1, m2, truth = rescue_truth_case()
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    plain = f.map_pairs(m1, m2, S, **TRUTH_PAIR)
    res = f.map_pairs(m1, m2, S, rescue=True, **TRUTH_PAIR)
    f.close()
    assert plain["pair_report"]["proper"] == 0 and res["first_pass"]["pairs"].tobytes() == plain["pairs"].tobytes()
    assert_rescue_truth(rows(res["first_pass"]["pairs"], pm.PAIR_FIELDS), rows(res["pairs"], pm.PAIR_FIELDS),
                        rows(res["first_pass"]["hits"], pm.HIT_FIELDS), rows(res["hits"], pm.HIT_FIELDS), rows(res["alignments"], am.FIELDS),
                        res["aln_source"], res["first_pass"]["alignments"], truth)
    assert res["pair_report"]["proper"] == 30 and res["rescue"]["rescued"] == 30 and res["rescue"]["report"]["pairs_planned"] == 35
