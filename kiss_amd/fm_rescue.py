"""Mate rescue: the pairs that are not proper turned into windows next to the hits of either mate (kiss_hip_fmi_rescue_dev /
_host), and two alignment sets of one batch made one (kiss_hip_fmi_aln_merge_dev / _host; include/kiss_hip.h has the
definitions).

plan_rescue() and merge_alignments() take numpy arrays and run the host entries; FMIndex.map_pairs(rescue=...) keeps
everything on the device and runs the device entries (rescue_dev, merge_dev).  All arithmetic runs in libkiss_hip.so; there
is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, check_mates, lengths_index, make_params, record_view, records, sized
from .fm_align import ALIGN_MAX_BAND, ALN_DTYPE
from .fm_chain import CHAIN_DTYPE
from .fm_pair import PAIR_DTYPE, _records  # noqa: F401
from .fm_select import HIT_DTYPE, _bounds_array
from .sorter import _check

RESCUE_DEFAULTS = dict(ins_min=0, ins_max=1000, max_anchors=4, min_anchor_score=0, max_width=960)
RESCUE_LIMITS = dict(max_width=ALIGN_MAX_BAND)


def rescue_params(**params):
    """kiss_hip_rescue_params from keywords; the defaults are RESCUE_DEFAULTS"""
    p = make_params("rescue", RESCUE_DEFAULTS, params)
    if p["ins_min"] > p["ins_max"]:
        raise ValueError("ins_min is at most ins_max")
    if p["max_anchors"] < 1:
        raise ValueError("max_anchors is at least 1")
    if not 1 <= p["max_width"] <= RESCUE_LIMITS["max_width"]:
        raise ValueError("max_width is at least 1 and at most %d" % RESCUE_LIMITS["max_width"])
    return _lib.RescueParams(**p)


def chain_room(Q, hits, params):
    """a chain_capacity that always suffices: no anchor is used twice, and a window has at most ins_max - ins_min + 1
    diagonals"""
    per = (params.ins_max - params.ins_min + params.max_width) // params.max_width
    return min(Q * params.max_anchors, hits) * per


def rescue_dev(lib, ctx, device, d_pairs, d_hits, d_hidx, Q, d_alns, aln_count, d_ridx, n, bounds, params, hits):
    """the plan's device entry on torch tensors -> dict of torch tensors and the report; two calls, the first one sizes the
    chains (the C interface's convention).  hits: hit_index[Q]"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.RescueReport()
    b = _bounds_array(bounds)
    d_bounds = torch.from_numpy(b.view(np.int64)).to(dev) if b is not None else None
    R = b.size - 1 if b is not None else 0
    d_cidx = torch.zeros(2 * Q + 1, dtype=torch.int64, device=dev)

    def call(d_chains, d_origin, cap):
        return lib.kiss_hip_fmi_rescue_dev(ctx._ctx, vp(d_pairs.data_ptr()), vp(d_hits.data_ptr()), vp(d_hidx.data_ptr()), Q,
                                           vp(d_alns.data_ptr()), aln_count, vp(d_ridx.data_ptr()), n,
                                           vp(d_bounds.data_ptr()) if d_bounds is not None else None, R, ctypes.byref(params),
                                           vp(d_chains.data_ptr()), vp(d_cidx.data_ptr()), vp(d_origin.data_ptr()), cap,
                                           ctypes.byref(rep), None)

    def room(total=0):
        return (torch.zeros((max(total, 1), 6), dtype=torch.int32, device=dev),
                torch.zeros(max(total, 1), dtype=torch.int32, device=dev), total)

    rc, (d_chains, d_origin, _) = sized(call, room, rep, "chains")
    _check(rc, "kiss_hip_fmi_rescue_dev", ctx._ctx)
    return {"d_chains": d_chains, "d_cidx": d_cidx, "d_origin": d_origin, "rep": rep, "C": int(rep.chains)}


def rescue_arrays(out):
    """the tensors of rescue_dev as numpy"""
    C = out["C"]
    return {"chains": record_view(out["d_chains"], C, CHAIN_DTYPE), "chain_index": out["d_cidx"].cpu().numpy().view(np.uint64),
            "origin": out["d_origin"][:C].cpu().numpy().view(np.uint32), "report": out["rep"].as_dict()}


def merge_dev(lib, ctx, device, V, a, b, want_cigar):
    """the merge's device entry on torch tensors.  a, b: dicts with d_alns, d_cidx, C and, with want_cigar, d_cigar, d_oidx
    and ops (the number of ops) -> dict of torch tensors and the report; capacities are known, so one call"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.MergeReport()
    C = a["C"] + b["C"]
    ops = a["ops"] + b["ops"] if want_cigar else 0
    d_alns = torch.zeros((max(C, 1), 12), dtype=torch.int32, device=dev)
    d_cidx = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    d_src = torch.zeros(max(C, 1), dtype=torch.int32, device=dev)
    d_cig = torch.zeros(max(ops, 1), dtype=torch.int32, device=dev) if want_cigar else None
    d_oidx = torch.zeros(C + 1, dtype=torch.int64, device=dev) if want_cigar else None

    def ptr(t):
        return vp(t.data_ptr()) if t is not None else None

    _check(lib.kiss_hip_fmi_aln_merge_dev(ctx._ctx, ptr(a["d_alns"]), ptr(a["d_cidx"]), ptr(a["d_cigar"] if want_cigar else None),
                                          ptr(a["d_oidx"] if want_cigar else None), ptr(b["d_alns"]), ptr(b["d_cidx"]),
                                          ptr(b["d_cigar"] if want_cigar else None), ptr(b["d_oidx"] if want_cigar else None), V,
                                          ptr(d_alns), C, ptr(d_cidx), ptr(d_src), ptr(d_cig), ptr(d_oidx), ops, ctypes.byref(rep),
                                          None), "kiss_hip_fmi_aln_merge_dev", ctx._ctx)
    return {"d_alns": d_alns, "d_cidx": d_cidx, "d_source": d_src, "d_cigar": d_cig, "d_oidx": d_oidx, "rep": rep, "C": C}


def merge_arrays(out, want_cigar):
    """the tensors of merge_dev as numpy"""
    C = out["C"]
    res = {"alignments": record_view(out["d_alns"], C, ALN_DTYPE),
           "chain_index": out["d_cidx"].cpu().numpy().view(np.uint64), "aln_source": out["d_source"][:C].cpu().numpy().view(np.uint32)}
    if want_cigar:
        res["cigar"] = out["d_cigar"][:int(out["rep"].cigar_ops)].cpu().numpy().view(np.uint32)
        res["cigar_index"] = out["d_oidx"].cpu().numpy().view(np.uint64)
    return res


def plan_rescue(pairs, hits, hit_index, alignments, read_lengths, n, bounds=None, device=0, hooks=None, **params):
    """Plan the rescue of the pairs that are not proper from arrays (numpy in, numpy out).  pairs: the structured array of the
    pair call, or a (P, 10) integer array in the order of its fields (only flags is read); hits / hit_index / alignments as
    pair_hits() takes them; read_lengths: the Q read lengths, reads 2 p and 2 p + 1 the mates of pair p; n: the length of the
    text; bounds: the R + 1 record starts of the text, None: one record; params: ins_min (0), ins_max (1000), max_anchors (4),
    min_anchor_score (0), max_width (960).  Returns dict(chains: structured array of the fields of kiss_hip_chain -- what
    align_chains() takes --, chain_index: 2 Q + 1 u64 over the virtual reads of both strands, origin: per chain the index of
    its anchor in hits, report)."""
    p = rescue_params(**params)
    pr = records(pairs, PAIR_DTYPE, "the fields of a pair are u32")
    ht = records(hits, HIT_DTYPE, "the fields of a hit are u32")
    al = records(alignments, ALN_DTYPE, "the fields of an alignment record are u32")
    hidx = np.ascontiguousarray(hit_index, dtype=np.uint64).ravel()
    ridx = lengths_index(read_lengths)
    Q = ridx.size - 1
    if hidx.size != Q + 1:
        raise ValueError("hit_index has Q + 1 = %d entries" % (Q + 1))
    check_mates(Q)
    if pr.size < Q // 2:
        raise ValueError("%d pairs, %d pair records given" % (Q // 2, pr.size))
    if np.all(hidx[1:] >= hidx[:-1]) and int(hidx[-1]) > ht.size:
        raise ValueError("hit_index spans %d hits, %d given" % (int(hidx[-1]), ht.size))
    b = _bounds_array(bounds)
    lib = _lib.load(hooks)
    rep = _lib.RescueReport()
    cidx = np.zeros(2 * Q + 1, np.uint64)
    (pp, hp, ap), hold = addresses(pr, ht, al)

    def call(chains, origin, cap):
        return lib.kiss_hip_fmi_rescue_host(pp, hp, hidx.ctypes.data, Q, ap, al.size,
                                            ridx.ctypes.data, int(n), b.ctypes.data if b is not None else None, b.size - 1 if b is not None else 0,
                                            ctypes.byref(p), chains.ctypes.data, cidx.ctypes.data, origin.ctypes.data, cap,
                                            ctypes.byref(rep), int(device))

    rc, (chains, origin, _) = sized(call, lambda m=0: (np.zeros(max(m, 1), CHAIN_DTYPE), np.zeros(max(m, 1), np.uint32), m), rep, "chains")
    _check(rc, "kiss_hip_fmi_rescue_host")
    C = int(rep.chains)
    return {"chains": chains[:C], "chain_index": cidx, "origin": origin[:C], "report": rep.as_dict()}


def merge_alignments(alignments_a, chain_index_a, alignments_b, chain_index_b, cigar_a=None, cigar_index_a=None, cigar_b=None,
                     cigar_index_b=None, device=0, hooks=None):
    """Two alignment sets over the same virtual reads made one (numpy in, numpy out): every virtual read gets all of A's
    alignments in their order, then all of B's.  alignments_*: structured arrays of the align call or (C, 12) integers;
    chain_index_*: V + 1 entries each; the ops of both sets (cigar_* with cigar_index_*) or of neither.  Returns
    dict(alignments, chain_index (from 0), source (i for alignments_a[i], C_A + j for alignments_b[j]), report) and, with the
    ops, cigar / cigar_index."""
    A = records(alignments_a, ALN_DTYPE, "the fields of an alignment record are u32")
    B = records(alignments_b, ALN_DTYPE, "the fields of an alignment record are u32")
    ia = np.ascontiguousarray(chain_index_a, dtype=np.uint64).ravel()
    ib = np.ascontiguousarray(chain_index_b, dtype=np.uint64).ravel()
    if ia.size < 1 or ia.size != ib.size:
        raise ValueError("both chain indices have V + 1 entries")
    V = ia.size - 1
    given = [x is not None for x in (cigar_a, cigar_index_a, cigar_b, cigar_index_b)]
    if any(given) and not all(given):
        raise ValueError("the ops of both sets (cigar and cigar_index each), or of neither")
    want = all(given)

    def span(idx):
        return int(idx[-1]) - int(idx[0]) if int(idx[-1]) >= int(idx[0]) else 0

    CA, CB = span(ia), span(ib)
    if CA > A.size or CB > B.size:
        raise ValueError("a chain index spans more alignments than were given")
    C = CA + CB
    ops = 0
    ptrs = [None] * 4
    hold = []
    if want:
        for k, (cig, oi, cnt) in enumerate(((cigar_a, cigar_index_a, CA), (cigar_b, cigar_index_b, CB))):
            cig = np.ascontiguousarray(cig, dtype=np.uint32).ravel()
            oi = np.ascontiguousarray(oi, dtype=np.uint64).ravel()
            if oi.size < cnt + 1 or (np.all(oi[1:] >= oi[:-1]) and int(oi[cnt]) > cig.size):
                raise ValueError("a cigar index has C + 1 entries and points inside its ops")
            ptrs[2 * k:2 * k + 2], kept = addresses(cig, oi)
            hold += kept
            ops += span(oi[:cnt + 1])
    lib = _lib.load(hooks)
    rep = _lib.MergeReport()
    alns = np.zeros(max(C, 1), ALN_DTYPE)
    cidx = np.zeros(V + 1, np.uint64)
    src = np.zeros(max(C, 1), np.uint32)
    cig = np.zeros(max(ops, 1), np.uint32) if want else None
    oidx = np.zeros(C + 1, np.uint64) if want else None
    (pa, pb), kept = addresses(A, B)
    _check(lib.kiss_hip_fmi_aln_merge_host(pa, ia.ctypes.data, ptrs[0], ptrs[1], pb, ib.ctypes.data, ptrs[2], ptrs[3], V,
                                           alns.ctypes.data, C, cidx.ctypes.data, src.ctypes.data,
                                           cig.ctypes.data if want else None, oidx.ctypes.data if want else None, ops,
                                           ctypes.byref(rep), int(device)), "kiss_hip_fmi_aln_merge_host")
    res = {"alignments": alns[:C], "chain_index": cidx, "source": src[:C], "report": rep.as_dict()}
    if want:
        res["cigar"] = cig[:int(rep.cigar_ops)]
        res["cigar_index"] = oidx
    return res
