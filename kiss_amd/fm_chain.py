"""Chaining of seed anchors into candidate loci (kiss_hip_fmi_chain_dev / _host; include/kiss_hip.h has the definition).

chain_seeds() takes numpy arrays -- anchors from anywhere -- and runs the host entry; FMIndex.chains() keeps the output of
the seeds call on the device and runs the device entry (chain_dev).  All arithmetic runs in libkiss_hip.so; there is no
CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, make_params, record_dtype, record_view, records, sized
from .sorter import _check

CHAIN_DEFAULTS = dict(max_gap=5000, band=500, gap_cost=2, max_lookback=64, min_score=40)
CHAIN_DTYPE = record_dtype(_lib.Chain)
ANCHOR_DTYPE = record_dtype(_lib.ChainAnchor)
SEED_DTYPE = record_dtype(_lib.FmiSeed)


def chain_params(**params):
    """kiss_hip_chain_params from keywords; the defaults are CHAIN_DEFAULTS"""
    p = make_params("chain", CHAIN_DEFAULTS, params)
    if p["max_gap"] > 0x7FFFFFFF or p["band"] > 0x7FFFFFFF or p["gap_cost"] > 65535:
        raise ValueError("max_gap and band are at most 2^31 - 1, gap_cost at most 65535")
    return _lib.ChainParams(**p)


def _raise(rc, rep, where, ctx=None):
    if rc == _lib.KISS_HIP_E_UNSUPPORTED:
        raise _lib.KissHipError(rc, where, "%d anchors are more than one call sorts: split the batch" % rep.anchors)
    _check(rc, where, ctx)


def chain_dev(lib, ctx, device, d_seeds, d_sidx, V, d_pos, d_pidx, params, want_anchors):
    """the device entry on torch tensors of the seeds call -> dict of torch tensors and the report; two calls, the first one
    sizes the output (the C interface's convention)"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.ChainReport()
    d_cidx = torch.zeros(V + 1, dtype=torch.int64, device=dev)

    def call(d_chains, ccap, d_anc, d_aidx, acap):
        return lib.kiss_hip_fmi_chain_dev(ctx._ctx, vp(d_seeds.data_ptr()), vp(d_sidx.data_ptr()), V, vp(d_pos.data_ptr()),
                                          vp(d_pidx.data_ptr()), ctypes.byref(params), vp(d_chains.data_ptr()),
                                          vp(d_cidx.data_ptr()), ccap, vp(d_anc.data_ptr()) if d_anc is not None else None,
                                          vp(d_aidx.data_ptr()) if d_aidx is not None else None, acap, ctypes.byref(rep), None)

    def room(n=0, m=0):
        d_chains = torch.zeros((max(n, 1), 6), dtype=torch.int32, device=dev)
        if not (n and want_anchors):
            return d_chains, n, None, None, 0
        return (d_chains, n, torch.zeros((max(m, 1), 3), dtype=torch.int32, device=dev),
                torch.zeros(n + 1, dtype=torch.int64, device=dev), m)

    rc, (d_chains, n, d_anc, d_aidx, _) = sized(call, room, rep, "chains", "chain_anchors")
    if rc == _lib.KISS_HIP_OK and want_anchors and not n:  # no chains at all
        d_anc = torch.zeros((1, 3), dtype=torch.int32, device=dev)
        d_aidx = torch.zeros(1, dtype=torch.int64, device=dev)
    _raise(rc, rep, "kiss_hip_fmi_chain_dev", ctx._ctx)
    return {"d_chains": d_chains, "d_cidx": d_cidx, "d_anc": d_anc, "d_aidx": d_aidx, "rep": rep}


def chain_arrays(out, want_anchors):
    """the tensors of chain_dev as numpy"""
    rep = out["rep"]
    res = {"chains": record_view(out["d_chains"], int(rep.chains), CHAIN_DTYPE), "chain_index": out["d_cidx"].cpu().numpy().view(np.uint64)}
    if want_anchors:
        res["anchors"] = record_view(out["d_anc"], int(rep.chain_anchors), ANCHOR_DTYPE)
        res["anchor_index"] = out["d_aidx"].cpu().numpy().view(np.uint64)
    res["report"] = rep.as_dict()
    return res


def chain_seeds(seeds, seed_index, positions, pos_index, want_anchors=True, device=0, hooks=None, **params):
    """Chain anchors given as the arrays of the seeds call (numpy in, numpy out): seeds is its structured array (start, len,
    sa_beg, sa_end) or an (n, 2) array of (start, len); seed_index has V + 1 entries, pos_index seeds + 1; params as in
    FMIndex.chains.  Returns dict(chains, chain_index, report) and, with want_anchors, anchors / anchor_index."""
    p = chain_params(**params)
    sd = records(seeds, SEED_DTYPE, "start and len are u32", columns=("start", "len"))
    sidx = np.ascontiguousarray(seed_index, dtype=np.uint64)
    pidx = np.ascontiguousarray(pos_index, dtype=np.uint64)
    pos = np.ascontiguousarray(positions, dtype=np.uint32)
    if sidx.ndim != 1 or sidx.size < 1 or pidx.ndim != 1:
        raise ValueError("seed_index has V + 1 entries, pos_index seeds + 1")
    V = sidx.size - 1
    if int(sidx.max()) > sd.size or pidx.size < int(sidx.max()) + 1 or (pidx.size and int(pidx.max()) > pos.size):
        raise ValueError("seed_index points past the seeds, or pos_index past the positions")
    lib = _lib.load(hooks)
    rep = _lib.ChainReport()
    cidx = np.zeros(V + 1, np.uint64)
    (sp, pp), hold = addresses(sd, pos)

    def call(chains, ccap, anc, aidx, acap):
        return lib.kiss_hip_fmi_chain_host(sp, sidx.ctypes.data, V, pp, pidx.ctypes.data, ctypes.byref(p),
                                           chains.ctypes.data, cidx.ctypes.data, ccap, anc.ctypes.data if anc is not None else None,
                                           aidx.ctypes.data if aidx is not None else None, acap, ctypes.byref(rep), int(device))

    def room(n=0, m=0):
        chains = np.zeros(max(n, 1), CHAIN_DTYPE)
        if not (n and want_anchors):
            return chains, n, None, None, 0
        return chains, n, np.zeros(max(m, 1), ANCHOR_DTYPE), np.zeros(n + 1, np.uint64), m

    rc, (chains, _, anc, aidx, _) = sized(call, room, rep, "chains", "chain_anchors")
    _raise(rc, rep, "kiss_hip_fmi_chain_host")
    n, m = int(rep.chains), int(rep.chain_anchors)
    res = {"chains": chains[:n], "chain_index": cidx}
    if want_anchors:
        res["anchors"] = anc[:m] if anc is not None else np.zeros(0, ANCHOR_DTYPE)
        res["anchor_index"] = aidx if aidx is not None else np.zeros(1, np.uint64)
    res["report"] = rep.as_dict()
    return res
