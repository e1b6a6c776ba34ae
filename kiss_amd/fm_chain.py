"""Chaining of seed anchors into candidate loci (kiss_hip_fmi_chain_dev / _host; include/kiss_hip.h has the definition).

chain_seeds() takes numpy arrays -- anchors from anywhere -- and runs the host entry; FMIndex.chains() keeps the output of
the seeds call on the device and runs the device entry (chain_dev).  All arithmetic runs in libkiss_hip.so; there is no
CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from .sorter import _check

CHAIN_DEFAULTS = dict(max_gap=5000, band=500, gap_cost=2, max_lookback=64, min_score=40)
CHAIN_DTYPE = np.dtype([(k, np.uint32) for k in ("score", "anchors", "rbeg", "rend", "tbeg", "tend")])
ANCHOR_DTYPE = np.dtype([(k, np.uint32) for k in ("rstart", "tpos", "len")])
SEED_DTYPE = np.dtype([(k, np.uint32) for k in ("start", "len", "sa_beg", "sa_end")])


def chain_params(**params):
    """kiss_hip_chain_params from keywords; the defaults are CHAIN_DEFAULTS"""
    p = dict(CHAIN_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown chain parameter %r (known: %s)" % (k, ", ".join(sorted(p))))
        p[k] = int(v)
    if min(p.values()) < 0 or max(p.values()) > 0xFFFFFFFF:
        raise ValueError("the chain parameters are u32")
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

    d_chains = torch.zeros((1, 6), dtype=torch.int32, device=dev)
    rc = call(d_chains, 0, None, None, 0)
    d_anc = d_aidx = None
    if rc == _lib.KISS_HIP_E_INVALID and rep.chains:  # the totals are in the report
        n, m = int(rep.chains), int(rep.chain_anchors)
        d_chains = torch.zeros((n, 6), dtype=torch.int32, device=dev)
        if want_anchors:
            d_anc = torch.zeros((max(m, 1), 3), dtype=torch.int32, device=dev)
            d_aidx = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rc = call(d_chains, n, d_anc, d_aidx, m if want_anchors else 0)
    elif rc == _lib.KISS_HIP_OK and want_anchors:  # no chains at all
        d_anc = torch.zeros((1, 3), dtype=torch.int32, device=dev)
        d_aidx = torch.zeros(1, dtype=torch.int64, device=dev)
    _raise(rc, rep, "kiss_hip_fmi_chain_dev", ctx._ctx)
    return {"d_chains": d_chains, "d_cidx": d_cidx, "d_anc": d_anc, "d_aidx": d_aidx, "rep": rep}


def chain_arrays(out, want_anchors):
    """the tensors of chain_dev as numpy"""
    rep = out["rep"]
    n, m = int(rep.chains), int(rep.chain_anchors)
    res = {"chains": np.ascontiguousarray(out["d_chains"][:n].cpu().numpy()).view(np.uint32).reshape(n, 6).view(CHAIN_DTYPE).reshape(n),
           "chain_index": out["d_cidx"].cpu().numpy().view(np.uint64)}
    if want_anchors:
        res["anchors"] = np.ascontiguousarray(out["d_anc"][:m].cpu().numpy()).view(np.uint32).reshape(m, 3).view(ANCHOR_DTYPE).reshape(m)
        res["anchor_index"] = out["d_aidx"].cpu().numpy().view(np.uint64)
    res["report"] = rep.as_dict()
    return res


def chain_seeds(seeds, seed_index, positions, pos_index, want_anchors=True, device=0, hooks=None, **params):
    """Chain anchors given as the arrays of the seeds call (numpy in, numpy out): seeds is its structured array (start, len,
    sa_beg, sa_end) or an (n, 2) array of (start, len); seed_index has V + 1 entries, pos_index seeds + 1; params as in
    FMIndex.chains.  Returns dict(chains, chain_index, report) and, with want_anchors, anchors / anchor_index."""
    p = chain_params(**params)
    seeds = np.asarray(seeds)
    if seeds.dtype.names:
        sd = np.zeros(seeds.shape[0], SEED_DTYPE)
        sd["start"], sd["len"] = seeds["start"], seeds["len"]
    else:
        pairs = np.asarray(seeds, np.int64).reshape(-1, 2)
        if pairs.size and (pairs.min() < 0 or pairs.max() > 0xFFFFFFFF):
            raise ValueError("start and len are u32")
        sd = np.zeros(pairs.shape[0], SEED_DTYPE)
        sd["start"], sd["len"] = pairs[:, 0], pairs[:, 1]
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
    if sd.size == 0:
        sd = np.zeros(1, SEED_DTYPE)  # (a pointer that is not NULL)
    if pos.size == 0:
        pos = np.zeros(1, np.uint32)

    def call(chains, ccap, anc, aidx, acap):
        return lib.kiss_hip_fmi_chain_host(sd.ctypes.data, sidx.ctypes.data, V, pos.ctypes.data, pidx.ctypes.data, ctypes.byref(p),
                                           chains.ctypes.data, cidx.ctypes.data, ccap, anc.ctypes.data if anc is not None else None,
                                           aidx.ctypes.data if aidx is not None else None, acap, ctypes.byref(rep), int(device))

    chains = np.zeros(1, CHAIN_DTYPE)
    anc = aidx = None
    rc = call(chains, 0, None, None, 0)
    if rc == _lib.KISS_HIP_E_INVALID and rep.chains:  # the totals are in the report
        n, m = int(rep.chains), int(rep.chain_anchors)
        chains = np.zeros(n, CHAIN_DTYPE)
        if want_anchors:
            anc, aidx = np.zeros(max(m, 1), ANCHOR_DTYPE), np.zeros(n + 1, np.uint64)
        rc = call(chains, n, anc, aidx, m if want_anchors else 0)
    _raise(rc, rep, "kiss_hip_fmi_chain_host")
    n, m = int(rep.chains), int(rep.chain_anchors)
    res = {"chains": chains[:n], "chain_index": cidx}
    if want_anchors:
        res["anchors"] = anc[:m] if anc is not None else np.zeros(0, ANCHOR_DTYPE)
        res["anchor_index"] = aidx if aidx is not None else np.zeros(1, np.uint64)
    res["report"] = rep.as_dict()
    return res
