"""The insert size of a paired library, estimated from the pairs on the device (kiss_hip_fmi_insert_dev / _host;
include/kiss_hip_insert.h has the definition).  Reads 2 p and 2 p + 1 of the batch are mate 1 and mate 2 of pair p; only the
first hit of either mate is looked at.

estimate_insert() takes numpy arrays -- hits and alignment records from anywhere -- and runs the host entry;
FMIndex.map_pairs(insert=...) keeps the output of the select call on the device and runs the device entry (insert_dev) between
the select and the pair call.  All arithmetic runs in libkiss_hip.so; there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, check_mates, make_params
from .fm_pair import _mates_of
from .sorter import _check

INSERT_DEFAULTS = dict(min_mapq=20, max_insert=10000, min_samples=25, out_mult=2, map_mult=3, sd_mult=4)
INSERT_LIMITS = dict(max_insert=_lib.INSERT_MAX, out_mult=255, map_mult=255, sd_mult=255)
INSERT_OK = _lib.INSERT_OK
INSERT_STATS = ("samples", "used", "q25", "q50", "q75", "mean", "sd", "ins_min", "ins_max", "ins_mean")


def insert_params(**params):
    """kiss_hip_insert_params from keywords; the defaults are INSERT_DEFAULTS"""
    p = make_params("insert", INSERT_DEFAULTS, params, INSERT_LIMITS)
    if p["max_insert"] < 1:
        raise ValueError("max_insert is at least 1")
    return _lib.InsertParams(**p)


def insert_dev(lib, ctx, device, d_hits, d_hidx, Q, d_alns, aln_count, params, want_hist=True):
    """the device entry on torch tensors -> dict of the histogram tensor (max_insert + 1; None without want_hist: it then
    lives in the context's scratch) and the report"""
    import torch
    check_mates(Q)
    vp = ctypes.c_void_p
    rep = _lib.InsertReport()
    d_hist = torch.zeros(params.max_insert + 1, dtype=torch.int32, device=torch.device("cuda", device)) if want_hist else None
    _check(lib.kiss_hip_fmi_insert_dev(ctx._ctx, vp(d_hits.data_ptr()), vp(d_hidx.data_ptr()), Q, vp(d_alns.data_ptr()), aln_count,
                                       ctypes.byref(params), vp(d_hist.data_ptr()) if want_hist else None, ctypes.byref(rep), None),
           "kiss_hip_fmi_insert_dev", ctx._ctx)
    return {"d_hist": d_hist, "rep": rep}


def insert_arrays(out):
    """the outputs of insert_dev as numpy: dict(stats, hist, report)"""
    rep = out["rep"].as_dict()
    hist = None if out["d_hist"] is None else np.ascontiguousarray(out["d_hist"].cpu().numpy()).view(np.uint32)
    return {"stats": {k: rep[k] for k in INSERT_STATS}, "hist": hist, "report": rep}


def estimate_insert(hits, hit_index, alignments, device=0, hooks=None, **params):
    """Estimate the insert size from the hits of mates given as arrays (numpy in, numpy out).  hits, hit_index and alignments as
    in pair_hits(); params: min_mapq (20), max_insert (10000, at most 65535), min_samples (25), out_mult (2), map_mult (3),
    sd_mult (4).  Returns dict(stats: samples, used, q25, q50, q75, mean, sd, ins_min, ins_max, ins_mean -- all 0 but samples
    unless report["flags"] has INSERT_OK --, hist: max_insert + 1 counts of the samples by insert, report: every field of
    kiss_hip_insert_report)."""
    p = insert_params(**params)
    ht, al, hidx, Q = _mates_of(hits, hit_index, alignments)
    lib = _lib.load(hooks)
    rep = _lib.InsertReport()
    hist = np.zeros(p.max_insert + 1, np.uint32)
    (hp, ap), hold = addresses(ht, al)
    _check(lib.kiss_hip_fmi_insert_host(hp, hidx.ctypes.data, Q, ap, al.size, ctypes.byref(p), hist.ctypes.data,
                                        ctypes.byref(rep), int(device)), "kiss_hip_fmi_insert_host")
    r = rep.as_dict()
    return {"stats": {k: r[k] for k in INSERT_STATS}, "hist": hist, "report": r}
