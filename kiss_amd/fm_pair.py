"""The mappings of two mates paired: proper pairs, pair MAPQ, TLEN (kiss_hip_fmi_pair_dev / _host; include/kiss_hip.h has
the definition).  Reads 2 p and 2 p + 1 of the batch are mate 1 and mate 2 of pair p.

pair_hits() takes numpy arrays -- hits and alignment records from anywhere -- and runs the host entry; FMIndex.map_pairs()
keeps the output of the select call on the device and runs the device entry (pair_dev).  All arithmetic runs in
libkiss_hip.so; there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from .fm_align import ALN_DTYPE
from .fm_select import HIT_DTYPE
from .sorter import _check

PAIR_DEFAULTS = dict(ins_min=0, ins_max=1000, ins_mean=400, pen_coef=8, pen_max=20, mapq_coef=120, mapq_max=60)
PAIR_LIMITS = dict(pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255)
PAIR_NONE = 0xFFFFFFFF
PAIR_PROPER, PAIR_MATE1_MAPPED, PAIR_MATE2_MAPPED, PAIR_SAME_REF, PAIR_PROMOTED1, PAIR_PROMOTED2, PAIR_BAD_INPUT = 1, 2, 4, 8, 16, 32, 64
PAIR_FIELDS = ("hit1", "hit2", "flags", "tlen", "score", "sub1", "sub2", "mapq1", "mapq2", "n_conc")
PAIR_DTYPE = np.dtype([(k, np.uint32) for k in PAIR_FIELDS])


def pair_params(**params):
    """kiss_hip_pair_params from keywords; the defaults are PAIR_DEFAULTS"""
    p = dict(PAIR_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown pair parameter %r (known: %s)" % (k, ", ".join(sorted(p))))
        p[k] = int(v)
    if min(p.values()) < 0 or max(p.values()) > 0xFFFFFFFF:
        raise ValueError("the pair parameters are u32")
    for k, top in PAIR_LIMITS.items():
        if p[k] > top:
            raise ValueError("%s is at most %d" % (k, top))
    if p["ins_min"] > p["ins_max"]:
        raise ValueError("ins_min is at most ins_max")
    return _lib.PairParams(**p)


def pair_dev(lib, ctx, device, d_hits, d_hidx, Q, d_alns, aln_count, params):
    """the device entry on torch tensors -> dict of the pairs tensor (P x 10) and the report"""
    import torch
    if Q % 2:
        raise ValueError("a batch of pairs has an even number of reads (2 p and 2 p + 1 are the mates of pair p), not %d" % Q)
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.PairReport()
    d_pairs = torch.zeros((max(Q // 2, 1), 10), dtype=torch.int32, device=dev)
    _check(lib.kiss_hip_fmi_pair_dev(ctx._ctx, vp(d_hits.data_ptr()), vp(d_hidx.data_ptr()), Q, vp(d_alns.data_ptr()), aln_count,
                                     ctypes.byref(params), vp(d_pairs.data_ptr()), ctypes.byref(rep), None),
           "kiss_hip_fmi_pair_dev", ctx._ctx)
    return {"d_pairs": d_pairs, "rep": rep}


def pair_arrays(out):
    """the tensors of pair_dev as numpy"""
    n = int(out["rep"].P)
    raw = np.ascontiguousarray(out["d_pairs"][:n].cpu().numpy()).view(np.uint32).reshape(n, 10)
    return {"pairs": raw.view(PAIR_DTYPE).reshape(n), "pair_report": out["rep"].as_dict()}


def _records(rows, dtype, what):
    """a structured array with the fields of dtype, or an (n, fields) integer array in their order -> dtype array"""
    arr = np.asarray(rows)
    width = len(dtype.names)
    if arr.dtype.names:
        out = np.zeros(arr.shape[0], dtype)
        for k in dtype.names:
            out[k] = arr[k]
        return out
    ints = np.asarray(arr, np.int64).reshape(-1, width)
    if ints.size and (ints.min() < 0 or ints.max() > 0xFFFFFFFF):
        raise ValueError("the fields of %s are u32" % what)
    return np.ascontiguousarray(ints.astype(np.uint32)).view(dtype).reshape(ints.shape[0])


def pair_hits(hits, hit_index, alignments, device=0, hooks=None, **params):
    """Pair the hits of mates given as arrays (numpy in, numpy out).  hits: the structured array of the select call, or an
    (H, 8) integer array in the order of its fields; hit_index: Q + 1 ascending offsets over the reads, Q even, reads 2 p and
    2 p + 1 the mates of pair p; alignments: the records a hit's aln field indexes (structured, or (C, 12) integers; only
    tbeg and tend are read); params: ins_min (0), ins_max (1000), ins_mean (400), pen_coef (8, in 256ths), pen_max (20),
    mapq_coef (120), mapq_max (60).  Returns dict(pairs: structured array of the fields of kiss_hip_pair, one per pair,
    report)."""
    p = pair_params(**params)
    ht = _records(hits, HIT_DTYPE, "a hit")
    al = _records(alignments, ALN_DTYPE, "an alignment record")
    hidx = np.ascontiguousarray(hit_index, dtype=np.uint64).ravel()
    if hidx.size < 1:
        raise ValueError("hit_index has Q + 1 entries")
    Q = hidx.size - 1
    if Q % 2:
        raise ValueError("a batch of pairs has an even number of reads (2 p and 2 p + 1 are the mates of pair p), not %d" % Q)
    if np.all(hidx[1:] >= hidx[:-1]) and int(hidx[-1]) > ht.size:
        raise ValueError("hit_index spans %d hits, %d given" % (int(hidx[-1]), ht.size))
    lib = _lib.load(hooks)
    rep = _lib.PairReport()
    pairs = np.zeros(max(Q // 2, 1), PAIR_DTYPE)
    keep_h, keep_a = np.zeros(1, HIT_DTYPE), np.zeros(1, ALN_DTYPE)  # (pointers that are not NULL)
    _check(lib.kiss_hip_fmi_pair_host(ht.ctypes.data if ht.size else keep_h.ctypes.data, hidx.ctypes.data, Q,
                                      al.ctypes.data if al.size else keep_a.ctypes.data, al.size, ctypes.byref(p), pairs.ctypes.data,
                                      ctypes.byref(rep), int(device)), "kiss_hip_fmi_pair_host")
    return {"pairs": pairs[:Q // 2], "report": rep.as_dict()}
