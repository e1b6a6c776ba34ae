"""The mappings of two mates paired: proper pairs, pair MAPQ, TLEN (kiss_hip_fmi_pair_dev / _host; include/kiss_hip.h has
the definition).  Reads 2 p and 2 p + 1 of the batch are mate 1 and mate 2 of pair p.

pair_hits() takes numpy arrays -- hits and alignment records from anywhere -- and runs the host entry; FMIndex.map_pairs()
keeps the output of the select call on the device and runs the device entry (pair_dev).  All arithmetic runs in
libkiss_hip.so; there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, check_mates, make_params, record_dtype, record_view, records
from .fm_align import ALN_DTYPE
from .fm_select import HIT_DTYPE
from .sorter import _check

PAIR_DEFAULTS = dict(ins_min=0, ins_max=1000, ins_mean=400, pen_coef=8, pen_max=20, mapq_coef=120, mapq_max=60)
PAIR_LIMITS = dict(pen_coef=65535, pen_max=65535, mapq_coef=65535, mapq_max=255)
PAIR_NONE = 0xFFFFFFFF
PAIR_PROPER, PAIR_MATE1_MAPPED, PAIR_MATE2_MAPPED, PAIR_SAME_REF, PAIR_PROMOTED1, PAIR_PROMOTED2, PAIR_BAD_INPUT = 1, 2, 4, 8, 16, 32, 64
PAIR_DTYPE = record_dtype(_lib.Pair)
PAIR_FIELDS = PAIR_DTYPE.names


def pair_params(**params):
    """kiss_hip_pair_params from keywords; the defaults are PAIR_DEFAULTS"""
    p = make_params("pair", PAIR_DEFAULTS, params, PAIR_LIMITS)
    if p["ins_min"] > p["ins_max"]:
        raise ValueError("ins_min is at most ins_max")
    return _lib.PairParams(**p)


def pair_dev(lib, ctx, device, d_hits, d_hidx, Q, d_alns, aln_count, params):
    """the device entry on torch tensors -> dict of the pairs tensor (P x 10) and the report"""
    import torch
    check_mates(Q)
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
    return {"pairs": record_view(out["d_pairs"], int(out["rep"].P), PAIR_DTYPE), "pair_report": out["rep"].as_dict()}


def _records(rows, dtype, what):
    """records() under the name and with the arguments it had here (tests/test_fm_rescue_gpu.py reaches it as fm_rescue._records)"""
    return records(rows, dtype, "the fields of %s are u32" % what)


def _mates_of(hits, hit_index, alignments):
    """what pair_hits() and estimate_insert() take, checked -> the hits and alignment records, the hit index, Q"""
    ht = records(hits, HIT_DTYPE, "the fields of a hit are u32")
    al = records(alignments, ALN_DTYPE, "the fields of an alignment record are u32")
    hidx = np.ascontiguousarray(hit_index, dtype=np.uint64).ravel()
    if hidx.size < 1:
        raise ValueError("hit_index has Q + 1 entries")
    Q = hidx.size - 1
    check_mates(Q)
    if np.all(hidx[1:] >= hidx[:-1]) and int(hidx[-1]) > ht.size:
        raise ValueError("hit_index spans %d hits, %d given" % (int(hidx[-1]), ht.size))
    return ht, al, hidx, Q


def pair_hits(hits, hit_index, alignments, device=0, hooks=None, **params):
    """Pair the hits of mates given as arrays (numpy in, numpy out).  hits: the structured array of the select call, or an
    (H, 8) integer array in the order of its fields; hit_index: Q + 1 ascending offsets over the reads, Q even, reads 2 p and
    2 p + 1 the mates of pair p; alignments: the records a hit's aln field indexes (structured, or (C, 12) integers; only
    tbeg and tend are read); params: ins_min (0), ins_max (1000), ins_mean (400), pen_coef (8, in 256ths), pen_max (20),
    mapq_coef (120), mapq_max (60).  Returns dict(pairs: structured array of the fields of kiss_hip_pair, one per pair,
    report)."""
    p = pair_params(**params)
    ht, al, hidx, Q = _mates_of(hits, hit_index, alignments)
    lib = _lib.load(hooks)
    rep = _lib.PairReport()
    pairs = np.zeros(max(Q // 2, 1), PAIR_DTYPE)
    (hp, ap), hold = addresses(ht, al)
    _check(lib.kiss_hip_fmi_pair_host(hp, hidx.ctypes.data, Q, ap, al.size, ctypes.byref(p), pairs.ctypes.data,
                                      ctypes.byref(rep), int(device)), "kiss_hip_fmi_pair_host")
    return {"pairs": pairs[:Q // 2], "report": rep.as_dict()}
