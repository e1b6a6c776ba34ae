"""Per-position pileup counts of the mappings, accumulated on the device (kiss_hip_fmi_pileup_dev / _host;
include/kiss_hip_pileup.h has the definition).

pileup() takes numpy arrays -- records and ops from anywhere -- and runs the host entry; FMIndex.map(pileup=...),
FMIndex.map_pairs(pileup=...) and batches.map_file(pileup=...) keep everything on the device and run the device entry
(pileup_dev), which adds onto a tensor the caller may keep from call to call.  All arithmetic runs in libkiss_hip.so; there
is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, make_params, read_batch, records
from .fm_align import ALN_DTYPE
from .fm_pair import PAIR_DTYPE
from .fm_select import HIT_DTYPE, HIT_REVERSE, HIT_SECONDARY, HIT_SUPPLEMENTARY
from .sorter import _check

PLANES = ("cov", "alt_a", "alt_c", "alt_g", "alt_t", "alt_n", "del", "ins")
COV, ALT_A, ALT_C, ALT_G, ALT_T, ALT_N, DEL, INS = range(8)
PILEUP_DEFAULTS = dict(min_mapq=0, skip_flags=HIT_SECONDARY, proper_only=0)
PILEUP_LIMITS = dict(min_mapq=255, skip_flags=HIT_REVERSE | HIT_SECONDARY | HIT_SUPPLEMENTARY)
REPORT_COUNTS = ("items", "bad", "filtered", "unmapped", "counted", "columns", "alt_columns", "deleted_bases", "insertions", "clipped")
# the keys of FMIndex.map(pileup=dict(...)) that are not parameters of the filter
WINDOW_KEYS = ("lo", "hi", "counts")


def pileup_params(**kw):
    """keywords -> kiss_hip_pileup_params; an unknown key is a TypeError, a value past its limit a ValueError"""
    p = make_params("pileup", PILEUP_DEFAULTS, kw, PILEUP_LIMITS)  # (skip_flags: REVERSE 1 | SECONDARY 2 | SUPPLEMENTARY 4)
    return _lib.PileupParams(p["min_mapq"], p["skip_flags"], 1 if p["proper_only"] else 0, 0)


def window(n, lo=0, hi=None):
    """-> lo, hi (hi None: the end of the text)"""
    lo, hi = int(lo), int(n) if hi is None else int(hi)
    if not 0 <= lo <= hi <= int(n):
        raise ValueError("the window is lo <= hi <= n = %d, not [%d, %d)" % (n, lo, hi))
    return lo, hi


def base_counts(counts, text_window):
    """the planes of a window and its text -> (5, W) u32: the A, C, G, T and no-base read bases per position, those equal to the
    text included (they number COV minus the five ALT planes; a text byte above 3 equals no base)"""
    c = np.asarray(counts, np.uint32).reshape(8, -1)
    t = np.asarray(text_window, np.uint8).ravel()
    if t.size != c.shape[1]:
        raise ValueError("the text of the window has W = %d bases" % c.shape[1])
    out = c[ALT_A:ALT_N + 1].copy()
    same = c[COV] - c[ALT_A:ALT_N + 1].sum(axis=0, dtype=np.uint32)
    at = np.flatnonzero(t <= 3)
    out[t[at], at] += same[at]
    return out


def pileup_dev(lib, ctx, device, d_text, n, d_reads, d_ridx, Q, both_strands, d_alns, d_cidx, d_cigar, d_oidx, d_hits=None, H=0,
               d_pairs=None, P=0, lo=0, hi=None, d_counts=None, stream=None, **params):
    """the device entry on torch tensors -> dict(d_counts: (8, W) int32 tensor holding the u32 planes, rep).  d_counts given: the
    call adds onto it (accumulate), else a new tensor is zeroed by the call.  d_pairs: pair mode (needs d_hits); d_hits alone:
    hits mode; neither: one item per alignment.  stream: None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    par = pileup_params(**params)
    lo, hi = window(n, lo, hi)
    W = hi - lo
    accumulate = d_counts is not None
    if accumulate:
        if d_counts.dtype != torch.int32 or tuple(d_counts.shape) != (8, W) or not d_counts.is_contiguous() or d_counts.device != dev:
            raise ValueError("counts is a contiguous (8, %d) int32 tensor on %s" % (W, dev))
    else:
        d_counts = torch.empty((8, W), dtype=torch.int32, device=dev)
    if d_pairs is not None and d_hits is None:
        raise ValueError("pairs need the hits they index")
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rep = _lib.PileupReport()
    rc = lib.kiss_hip_fmi_pileup_dev(ctx._ctx, vp(d_text.data_ptr()), n, vp(d_reads.data_ptr()), vp(d_ridx.data_ptr()), Q,
                                     1 if both_strands else 0, vp(d_alns.data_ptr()), vp(d_cidx.data_ptr()), vp(d_cigar.data_ptr()),
                                     vp(d_oidx.data_ptr()), vp(d_hits.data_ptr()) if d_hits is not None else None,
                                     int(H) if d_hits is not None else 0, vp(d_pairs.data_ptr()) if d_pairs is not None else None,
                                     int(P) if d_pairs is not None else 0, ctypes.byref(par), lo, hi, vp(d_counts.data_ptr()) if W else None,
                                     1 if accumulate else 0, ctypes.byref(rep), vp(stream) if stream else None)
    _check(rc, "kiss_hip_fmi_pileup_dev", ctx._ctx)
    return {"d_counts": d_counts, "rep": rep}


def planes_of(d_counts):
    """the tensor of pileup_dev as numpy: (8, W) u32"""
    return np.ascontiguousarray(d_counts.cpu().numpy()).view(np.uint32)


def add_reports(total, rep):
    """the counts and times of one more call added to a dict (map_file: the sums over the batches)"""
    for k, v in rep.items():
        total[k] = total.get(k, 0) + v
    return total


def pileup(text, reads, alignments, chain_index, cigar, cigar_index, both_strands=False, hits=None, pairs=None, lo=0, hi=None,
           counts=None, device=0, hooks=None, **params):
    """The pileup of alignments given as arrays (numpy in, numpy out).  text: uint8 bases 0..3; reads: a list of uint8 arrays, or
    (concatenated, index); alignments: the structured array of the align call, or a (C, 12) integer array in the order of its
    fields; chain_index has V + 1 entries; cigar / cigar_index: the ops (len << 4 | op) in CSR layout over the alignments;
    hits: None (one item per alignment, no filter), the structured array of the select call or an (H, 8) integer array in the
    order of its fields; pairs: None, or the records of the pair call (pair mode; needs hits); lo, hi: the window of text
    positions (hi None: n); counts: an (8, hi - lo) u32 array to add to (it is not changed: the sums are returned), None:
    from zero; params: min_mapq, skip_flags, proper_only.  Returns dict(counts: (8, W) u32 in the order of PLANES, report)."""
    text = np.ascontiguousarray(text, dtype=np.uint8).ravel()
    cat, ridx = read_batch(reads)
    al = records(alignments, ALN_DTYPE, "the fields of an alignment record are u32")
    cidx = np.ascontiguousarray(chain_index, dtype=np.uint64).ravel()
    cig = np.ascontiguousarray(cigar, dtype=np.uint32).ravel()
    oidx = np.ascontiguousarray(cigar_index, dtype=np.uint64).ravel()
    par = pileup_params(**params)
    lo, hi = window(text.size, lo, hi)
    W = hi - lo
    if ridx.ndim != 1 or ridx.size < 1:
        raise ValueError("the read index has Q + 1 entries")
    Q = ridx.size - 1
    V = 2 * Q if both_strands else Q
    if cidx.size != V + 1:
        raise ValueError("chain_index has V + 1 = %d entries" % (V + 1))
    ascending = bool(np.all(cidx[1:] >= cidx[:-1]))
    C = int(cidx[-1]) - int(cidx[0]) if ascending else 0
    if int(ridx.max()) > cat.size or C > al.size:
        raise ValueError("the read index points past the reads, or chain_index spans more alignments than were given")
    if oidx.size < C + 1 or (np.all(oidx[1:C + 1] >= oidx[:C]) and int(oidx[C]) > cig.size):
        raise ValueError("cigar_index has C + 1 entries and points inside the ops")
    ht = None if hits is None else records(hits, HIT_DTYPE, "the fields of a hit are u32")
    pr = None if pairs is None else records(pairs, PAIR_DTYPE, "the fields of a pair are u32")
    if pr is not None and ht is None:
        raise ValueError("pairs need the hits they index")
    accumulate = counts is not None
    if accumulate:
        out = np.array(counts, dtype=np.uint32, order="C", copy=True)
        if out.shape != (8, W):
            raise ValueError("counts has the shape (8, %d)" % W)
    else:
        out = np.zeros((8, W), np.uint32)
    lib = _lib.load(hooks)
    rep = _lib.PileupReport()
    (tp, rp, ap, cp, hp, pp), hold = addresses(text, cat, al, cig, ht, pr)
    rc = lib.kiss_hip_fmi_pileup_host(tp, text.size, rp, ridx.ctypes.data, Q, 1 if both_strands else 0, ap, cidx.ctypes.data, cp,
                                      oidx.ctypes.data, hp, ht.size if ht is not None else 0, pp, pr.size if pr is not None else 0,
                                      ctypes.byref(par), lo, hi, out.ctypes.data if W else None, 0, 1 if accumulate else 0,
                                      ctypes.byref(rep), int(device))
    _check(rc, "kiss_hip_fmi_pileup_host")
    del hold
    return {"counts": out, "report": rep.as_dict()}
