"""The alignments of a read turned into its mappings: primary, secondary, supplementary, MAPQ (kiss_hip_fmi_select_dev /
_host; include/kiss_hip.h has the definition).

select_alignments() takes numpy arrays -- alignment records from anywhere -- and runs the host entry; FMIndex.map() keeps
the output of the align call on the device and runs the device entry (select_dev).  All arithmetic runs in libkiss_hip.so;
there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, make_params, read_index, record_dtype, record_view, records
from .fm_align import ALN_DTYPE
from .sorter import _check

SELECT_DEFAULTS = dict(min_score=30, overlap=128, mapq_coef=120, mapq_max=60, max_hits=0)
SELECT_LIMITS = dict(overlap=256, mapq_coef=65535, mapq_max=255)
HIT_REVERSE, HIT_SECONDARY, HIT_SUPPLEMENTARY = 1, 2, 4
HIT_DTYPE = record_dtype(_lib.Hit)
HIT_FIELDS = HIT_DTYPE.names


def select_params(**params):
    """kiss_hip_select_params from keywords; the defaults are SELECT_DEFAULTS"""
    return _lib.SelectParams(**make_params("select", SELECT_DEFAULTS, params, SELECT_LIMITS))


def _bounds_array(bounds):
    """None, or the R + 1 record starts as u64 (checked here so that the message names the fault)"""
    if bounds is None:
        return None
    b = np.ascontiguousarray(bounds, dtype=np.uint64).ravel()
    if b.size < 2 or int(b[0]) != 0 or np.any(b[1:] <= b[:-1]):
        raise ValueError("bounds has R + 1 >= 2 strictly ascending entries and starts at 0")
    return b


def select_dev(lib, ctx, device, d_alns, d_cidx, d_ridx, Q, C, both_strands, bounds, params):
    """the device entry on torch tensors -> dict of torch tensors and the report.  One call: a read keeps no more hits than
    it has alignments, so room for C hits always suffices and nothing is sized by a first pass"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.SelectReport()
    b = _bounds_array(bounds)
    d_bounds = torch.from_numpy(b.view(np.int64)).to(dev) if b is not None else None
    R = b.size - 1 if b is not None else 0
    d_hidx = torch.zeros(Q + 1, dtype=torch.int64, device=dev)

    def call(d_hits, cap):
        return lib.kiss_hip_fmi_select_dev(ctx._ctx, vp(d_alns.data_ptr()), vp(d_cidx.data_ptr()), vp(d_ridx.data_ptr()), Q,
                                           1 if both_strands else 0, vp(d_bounds.data_ptr()) if d_bounds is not None else None, R,
                                           ctypes.byref(params), vp(d_hits.data_ptr()), vp(d_hidx.data_ptr()), cap,
                                           ctypes.byref(rep), None)

    d_hits = torch.zeros((max(C, 1), 8), dtype=torch.int32, device=dev)
    _check(call(d_hits, C), "kiss_hip_fmi_select_dev", ctx._ctx)
    return {"d_hits": d_hits, "d_hidx": d_hidx, "rep": rep}


def select_arrays(out):
    """the tensors of select_dev as numpy"""
    return {"hits": record_view(out["d_hits"], int(out["rep"].hits), HIT_DTYPE),
            "hit_index": out["d_hidx"].cpu().numpy().view(np.uint64), "select_report": out["rep"].as_dict()}


def select_alignments(alignments, chain_index, read_lengths_or_index, both_strands=False, bounds=None, device=0, hooks=None,
                      **params):
    """Select the mappings of reads from alignment records given as arrays (numpy in, numpy out).  alignments: the structured
    array of the align call, or a (C, 12) integer array in the order of its fields; alignment a belongs to the virtual read
    that contains chain_index[0] + a (chain_index has V + 1 entries); read_lengths_or_index: the Q read lengths, or the tuple
    ("index", array of Q + 1 ascending offsets) as the other calls take it (only the differences are used); bounds: the R + 1
    record starts of the text, None: one record; params: min_score (30), overlap (128, in 256ths), mapq_coef (120), mapq_max
    (60), max_hits (0: all).  Returns dict(hits: structured array of the fields of kiss_hip_hit, hit_index: Q + 1 u64 over
    the reads, report)."""
    p = select_params(**params)
    al = records(alignments, ALN_DTYPE, "the fields of an alignment record are u32")
    ridx = read_index(read_lengths_or_index)
    cidx = np.ascontiguousarray(chain_index, dtype=np.uint64).ravel()
    if ridx.size < 1:
        raise ValueError("the read index has Q + 1 entries")
    Q = ridx.size - 1
    V = 2 * Q if both_strands else Q
    if cidx.size != V + 1:
        raise ValueError("chain_index has V + 1 = %d entries" % (V + 1))
    C = int(cidx[-1]) - int(cidx[0]) if int(cidx[-1]) >= int(cidx[0]) else 0
    if C > al.size:
        raise ValueError("chain_index spans %d alignments, %d given" % (C, al.size))
    b = _bounds_array(bounds)
    lib = _lib.load(hooks)
    rep = _lib.SelectReport()
    hidx = np.zeros(Q + 1, np.uint64)
    (ap,), hold = addresses(al)

    def call(hits, cap):
        return lib.kiss_hip_fmi_select_host(ap, cidx.ctypes.data, ridx.ctypes.data, Q, 1 if both_strands else 0,
                                            b.ctypes.data if b is not None else None, b.size - 1 if b is not None else 0,
                                            ctypes.byref(p), hits.ctypes.data, hidx.ctypes.data, cap, ctypes.byref(rep), int(device))

    hits = np.zeros(max(C, 1), HIT_DTYPE)  # (no more hits than alignments: one call, nothing sized by a first pass)
    _check(call(hits, C), "kiss_hip_fmi_select_host")
    return {"hits": hits[:int(rep.hits)], "hit_index": hidx, "report": rep.as_dict()}
