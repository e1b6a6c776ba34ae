"""Banded affine-gap local alignment of chains to the text (kiss_hip_fmi_align_dev / _host; include/kiss_hip.h has the
definition).

align_chains() takes numpy arrays -- chain records from anywhere -- and runs the host entry; FMIndex.align() keeps the
reads and the output of the chain call on the device and runs the device entry (align_dev).  All arithmetic runs in
libkiss_hip.so; there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, make_params, read_batch, record_dtype, record_view, records, sized
from .fm_chain import CHAIN_DTYPE
from .sorter import _check

ALIGN_DEFAULTS = dict(match=1, mismatch=4, gap_open=6, gap_extend=1, band=32)
ALIGN_MAX_BAND = 1024  # KISS_HIP_ALIGN_MAX_BAND
ALIGN_CELLS_PER_N = 16  # KISS_HIP_ALIGN_CELLS_PER_N
ALN_BAND_TOO_WIDE = 1
ALN_DTYPE = record_dtype(_lib.Aln)
ALN_FIELDS = ALN_DTYPE.names
CIGAR_OPS = "MID"


def align_params(**params):
    """kiss_hip_align_params from keywords; the defaults are ALIGN_DEFAULTS"""
    p = make_params("align", ALIGN_DEFAULTS, params)
    if p["match"] < 1 or max(p["match"], p["mismatch"], p["gap_open"], p["gap_extend"]) > 65535 or p["band"] > 0x7FFFFFFF:
        raise ValueError("match is at least 1, the four scores at most 65535, band at most 2^31 - 1")
    return _lib.AlignParams(**p)


def cigar_string(ops):
    """u32 ops (len << 4 | op) -> '20M2D26M'"""
    return "".join("%d%s" % (int(o) >> 4, CIGAR_OPS[int(o) & 15]) for o in ops)


def _raise(rc, rep, where, ctx=None):
    if rc == _lib.KISS_HIP_E_UNSUPPORTED and rep.cells:
        raise _lib.KissHipError(rc, where, "%d DP cells are more than the traceback store of one call holds (%d per base of the "
                                "context's max_n): split the batch" % (rep.cells, ALIGN_CELLS_PER_N))
    _check(rc, where, ctx)


def align_dev(lib, ctx, device, d_text, n, d_reads, d_ridx, Q, both_strands, d_chains, d_cidx, C, params, want_cigar):
    """the device entry on torch tensors -> dict of torch tensors and the report; two calls when the ops are wanted, the
    first one sizes them (the C interface's convention)"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.AlignReport()
    d_alns = torch.zeros((max(C, 1), 12), dtype=torch.int32, device=dev)

    def call(d_cig, d_oidx, ocap):
        return lib.kiss_hip_fmi_align_dev(ctx._ctx, vp(d_text.data_ptr()), n, vp(d_reads.data_ptr()), vp(d_ridx.data_ptr()), Q,
                                          1 if both_strands else 0, vp(d_chains.data_ptr()), vp(d_cidx.data_ptr()),
                                          ctypes.byref(params), vp(d_alns.data_ptr()), C,
                                          vp(d_cig.data_ptr()) if d_cig is not None else None,
                                          vp(d_oidx.data_ptr()) if d_oidx is not None else None, ocap, ctypes.byref(rep), None)

    d_cig = d_oidx = None
    if want_cigar:
        d_oidx = torch.zeros(C + 1, dtype=torch.int64, device=dev)
        rc, (d_cig, _, _) = sized(call, lambda m=0: (torch.zeros(max(m, 1), dtype=torch.int32, device=dev), d_oidx, m), rep, "cigar_ops")
    else:
        rc = call(None, None, 0)
    _raise(rc, rep, "kiss_hip_fmi_align_dev", ctx._ctx)
    return {"d_alns": d_alns, "d_cigar": d_cig, "d_oidx": d_oidx, "rep": rep, "C": C}


def align_arrays(out, want_cigar):
    """the tensors of align_dev as numpy"""
    rep, C = out["rep"], out["C"]
    res = {"alignments": record_view(out["d_alns"], C, ALN_DTYPE)}
    if want_cigar:
        m = int(rep.cigar_ops)
        res["cigar"] = out["d_cigar"][:m].cpu().numpy().view(np.uint32)
        res["cigar_index"] = out["d_oidx"].cpu().numpy().view(np.uint64)
    res["align_report"] = rep.as_dict()
    return res


def align_chains(text, reads, chains, chain_index, both_strands=False, want_cigar=True, device=0, hooks=None, **params):
    """Align chains given as arrays (numpy in, numpy out).  text: uint8 bases 0..3; reads: a list of uint8 arrays, or
    (concatenated, index); chains: the structured array of the chain call, or an (n, 4) array of (rbeg, rend, tbeg, tend) --
    the only fields the band is made of; chain_index has V + 1 entries; params: match (1), mismatch (4), gap_open (6),
    gap_extend (1), band (32).  Returns dict(alignments: structured array of the fields of kiss_hip_aln, report) and, with
    want_cigar, cigar (u32 ops len << 4 | op, op 0 M, 1 I, 2 D) / cigar_index in CSR layout over the chains."""
    p = align_params(**params)
    text = np.ascontiguousarray(text, dtype=np.uint8).ravel()
    cat, ridx = read_batch(reads)
    ch = records(chains, CHAIN_DTYPE, "rbeg, rend, tbeg and tend are u32", columns=("rbeg", "rend", "tbeg", "tend"), structured=CHAIN_DTYPE.names)
    cidx = np.ascontiguousarray(chain_index, dtype=np.uint64)
    if ridx.ndim != 1 or ridx.size < 1 or cidx.ndim != 1:
        raise ValueError("the read index has Q + 1 entries, chain_index V + 1")
    Q = ridx.size - 1
    V = 2 * Q if both_strands else Q
    if cidx.size != V + 1:
        raise ValueError("chain_index has V + 1 = %d entries" % (V + 1))
    if int(ridx.max()) > cat.size or int(cidx.max()) > ch.size:
        raise ValueError("the read index points past the reads, or chain_index past the chains")
    lib = _lib.load(hooks)
    rep = _lib.AlignReport()
    C = int(cidx[-1]) - int(cidx[0]) if int(cidx[-1]) >= int(cidx[0]) else 0
    alns = np.zeros(max(C, 1), ALN_DTYPE)
    oidx = np.zeros(C + 1, np.uint64)
    (tp, rp, cp), hold = addresses(text, cat, ch)

    def call(cig, ocap):
        return lib.kiss_hip_fmi_align_host(tp, text.size, rp, ridx.ctypes.data, Q, 1 if both_strands else 0, cp, cidx.ctypes.data,
                                           ctypes.byref(p), alns.ctypes.data, C, cig.ctypes.data if cig is not None else None,
                                           oidx.ctypes.data if cig is not None else None, ocap, ctypes.byref(rep), int(device))

    cig = None
    if want_cigar:
        rc, (cig, _) = sized(call, lambda m=0: (np.zeros(max(m, 1), np.uint32), m), rep, "cigar_ops")
    else:
        rc = call(None, 0)
    _raise(rc, rep, "kiss_hip_fmi_align_host")
    res = {"alignments": alns[:C]}
    if want_cigar:
        res["cigar"] = cig[:int(rep.cigar_ops)]
        res["cigar_index"] = oidx
    res["report"] = rep.as_dict()
    return res
