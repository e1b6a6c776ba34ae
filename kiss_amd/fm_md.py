"""The MD:Z strings of alignments, written on the device (kiss_hip_fmi_md_dev / _host; include/kiss_hip_md.h has the
definition).

md_tags() takes numpy arrays -- records and ops from anywhere -- and runs the host entry; FMIndex.map(want_md=True) and
FMIndex.map_pairs(want_md=True) keep everything on the device and run the device entry (md_dev).  All arithmetic runs in
libkiss_hip.so; there is no CPU path.
"""
import ctypes

import numpy as np

from . import _lib
from ._frame import addresses, read_batch, records, sized
from .fm_align import ALN_DTYPE
from .fm_select import HIT_DTYPE
from .sorter import _check


def md_strings(md, md_index):
    """the bytes and their CSR index -> one str per item"""
    raw = np.ascontiguousarray(md, dtype=np.uint8).tobytes()
    idx = [int(x) for x in md_index]
    return [raw[idx[k]:idx[k + 1]].decode("ascii") for k in range(len(idx) - 1)]


def md_dev(lib, ctx, device, d_text, n, d_reads, d_ridx, Q, both_strands, d_alns, d_cidx, C, d_cigar, d_oidx, d_hits=None, H=0,
           stream=None):
    """the device entry on torch tensors -> dict of torch tensors and the report; two calls, the first one sizes the bytes (the C
    interface's convention).  C: the alignments, chain_index[V] - chain_index[0]; d_hits None: one item per alignment.  stream: None, the current stream of torch"""
    import torch
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    rep = _lib.MdReport()
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    with_hits = d_hits is not None
    items = int(H) if with_hits else int(C)
    d_midx = torch.zeros(items + 1, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros((max(items, 1), 2), dtype=torch.int32, device=dev)

    def call(d_md, cap):
        return lib.kiss_hip_fmi_md_dev(ctx._ctx, vp(d_text.data_ptr()), n, vp(d_reads.data_ptr()), vp(d_ridx.data_ptr()), Q,
                                       1 if both_strands else 0, vp(d_alns.data_ptr()), vp(d_cidx.data_ptr()), vp(d_cigar.data_ptr()),
                                       vp(d_oidx.data_ptr()), vp(d_hits.data_ptr()) if with_hits else None, H if with_hits else 0,
                                       vp(d_md.data_ptr()) if d_md is not None else None, vp(d_midx.data_ptr()),
                                       vp(d_cnt.data_ptr()) if d_cnt is not None else None, cap, ctypes.byref(rep), vp(stream) if stream else None)

    rc, (d_md, _) = sized(call, lambda m=0: (torch.zeros(max(m, 1), dtype=torch.uint8, device=dev), m), rep, "md_bytes")
    _check(rc, "kiss_hip_fmi_md_dev", ctx._ctx)
    return {"d_md": d_md, "d_midx": d_midx, "d_counts": d_cnt, "rep": rep, "items": items}


def md_arrays(out):
    """the tensors of md_dev as numpy"""
    items, total = out["items"], int(out["rep"].md_bytes)
    return {"md": out["d_md"][:total].cpu().numpy(), "md_index": out["d_midx"].cpu().numpy().view(np.uint64),
            "md_counts": np.ascontiguousarray(out["d_counts"][:items].cpu().numpy()).view(np.uint32).reshape(items, 2),
            "md_report": out["rep"].as_dict()}


def md_tags(text, reads, alignments, chain_index, cigar, cigar_index, both_strands=False, hits=None, device=0, hooks=None):
    """The MD strings of alignments given as arrays (numpy in, numpy out).  text: uint8 bases 0..3; reads: a list of uint8
    arrays, or (concatenated, index); alignments: the structured array of the align call, or a (C, 12) integer array in the
    order of its fields (only rbeg, rend, tbeg and tend are read); chain_index has V + 1 entries; cigar / cigar_index: the ops
    (len << 4 | op) in CSR layout over the alignments; hits: None (one item per alignment), the structured array of the
    select call, an (H, 8) integer array in the order of its fields, or a plain sequence of alignment numbers.  Returns
    dict(md: the bytes, md_index: items + 1 u64, md_counts: (items, 2) u32 -- mismatch columns, deleted bases --, report).
    A bad item (see the header) has an empty string and is counted in report['bad']."""
    text = np.ascontiguousarray(text, dtype=np.uint8).ravel()
    cat, ridx = read_batch(reads)
    al = records(alignments, ALN_DTYPE, "the fields of an alignment record are u32")
    cidx = np.ascontiguousarray(chain_index, dtype=np.uint64).ravel()
    cig = np.ascontiguousarray(cigar, dtype=np.uint32).ravel()
    oidx = np.ascontiguousarray(cigar_index, dtype=np.uint64).ravel()
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
    ht = None
    if hits is not None:
        h = np.asarray(hits)
        if h.dtype.names or h.ndim == 2:
            ht = records(h, HIT_DTYPE, "the fields of a hit are u32")
        else:
            ht = records(h.ravel(), HIT_DTYPE, "an alignment number is u32", columns=("aln",))
    items = ht.size if ht is not None else C
    lib = _lib.load(hooks)
    rep = _lib.MdReport()
    midx = np.zeros(items + 1, np.uint64)
    cnt = np.zeros((max(items, 1), 2), np.uint32)
    (tp, rp, ap, cp, hp), hold = addresses(text, cat, al, cig, ht)

    def call(md, cap):
        return lib.kiss_hip_fmi_md_host(tp, text.size, rp, ridx.ctypes.data, Q, 1 if both_strands else 0, ap, cidx.ctypes.data, cp,
                                        oidx.ctypes.data, hp, ht.size if ht is not None else 0, md.ctypes.data, midx.ctypes.data,
                                        cnt.ctypes.data, cap, ctypes.byref(rep), int(device))

    rc, (md, _) = sized(call, lambda m=0: (np.zeros(max(m, 1), np.uint8), m), rep, "md_bytes")
    _check(rc, "kiss_hip_fmi_md_host")
    return {"md": md[:int(rep.md_bytes)], "md_index": midx, "md_counts": cnt[:items], "report": rep.as_dict()}
