#!/usr/bin/env python3
"""Selection of mappings (kiss_hip_fmi_select_dev) after the seeds call, the chain call and the align call, in one process,
one JSON line: tools/bench_align.py's workload -- the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4),
--reads (10^5) reads of --read-len (150) bases with --sub-rate (2 %) substitutions, min_len 19, max_occ 500, both strands,
default parameters everywhere.  The reads, the seeds, the chains and the alignments stay on the device and go straight into
the select call.
Best ms_total of --steps select calls after a warm-up (device events of the report) with its three phase times, the counts
of the report, and the seeds call's, the chain call's and the align call's times in this same run (best of --steps) to hold
the select time against -- boxes differ.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_select_dm_size.json).
usage: bench_select.py [--n N] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain, fm_select  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_align import align_call  # noqa: E402
from bench_chain import chain_call, cut_reads  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402


def select_call(f, alns, cidx, d_index, Q, params, hits, hidx, cap):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.SelectReport()
    rc = lib.kiss_hip_fmi_select_dev(f._ctx._ctx, vp(alns.data_ptr()), vp(cidx.data_ptr()), vp(d_index.data_ptr()), Q, 1, None, 0,
                                     ctypes.byref(params), vp(hits.data_ptr()), vp(hidx.data_ptr()), cap, ctypes.byref(rep), None)
    return rc, rep.as_dict()


def workload(S, n, Q, L, sub_rate, min_len, max_occ, sa_intv, steps, dev, after_select=None):
    """after_select(f, state) -> dict: a later stage timed on the buffers of this run (tools/bench_md.py); its result is merged in"""
    f = fm.FMIndex(sa_intv=sa_intv)
    bases = 2 * Q * L
    ctx = f._context(max(n + 1, 4 * (bases + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    reads = cut_reads(S, n, Q, L, sub_rate, dev, 3)
    d_index = torch.arange(0, (Q + 1) * L, L, dtype=torch.int64, device=dev)
    sp = (min_len, 0, max_occ, 1)
    V = 2 * Q
    bufs = {"seeds": torch.empty((bases, 4), dtype=torch.int32, device=dev), "sidx": torch.empty(V + 1, dtype=torch.int64, device=dev)}
    first = seeds_call(f, reads, d_index, Q, bases, sp, False, bufs)  # warm-up; sizes the positions
    if first["positions"] > 0.3 * f._ctx.max_n:
        f._context(int(3.3 * first["positions"]) + (1 << 20))
    bufs["pos"] = torch.empty(max(first["positions"], 1), dtype=torch.int32, device=dev)
    bufs["pidx"] = torch.empty(first["seeds"] + 1, dtype=torch.int64, device=dev)
    seeds_call(f, reads, d_index, Q, bases, sp, True, bufs)  # warm-up
    seeds = min((seeds_call(f, reads, d_index, Q, bases, sp, True, bufs) for _ in range(steps)), key=lambda r: r["ms_total"])
    cparams = fm_chain.chain_params()
    ch = {"chains": torch.empty((1, 6), dtype=torch.int32, device=dev), "cidx": torch.empty(V + 1, dtype=torch.int64, device=dev),
          "anc": torch.empty((1, 3), dtype=torch.int32, device=dev), "aidx": torch.empty(2, dtype=torch.int64, device=dev)}
    rc, rep = chain_call(f, bufs, V, cparams, ch)  # warm-up; sizes the output
    if rc == _lib.KISS_HIP_E_INVALID and rep["chains"]:
        ch["chains"] = torch.empty((rep["chains"], 6), dtype=torch.int32, device=dev)
        ch["anc"] = torch.empty((max(rep["chain_anchors"], 1), 3), dtype=torch.int32, device=dev)
        ch["aidx"] = torch.empty(rep["chains"] + 1, dtype=torch.int64, device=dev)
        rc, rep = chain_call(f, bufs, V, cparams, ch)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_chain_dev", f._ctx._ctx)
    chain_runs = []
    for _ in range(steps):
        rc, rep = chain_call(f, bufs, V, cparams, ch)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_chain_dev", f._ctx._ctx)
        chain_runs.append(rep)
    chain = min(chain_runs, key=lambda r: r["ms_total"])
    C = int(chain["chains"])
    params = fm_align.align_params()
    out = {"alns": torch.empty((max(C, 1), 12), dtype=torch.int32, device=dev), "cigar": torch.empty(1, dtype=torch.int32, device=dev),
           "oidx": torch.empty(C + 1, dtype=torch.int64, device=dev), "C": C}
    ocap = 0
    rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], params, out, ocap)  # sizes the ops
    if rc == _lib.KISS_HIP_E_UNSUPPORTED and rep["cells"]:  # a context whose traceback store holds the batch
        f._context(rep["cells"] // fm_align.ALIGN_CELLS_PER_N + (1 << 20))
        rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], params, out, ocap)
    if rc == _lib.KISS_HIP_E_INVALID and rep["cigar_ops"]:
        ocap = rep["cigar_ops"]
        out["cigar"] = torch.empty(ocap, dtype=torch.int32, device=dev)
        rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], params, out, ocap)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_align_dev", f._ctx._ctx)
    runs = []
    for _ in range(steps):
        rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], params, out, ocap)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_align_dev", f._ctx._ctx)
        runs.append(rep)
    align = min(runs, key=lambda r: r["ms_total"])
    sparams = fm_select.select_params()
    hidx = torch.empty(Q + 1, dtype=torch.int64, device=dev)
    cap = C  # (a read keeps no more hits than it has alignments: one call, as FMIndex.map makes it)
    hits = torch.empty((max(cap, 1), 8), dtype=torch.int32, device=dev)
    rc, rep = select_call(f, out["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, cap)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_select_dev", f._ctx._ctx)
    sel_runs = []
    for _ in range(steps):
        rc, rep = select_call(f, out["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, cap)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_select_dev", f._ctx._ctx)
        sel_runs.append(rep)
    best = min(sel_runs, key=lambda r: r["ms_total"])
    h = hits[:best["hits"]].to(torch.int64)
    heads = (h[:, 1] & fm_select.HIT_SECONDARY) == 0
    primary = heads & ((h[:, 1] & fm_select.HIT_SUPPLEMENTARY) == 0)
    res = {
        "n": n, "reads": Q, "read_len": L, "sub_rate": sub_rate, "min_len": min_len, "max_occ": max_occ, "both_strands": True,
        "virtual_reads": V, "alignments": best["alignments"], "candidates": best["candidates"], "spanning": best["spanning"],
        "redundant": best["redundant"], "hits": best["hits"], "heads": best["heads"], "mapped": best["mapped"],
        "max_candidates": best["max_candidates"],
        "primaries_with_mapq_max": int((primary & (h[:, 2] == sparams.mapq_max)).sum()) if best["hits"] else 0,
        "primaries_with_mapq_0": int((primary & (h[:, 2] == 0)).sum()) if best["hits"] else 0,
        "ms_total": round(best["ms_total"], 3), "ms_sort": round(best["ms_sort"], 3), "ms_walk": round(best["ms_walk"], 3),
        "ms_emit": round(best["ms_emit"], 3), "ms_total_all_steps": [round(r["ms_total"], 3) for r in sel_runs],
        "alignments_per_s": best["alignments"] / (1e-3 * best["ms_total"]), "reads_per_s": Q / (1e-3 * best["ms_total"]),
        "seeds_call_ms_total_same_run": round(seeds["ms_total"], 3), "chain_call_ms_total_same_run": round(chain["ms_total"], 3),
        "align_call_ms_total_same_run": round(align["ms_total"], 3),
        "select_over_align_call": best["ms_total"] / align["ms_total"] if align["ms_total"] > 0 else 0.0,
    }
    if after_select:
        res.update(after_select(f, dict(S=S, n=n, reads=reads, d_index=d_index, Q=Q, alns=out["alns"], cidx=ch["cidx"], C=C, cigar=out["cigar"],
                                        oidx=out["oidx"], hits=hits, H=int(best["hits"]), steps=steps, dev=dev)))
    f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sa-intv", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    line = {"bench": "fm_select", "sa_intv": args.sa_intv, "steps": args.steps, "select_params": dict(fm_select.SELECT_DEFAULTS),
            "align_params": dict(fm_align.ALIGN_DEFAULTS), "chain_params": dict(fm_chain.CHAIN_DEFAULTS),
            "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(args.n, 1, dev)
    line["dm_size"] = workload(S, args.n, args.reads, args.read_len, args.sub_rate, 19, 500, args.sa_intv, args.steps, dev)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
