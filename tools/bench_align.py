#!/usr/bin/env python3
"""Alignment of chains (kiss_hip_fmi_align_dev) after the seeds call and the chain call, in one process, one JSON line:
tools/bench_seeds.py's workload -- the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), --reads (10^5) reads
of --read-len (150) bases with --sub-rate (2 %) substitutions, min_len 19, max_occ 500, both strands.  The reads, the seeds,
their positions and the chains stay on the device and go straight into the align call with the default parameters, ops
included.
Best ms_total of --steps align calls after a warm-up (device events of the report) with its three phase times, chains per
second, DP cells per second of the DP phase, and the seeds call's and the chain call's times in this same run (best of
--steps) to hold the align time against -- boxes differ.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_align_dm_size.json).
usage: bench_align.py [--n N] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import chain_call, cut_reads  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402


def align_call(f, S, n, reads, d_index, Q, chains, cidx, params, out, ocap):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.AlignReport()
    rc = lib.kiss_hip_fmi_align_dev(f._ctx._ctx, vp(S.data_ptr()), n, vp(reads.data_ptr()), vp(d_index.data_ptr()), Q, 1,
                                    vp(chains.data_ptr()), vp(cidx.data_ptr()), ctypes.byref(params), vp(out["alns"].data_ptr()),
                                    out["C"], vp(out["cigar"].data_ptr()), vp(out["oidx"].data_ptr()), ocap, ctypes.byref(rep), None)
    return rc, rep.as_dict()


def workload(S, n, Q, L, sub_rate, min_len, max_occ, sa_intv, steps, dev):
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
    best = min(runs, key=lambda r: r["ms_total"])
    alns = out["alns"][:C].to(torch.int64)
    res = {
        "n": n, "reads": Q, "read_len": L, "sub_rate": sub_rate, "min_len": min_len, "max_occ": max_occ, "both_strands": True,
        "virtual_reads": V, "seeds": seeds["seeds"], "anchors": chain["anchors"], "chains": best["chains"], "aligned": best["aligned"],
        "too_wide": best["too_wide"], "cells": best["cells"], "max_band": best["max_band"], "cigar_ops": best["cigar_ops"],
        "best_score": best["best_score"], "chains_with_a_score": int((alns[:, 0] > 0).sum()) if C else 0,
        "chains_end_to_end": int(((alns[:, 2] == 0) & (alns[:, 3] == L)).sum()) if C else 0,
        "mean_score": float(alns[:, 0].to(torch.float64).mean()) if C else 0.0,
        "ms_total": round(best["ms_total"], 3), "ms_dp": round(best["ms_dp"], 3), "ms_trace": round(best["ms_trace"], 3),
        "ms_emit": round(best["ms_emit"], 3), "ms_total_all_steps": [round(r["ms_total"], 3) for r in runs],
        "chains_per_s": best["chains"] / (1e-3 * best["ms_total"]), "reads_per_s": Q / (1e-3 * best["ms_total"]),
        "cells_per_s": best["cells"] / (1e-3 * best["ms_dp"]) if best["ms_dp"] > 0 else 0.0,
        "seeds_call_ms_total_same_run": round(seeds["ms_total"], 3), "chain_call_ms_total_same_run": round(chain["ms_total"], 3),
        "align_over_seeds_call": best["ms_total"] / seeds["ms_total"],
        "align_over_chain_call": best["ms_total"] / chain["ms_total"] if chain["ms_total"] > 0 else 0.0,
    }
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
    line = {"bench": "fm_align", "sa_intv": args.sa_intv, "steps": args.steps, "align_params": dict(fm_align.ALIGN_DEFAULTS),
            "chain_params": dict(fm_chain.CHAIN_DEFAULTS), "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(args.n, 1, dev)
    line["dm_size"] = workload(S, args.n, args.reads, args.read_len, args.sub_rate, 19, 500, args.sa_intv, args.steps, dev)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
