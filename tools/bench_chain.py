#!/usr/bin/env python3
"""Chaining (kiss_hip_fmi_chain_dev) after the seeds call, in one process, one JSON line with two workloads:
  (1) tools/bench_seeds.py's own: the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), --reads (10^5)
      reads of --read-len (150) bases with --sub-rate (2 %) substitutions, min_len 19, max_occ 500, both strands; the
      seeds and their positions stay on the device and go straight into the chain call with the default parameters;
  (2) repeat-heavy: a text of --rep-n bases that repeats a random unit of --rep-unit bases with a few mutations,
      --rep-reads reads cut from it, max_occ 0: thousands of anchors per read, so that the DP dominates.
Per workload: best ms_total of --steps chain calls after a warm-up (device events of the report) with its three phase
times, chains per second, dp_pairs per second of the DP phase, and the chain call's time as a fraction of the seeds call's
time in this same run (best of --steps, with positions) -- that seeds time is the yardstick, boxes differ.
Run it under one `timeout`.  --out FILE: the line as a JSON file.
usage: bench_chain.py [--n N] [--reads Q] [--read-len L] [--steps K] [--skip-dm] [--skip-rep] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, fm_chain  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402


def chain_call(f, bufs, V, params, out):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.ChainReport()
    rc = lib.kiss_hip_fmi_chain_dev(f._ctx._ctx, vp(bufs["seeds"].data_ptr()), vp(bufs["sidx"].data_ptr()), V, vp(bufs["pos"].data_ptr()),
                                    vp(bufs["pidx"].data_ptr()), ctypes.byref(params), vp(out["chains"].data_ptr()),
                                    vp(out["cidx"].data_ptr()), out["chains"].shape[0], vp(out["anc"].data_ptr()),
                                    vp(out["aidx"].data_ptr()), out["anc"].shape[0], ctypes.byref(rep), None)
    return rc, rep.as_dict()


def cut_reads(S, n, Q, L, sub_rate, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    at = torch.randint(0, n - L, (Q,), device=dev, generator=g)
    reads = S[at[:, None] + torch.arange(L, device=dev)[None, :]]
    sub = torch.rand((Q, L), device=dev, generator=g) < sub_rate
    other = (reads + 1 + torch.randint(0, 3, (Q, L), device=dev, generator=g).to(torch.uint8)) & 3
    return torch.where(sub, other, reads).contiguous().flatten()


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
    params = fm_chain.chain_params()
    out = {"chains": torch.empty((1, 6), dtype=torch.int32, device=dev), "cidx": torch.empty(V + 1, dtype=torch.int64, device=dev),
           "anc": torch.empty((1, 3), dtype=torch.int32, device=dev), "aidx": torch.empty(2, dtype=torch.int64, device=dev)}
    rc, rep = chain_call(f, bufs, V, params, out)  # warm-up; sizes the output
    if rc == _lib.KISS_HIP_E_INVALID and rep["chains"]:
        out["chains"] = torch.empty((rep["chains"], 6), dtype=torch.int32, device=dev)
        out["anc"] = torch.empty((max(rep["chain_anchors"], 1), 3), dtype=torch.int32, device=dev)
        out["aidx"] = torch.empty(rep["chains"] + 1, dtype=torch.int64, device=dev)
        rc, rep = chain_call(f, bufs, V, params, out)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_chain_dev", f._ctx._ctx)
    runs = []
    for _ in range(steps):
        rc, rep = chain_call(f, bufs, V, params, out)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_chain_dev", f._ctx._ctx)
        runs.append(rep)
    best = min(runs, key=lambda r: r["ms_total"])
    anchors_of_chains = out["chains"][:, 1].to(torch.int64)
    res = {
        "n": n, "reads": Q, "read_len": L, "sub_rate": sub_rate, "min_len": min_len, "max_occ": max_occ, "both_strands": True,
        "virtual_reads": V, "seeds": seeds["seeds"], "anchors": best["anchors"], "anchors_per_virtual_read": best["anchors"] / V,
        "max_anchors": best["max_anchors"], "chains": best["chains"], "chain_anchors": best["chain_anchors"],
        "chains_with_2_or_more_anchors": int((anchors_of_chains > 1).sum()), "best_score": best["best_score"], "dp_pairs": best["dp_pairs"],
        "ms_total": round(best["ms_total"], 3), "ms_sort": round(best["ms_sort"], 3), "ms_dp": round(best["ms_dp"], 3),
        "ms_emit": round(best["ms_emit"], 3), "ms_total_all_steps": [round(r["ms_total"], 3) for r in runs],
        "chains_per_s": best["chains"] / (1e-3 * best["ms_total"]), "reads_per_s": Q / (1e-3 * best["ms_total"]),
        "dp_pairs_per_s": best["dp_pairs"] / (1e-3 * best["ms_dp"]) if best["ms_dp"] > 0 else 0.0,
        "seeds_call_ms_total_same_run": round(seeds["ms_total"], 3),
        "chain_over_seeds_call": best["ms_total"] / seeds["ms_total"],
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
    ap.add_argument("--rep-n", type=int, default=1 << 18)
    ap.add_argument("--rep-unit", type=int, default=256)
    ap.add_argument("--rep-reads", type=int, default=4000)
    ap.add_argument("--skip-dm", action="store_true")
    ap.add_argument("--skip-rep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    line = {"bench": "fm_chain", "sa_intv": args.sa_intv, "steps": args.steps, "chain_params": dict(fm_chain.CHAIN_DEFAULTS),
            "device": torch.cuda.get_device_name(0)}
    if not args.skip_dm:
        S = gen_text_device(args.n, 1, dev)
        line["dm_size"] = workload(S, args.n, args.reads, args.read_len, args.sub_rate, 19, 500, args.sa_intv, args.steps, dev)
        del S
    if not args.skip_rep:
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        n = args.rep_n
        unit = torch.randint(0, 4, (args.rep_unit,), device=dev, generator=g).to(torch.uint8)
        S = unit.repeat((n + args.rep_unit - 1) // args.rep_unit)[:n].contiguous()
        hit = torch.randint(0, n, (n // 1000,), device=dev, generator=g)  # one base in a thousand mutated
        S[hit] = (S[hit] + 1) & 3
        line["repeat_heavy"] = workload(S, n, args.rep_reads, args.read_len, args.sub_rate, 19, 0, args.sa_intv, args.steps, dev)
        line["repeat_heavy"]["unit"] = args.rep_unit
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
