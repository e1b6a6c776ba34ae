#!/usr/bin/env python3
"""MD strings (kiss_hip_fmi_md_dev) after the seeds, chain, align and select calls, in one process, one JSON line:
tools/bench_select.py's workload -- the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), --reads (10^5) reads
of --read-len (150) bases with --sub-rate (2 %) substitutions, both strands, default parameters everywhere.  Everything stays
on the device; the md call runs over the hits of the select call, as FMIndex.map(want_md=True) makes it.
Best ms_total of --steps md calls after a warm-up (device events of the report) with its two phase times, the counts of the
report, and the select call's and the align call's times in this same run to hold it against -- boxes differ.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_md_dm_size.json).
usage: bench_md.py [--n N] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain, fm_select  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_select import workload  # noqa: E402


def md_stage(f, t):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    H, dev = t["H"], t["dev"]
    midx = torch.empty(H + 1, dtype=torch.int64, device=dev)
    counts = torch.empty((max(H, 1), 2), dtype=torch.int32, device=dev)

    def call(md, cap):
        rep = _lib.MdReport()
        rc = lib.kiss_hip_fmi_md_dev(f._ctx._ctx, vp(t["S"].data_ptr()), t["n"], vp(t["reads"].data_ptr()), vp(t["d_index"].data_ptr()), t["Q"], 1,
                                     vp(t["alns"].data_ptr()), vp(t["cidx"].data_ptr()), vp(t["cigar"].data_ptr()), vp(t["oidx"].data_ptr()),
                                     vp(t["hits"].data_ptr()), H, vp(md.data_ptr()), vp(midx.data_ptr()), vp(counts.data_ptr()), cap,
                                     ctypes.byref(rep), None)
        return rc, rep.as_dict()

    md = torch.empty(1, dtype=torch.uint8, device=dev)
    rc, rep = call(md, 0)  # sizes the bytes
    cap = 0
    if rc == _lib.KISS_HIP_E_INVALID and rep["md_bytes"]:
        cap = rep["md_bytes"]
        md = torch.empty(cap, dtype=torch.uint8, device=dev)
        rc, rep = call(md, cap)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_md_dev", f._ctx._ctx)
    runs = []
    for _ in range(t["steps"]):
        rc, rep = call(md, cap)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_md_dev", f._ctx._ctx)
        runs.append(rep)
    best = min(runs, key=lambda r: r["ms_total"])
    return {"md": {k: best[k] for k in ("items", "bad", "md_bytes", "mismatch_columns", "deleted_bases", "longest")},
            "md_ms_total": round(best["ms_total"], 3), "md_ms_count": round(best["ms_count"], 3), "md_ms_emit": round(best["ms_emit"], 3),
            "md_ms_total_all_steps": [round(r["ms_total"], 3) for r in runs]}


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
    line = {"bench": "fm_md", "sa_intv": args.sa_intv, "steps": args.steps, "select_params": dict(fm_select.SELECT_DEFAULTS),
            "align_params": dict(fm_align.ALIGN_DEFAULTS), "chain_params": dict(fm_chain.CHAIN_DEFAULTS),
            "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(args.n, 1, dev)
    w = workload(S, args.n, args.reads, args.read_len, args.sub_rate, 19, 500, args.sa_intv, args.steps, dev, after_select=md_stage)
    res = {k: w[k] for k in ("n", "reads", "read_len", "sub_rate", "min_len", "max_occ", "both_strands", "virtual_reads", "alignments", "hits")}
    res.update(w["md"])
    res.update(ms_total=w["md_ms_total"], ms_count=w["md_ms_count"], ms_emit=w["md_ms_emit"], ms_total_all_steps=w["md_ms_total_all_steps"],
               hits_per_s=w["hits"] / (1e-3 * w["md_ms_total"]) if w["md_ms_total"] > 0 else 0.0,
               select_call_ms_total_same_run=w["ms_total"], align_call_ms_total_same_run=w["align_call_ms_total_same_run"],
               md_over_select_call=w["md_ms_total"] / w["ms_total"] if w["ms_total"] > 0 else 0.0)
    line["dm_size"] = res
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
