#!/usr/bin/env python3
"""Insert-size estimate (kiss_hip_fmi_insert_dev) after the seeds, chain, align, select and pair calls, in one process, one JSON
line: tools/bench_pair.py's workload -- the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), --pairs (5 * 10^4)
pairs of --read-len (150) base mates with --sub-rate (2 %) substitutions, fragments of --frag-mean (400) +- --frag-sd (50) bases,
default parameters everywhere.  Everything stays on the device; the insert call runs over the hits of the select call, as
FMIndex.map_pairs(insert="auto") makes it.
Best ms_total of --steps insert calls after a warm-up (device events of the report) with its two phase times, with the
histogram in the caller's array and in the context's scratch; the report; the proper pairs with the default parameters and
with the estimate; and the pair call's and the select call's times in this same run to hold it against -- boxes differ.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_insert_dm_size.json).
usage: bench_insert.py [--n N] [--pairs P] [--read-len L] [--frag-mean M] [--frag-sd D] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain, fm_insert, fm_pair, fm_select  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_pair import pair_call, workload  # noqa: E402

COUNTS = ("P", "unmapped", "bad_input", "low_mapq", "discordant", "too_long", "samples", "used", "flags", "q25", "q50", "q75", "mean", "sd",
          "ins_min", "ins_max", "ins_mean")


def insert_stage(f, t):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    params = fm_insert.insert_params()
    hist = torch.zeros(params.max_insert + 1, dtype=torch.int32, device=t["dev"])

    def call(d_hist):
        rep = _lib.InsertReport()
        rc = lib.kiss_hip_fmi_insert_dev(f._ctx._ctx, vp(t["hits"].data_ptr()), vp(t["hidx"].data_ptr()), t["Q"], vp(t["alns"].data_ptr()), t["C"],
                                         ctypes.byref(params), vp(d_hist.data_ptr()) if d_hist is not None else None, ctypes.byref(rep), None)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_insert_dev", f._ctx._ctx)
        return rep.as_dict()

    out = {}
    for name, d_hist in (("", hist), ("scratch_", None)):
        call(d_hist)  # warm-up
        runs = [call(d_hist) for _ in range(t["steps"])]
        best = min(runs, key=lambda r: r["ms_total"])
        out.update({"insert_" + name + "ms_total": round(best["ms_total"], 4), "insert_" + name + "ms_hist": round(best["ms_hist"], 4),
                    "insert_" + name + "ms_stats": round(best["ms_stats"], 4),
                    "insert_" + name + "ms_total_all_steps": [round(r["ms_total"], 4) for r in runs]})
    out["insert"] = {k: best[k] for k in COUNTS}
    frag = t["frag"].to(torch.int64)
    out["hist_equals_the_fragment_lengths_in_bins"] = int((hist.to(torch.int64) == torch.bincount(frag, minlength=hist.numel())[:hist.numel()]).sum())
    out["fragment_mean"] = float(frag.double().mean())
    out["fragment_sd"] = float(frag.double().std())
    # the pair call once more, with the estimate in its parameters
    pp = fm_pair.pair_params(ins_min=best["ins_min"], ins_max=best["ins_max"], ins_mean=best["ins_mean"])
    pairs = torch.empty_like(t["pairs"])
    rc, rep = pair_call(f, t["hits"], t["hidx"], t["Q"], t["alns"], t["C"], pp, pairs)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_pair_dev", f._ctx._ctx)
    out["proper_with_the_estimate"] = rep["proper"]
    out["concordant_with_the_estimate"] = rep["concordant"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--frag-mean", type=int, default=400)
    ap.add_argument("--frag-sd", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sa-intv", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    line = {"bench": "fm_insert", "sa_intv": args.sa_intv, "steps": args.steps, "insert_params": dict(fm_insert.INSERT_DEFAULTS),
            "pair_params": dict(fm_pair.PAIR_DEFAULTS), "select_params": dict(fm_select.SELECT_DEFAULTS),
            "align_params": dict(fm_align.ALIGN_DEFAULTS), "chain_params": dict(fm_chain.CHAIN_DEFAULTS),
            "device": torch.cuda.get_device_name(0), "library": os.environ.get("KISS_AMD_LIB_PATH", "")}
    S = gen_text_device(args.n, 1, dev)
    w = workload(S, args.n, args.pairs, args.read_len, args.sub_rate, args.frag_mean, args.frag_sd, 19, 500, args.sa_intv, args.steps, dev,
                 after_pair=insert_stage)
    res = {k: w[k] for k in ("n", "pairs", "reads", "read_len", "sub_rate", "frag_mean", "frag_sd", "min_len", "max_occ", "alignments", "hits")}
    res.update(w["insert"])
    res.update(ms_total=w["insert_ms_total"], ms_hist=w["insert_ms_hist"], ms_stats=w["insert_ms_stats"],
               ms_total_all_steps=w["insert_ms_total_all_steps"], ms_total_hist_in_scratch=w["insert_scratch_ms_total"],
               ms_hist_hist_in_scratch=w["insert_scratch_ms_hist"], ms_stats_hist_in_scratch=w["insert_scratch_ms_stats"],
               pairs_per_s=args.pairs / (1e-3 * w["insert_ms_total"]) if w["insert_ms_total"] > 0 else 0.0,
               hist_bins=fm_insert.INSERT_DEFAULTS["max_insert"] + 1,
               hist_equals_the_fragment_lengths_in_bins=w["hist_equals_the_fragment_lengths_in_bins"],
               fragment_mean=w["fragment_mean"], fragment_sd=w["fragment_sd"],
               proper_with_the_defaults=w["proper"], concordant_with_the_defaults=w["concordant"],
               proper_with_the_estimate=w["proper_with_the_estimate"], concordant_with_the_estimate=w["concordant_with_the_estimate"],
               pair_call_ms_total_same_run=w["ms_total"], select_call_ms_total_same_run=w["select_call_ms_total_same_run"],
               insert_over_pair_call=w["insert_ms_total"] / w["ms_total"] if w["ms_total"] > 0 else 0.0)
    line["dm_size"] = res
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
