#!/usr/bin/env python3
"""FM-index search with mismatches (kiss_hip_fmi_query_mm_dev) on one device-resident text, one JSON line per bound e:
  - the dm-size text of bench.py (seed 1), its EXACT suffix array, FMIndex<4>; 10^6 x 32-base patterns cut from the text
    with 0..2 substitutions (10^5 patterns for e = 3);
  - ms_search / ms_locate / ms_sort of the report (best of --steps), queries/s, lf_pairs/s, leaves and hits per pattern;
  - the yardstick: the library's own exact path on the same index and patterns -- query_batch's ms_fm_range -- as LF pairs
    per second, nominal (Q x 32) and as walked (the lf_pairs of the e = 0 search: an exact search stops at an empty
    range); the search's lf_pairs/s is given as a ratio of both;
  - with --ab (needs libkiss_hip_hooks.so): the search kernels of the hooks build as shipped (a wave per pattern for a
    batch of at most 65 536 patterns; beyond that lanes, then a wave for every pattern a lane gave up), with lanes then
    waves whatever the batch size, with lanes only, with a wave per pattern from the start, and with the lanes' bound at
    a quarter and at four times the default (KISS_HIP_FM_MM_WAVE / KISS_HIP_FM_MM_BUDGET), each also on the first 32nd
    of the batch: a small batch shows the longest pattern, and it is the size of the parts a batch with positions is
    cut into.
One process; run it under one `timeout`.  --out FILE: the lines as one JSON array.
usage: bench_fm_mismatch.py [--n N] [--queries Q] [--steps K] [--ab] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402


def mm_call(f, d_p, e, positions):
    """one batch through kiss_hip_fmi_query_mm_dev on f's context -> list of report dicts: the counts-only call, or, with
    positions, the calls of the parts the batch is cut into so that none has more hits than one call sorts (the cut
    FMIndex.query_mismatch makes, from the counts of a first call that is not in the list)"""
    lib = _lib.load(f._hooks)
    ctx, view = f._ctx, f._view()
    dev = d_p.device
    Q, L = int(d_p.shape[0]), int(d_p.shape[1])
    counts = torch.empty((Q, e + 1), dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    rep = _lib.FmiMmReport()
    rc = lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), vp(d_p.data_ptr()), L, Q, e, vp(counts.data_ptr()), None, None,
                                       None, 0, ctypes.byref(rep), None)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_query_mm_dev", ctx._ctx)
    if not positions:
        return [rep.as_dict()]
    ends = counts.to(torch.int64).sum(dim=1).cumsum(0).cpu().numpy()
    cap = int(0.32 * ctx.max_n)
    reps, lo = [], 0
    while lo < Q:
        before = int(ends[lo - 1]) if lo else 0
        hi = max(int(ends.searchsorted(before + cap, side="right")), lo + 1)
        total = int(ends[hi - 1]) - before
        pos = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        mis = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        idx = torch.empty(hi - lo + 1, dtype=torch.int64, device=dev)
        rep = _lib.FmiMmReport()
        rc = lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), vp(d_p.data_ptr() + lo * L), L, hi - lo, e,
                                           vp(counts.data_ptr() + lo * (e + 1) * 4), vp(pos.data_ptr()), vp(mis.data_ptr()),
                                           vp(idx.data_ptr()), total, ctypes.byref(rep), None)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi_query_mm_dev", ctx._ctx)
        reps.append(rep.as_dict())
        del pos, mis, idx
        lo = hi
    return reps


def best(steps, fn, key):
    out = None
    for _ in range(steps):
        reps = fn()
        v = sum(r[key] for r in reps)
        if out is None or v < out[0]:
            out = (v, reps)
    return out[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bounds", default="0,1,2,3")
    ap.add_argument("--ab", action="store_true", help="also the tiers of the search apart (hooks build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, Q, L = args.n, args.queries, 32
    S = gen_text_device(n, args.seed, dev)
    ctx = kiss_amd.Context(max_n=max(n + 1, 4 * Q), device=0)
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex()
    f._ctx = ctx
    f.build(S, sa=SA, exact_sa=True)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pos = torch.randint(0, n - L, (Q,), device=dev, generator=g)
    pats = S[pos[:, None] + torch.arange(L, device=dev)[None, :]]
    nsub = torch.randint(0, 3, (Q,), device=dev, generator=g)  # 0, 1 or 2 substitutions
    for k in range(2):
        rows = torch.nonzero(nsub > k).flatten()
        col = torch.randint(0, L, (rows.numel(),), device=dev, generator=g)
        pats[rows, col] = (pats[rows, col] + 1 + torch.randint(0, 3, (rows.numel(),), device=dev, generator=g).to(torch.uint8)) % 4
    d_p = pats.contiguous()
    # the yardstick: the exact path's range kernel on the same index and patterns
    ctx.set_profiling(True)
    f.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
    range_ms = float("inf")
    for _ in range(args.steps):
        s0 = ctx.stats()["ms_fm_range"]
        f.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
        range_ms = min(range_ms, ctx.stats()["ms_fm_range"] - s0)
    ctx.set_profiling(False)
    e0 = mm_call(f, d_p, 0, False)[0]
    exact_nominal = Q * L / (1e-3 * range_ms)
    exact_walked = e0["lf_pairs"] / (1e-3 * range_ms)
    fh = None
    if args.ab:
        fh = fm.FMIndex(hooks=True)
        fh._ctx = kiss_amd.Context(max_n=max(n + 1, 4 * Q), device=0, hooks=True)
        fh.build(S, sa=SA, exact_sa=True)
    del SA
    lines = []
    for e in [int(x) for x in args.bounds.split(",")]:
        q = Q if e < 3 else Q // 10
        p = d_p[:q]
        mm_call(f, p, e, False)  # warm-up: the pool grows to this batch
        search = best(args.steps, lambda: mm_call(f, p, e, False), "ms_search")[0]
        full = best(args.steps, lambda: mm_call(f, p, e, True), "ms_total")
        hits = [sum(r["hits"][j] for r in full) for j in range(4)]
        rate = search["lf_pairs"] / (1e-3 * search["ms_search"])
        line = {
            "bench": "fm_mismatch", "n": n, "sa_intv": 4, "L": L, "queries": q, "max_mismatches": e, "steps": args.steps,
            "ms_search": round(search["ms_search"], 3),
            "ms_locate": round(sum(r["ms_locate"] for r in full), 3), "ms_sort": round(sum(r["ms_sort"] for r in full), 3),
            "ms_total_with_positions": round(sum(r["ms_total"] for r in full), 3), "calls_with_positions": len(full),
            "ms_search_in_those_calls": round(sum(r["ms_search"] for r in full), 3),
            "queries_per_s_counts_only": q / (1e-3 * search["ms_total"]),
            "queries_per_s_with_positions": q / (1e-3 * sum(r["ms_total"] for r in full)),
            "lf_pairs": search["lf_pairs"], "lf_pairs_per_s": rate, "lf_pairs_per_pattern": search["lf_pairs"] / q,
            "leaves_per_pattern": search["ranges"] / q, "hits_by_mismatch": hits[:e + 1], "hits_per_pattern": sum(hits) / q,
            "checksum": sum(r["checksum"] for r in full), "walk_failures": sum(r["walk_failures"] for r in full),
            "exact_path": {"ms_fm_range": round(range_ms, 3), "lf_pairs_per_s_nominal_Qx32": exact_nominal,
                           "lf_pairs_walked": e0["lf_pairs"], "lf_pairs_per_s_walked": exact_walked},
            "rate_over_exact_nominal": rate / exact_nominal, "rate_over_exact_walked": rate / exact_walked,
            "device": torch.cuda.get_device_name(0),
        }
        if fh is not None and e:
            dflt = {1: 1024, 2: 8192, 3: 131072}[e]  # MM_HEAVY_PAIRS of fm_mm.hip
            variants = (("hooks_as_shipped", {}), ("hooks_lanes_then_waves", {"KISS_HIP_FM_MM_BUDGET": str(dflt)}),
                        ("hooks_lane_only", {"KISS_HIP_FM_MM_BUDGET": str(1 << 62)}),
                        ("hooks_wave_only", {"KISS_HIP_FM_MM_WAVE": "1"}),
                        ("hooks_bound_quarter", {"KISS_HIP_FM_MM_BUDGET": str(dflt // 4)}),
                        ("hooks_bound_x4", {"KISS_HIP_FM_MM_BUDGET": str(dflt * 4)}))
            for name, env in variants:
                for k in ("KISS_HIP_FM_MM_BUDGET", "KISS_HIP_FM_MM_WAVE"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                mm_call(fh, p, e, False)
                r = best(args.steps, lambda: mm_call(fh, p, e, False), "ms_search")[0]
                small = best(args.steps, lambda: mm_call(fh, p[:q // 32], e, False), "ms_search")[0]
                lr = r["lf_pairs"] / (1e-3 * r["ms_search"])
                line[name] = {"env": env, "ms_search": round(r["ms_search"], 3), "ms_search_first_32nd_of_the_batch": round(small["ms_search"], 3),
                              "lf_pairs": r["lf_pairs"], "lf_pairs_per_s": lr,
                              "rate_over_exact_nominal": lr / exact_nominal, "rate_over_exact_walked": lr / exact_walked,
                              "hits_equal": r["hits"] == search["hits"]}
            for k in ("KISS_HIP_FM_MM_BUDGET", "KISS_HIP_FM_MM_WAVE"):
                os.environ.pop(k, None)
        lines.append(line)
        print(json.dumps(line), flush=True)
        if args.out:  # (rewritten after every bound: a run that is cut short leaves what it has)
            with open(args.out, "w") as out:
                out.write("[\n" + ",\n".join(json.dumps(x) for x in lines) + "\n]\n")


if __name__ == "__main__":
    main()
