#!/usr/bin/env python3
"""Maximal exact match seeds (kiss_hip_fmi_seeds_dev) on the dm-size text of bench.py's fm_query leg, one JSON line:
  - the text of bench.py (seed 1), its exact suffix array, the index built from it (SA_INTV = 4), all resident;
  - --reads (10^5) reads of --read-len (150) bases cut from the text, --sub-rate (2 %) of their bases substituted;
    min_len 19, max_occ 500, both strands;
  - ms_search / ms_compact / ms_locate / ms_sort of the report (the call with positions, best ms_total of --steps after a
    warm-up), reads/s from ms_total, seeds per read, LF pairs/s of the search kernel (lf_pairs / ms_search, best ms_search
    of the calls without positions);
  - the yardstick, in the same run on the same index: the exact range kernel (query_batch's ms_fm_range, 10^6 patterns of
    32 bases cut from the text, every one of them walks its 32 pairs) as LF pairs per second, and the ratio of the two.
One process; run it under one `timeout`.  --out FILE: the line as a JSON file.
usage: bench_seeds.py [--n N] [--reads Q] [--read-len L] [--sub-rate R] [--steps K] [--sa-intv I] [--out FILE]"""
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


def seeds_call(f, d_reads, d_index, Q, bases, params, positions, bufs):
    """one batch through kiss_hip_fmi_seeds_dev on f's context -> report dict"""
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    vex = _lib.FmiViewEx()
    vex.base = f._view()
    vex.lookup_len = f.lookup_len
    vex.lookup = f.lookup.data_ptr()
    rep = _lib.FmiSeedReport()
    min_len, max_len, max_occ, both = params
    d_pos, d_pidx, cap = (bufs["pos"], bufs["pidx"], bufs["pos"].numel()) if positions else (None, None, 0)
    rc = lib.kiss_hip_fmi_seeds_dev(f._ctx._ctx, ctypes.byref(vex), vp(d_reads.data_ptr()), vp(d_index.data_ptr()), Q, min_len,
                                    max_len, max_occ, both, None, vp(bufs["seeds"].data_ptr()), vp(bufs["sidx"].data_ptr()), bases,
                                    vp(d_pos.data_ptr()) if positions else None, vp(d_pidx.data_ptr()) if positions else None, cap,
                                    ctypes.byref(rep), None)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_seeds_dev", f._ctx._ctx)
    return rep.as_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--min-len", type=int, default=19)
    ap.add_argument("--max-occ", type=int, default=500)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sa-intv", type=int, default=4)
    ap.add_argument("--range-queries", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, Q, L = args.n, args.reads, args.read_len
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=args.sa_intv)
    bases = 2 * Q * L
    ctx = f._context(max(n + 1, 4 * (bases + 1), 4 * args.range_queries))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    at = torch.randint(0, n - L, (Q,), device=dev, generator=g)
    reads = S[at[:, None] + torch.arange(L, device=dev)[None, :]]
    sub = torch.rand((Q, L), device=dev, generator=g) < args.sub_rate
    other = (reads + 1 + torch.randint(0, 3, (Q, L), device=dev, generator=g).to(torch.uint8)) & 3
    reads = torch.where(sub, other, reads).contiguous().flatten()
    d_index = torch.arange(0, (Q + 1) * L, L, dtype=torch.int64, device=dev)
    params = (args.min_len, 0, args.max_occ, 1)
    bufs = {"seeds": torch.empty((bases, 4), dtype=torch.int32, device=dev),
            "sidx": torch.empty(2 * Q + 1, dtype=torch.int64, device=dev)}
    first = seeds_call(f, reads, d_index, Q, bases, params, False, bufs)  # warm-up; sizes the positions
    if first["positions"] > 0.3 * f._ctx.max_n:
        f._context(int(3.3 * first["positions"]) + (1 << 20))
    bufs["pos"] = torch.empty(max(first["positions"], 1), dtype=torch.int32, device=dev)
    bufs["pidx"] = torch.empty(first["seeds"] + 1, dtype=torch.int64, device=dev)
    seeds_call(f, reads, d_index, Q, bases, params, True, bufs)  # warm-up
    search = min((seeds_call(f, reads, d_index, Q, bases, params, False, bufs) for _ in range(args.steps)), key=lambda r: r["ms_search"])
    full = min((seeds_call(f, reads, d_index, Q, bases, params, True, bufs) for _ in range(args.steps)), key=lambda r: r["ms_total"])
    rate = search["lf_pairs"] / (1e-3 * search["ms_search"])
    # the yardstick: the exact range kernel on the same index
    RL, RQ = 32, args.range_queries
    at = torch.randint(0, n - RL, (RQ,), device=dev, generator=g)
    d_p = S[at[:, None] + torch.arange(RL, device=dev)[None, :]].contiguous()
    ctx = f._ctx
    ctx.set_profiling(True)
    f.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
    range_ms = float("inf")
    for _ in range(args.steps):
        s0 = ctx.stats()["ms_fm_range"]
        f.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
        range_ms = min(range_ms, ctx.stats()["ms_fm_range"] - s0)
    ctx.set_profiling(False)
    range_rate = RQ * RL / (1e-3 * range_ms)
    line = {
        "bench": "fm_seeds", "n": n, "sa_intv": args.sa_intv, "reads": Q, "read_len": L, "sub_rate": args.sub_rate,
        "min_len": args.min_len, "max_len": 0, "max_occ": args.max_occ, "both_strands": True, "steps": args.steps,
        "ends": full["bases"], "seeds": full["seeds"], "seeds_per_read": full["seeds"] / Q, "located_seeds": full["located_seeds"],
        "positions": full["positions"], "max_ms": full["max_ms"], "walk_failures": full["walk_failures"], "checksum": full["checksum"],
        "lf_pairs": search["lf_pairs"], "lf_pairs_per_read": search["lf_pairs"] / Q,
        "ms_search": round(search["ms_search"], 3), "ms_total_without_positions": round(search["ms_total"], 3),
        "ms_total": round(full["ms_total"], 3), "ms_search_in_full_call": round(full["ms_search"], 3),
        "ms_compact": round(full["ms_compact"], 3), "ms_locate": round(full["ms_locate"], 3), "ms_sort": round(full["ms_sort"], 3),
        "reads_per_s": Q / (1e-3 * full["ms_total"]), "reads_per_s_without_positions": Q / (1e-3 * search["ms_total"]),
        "lf_pairs_per_s": rate,
        "range_kernel": {"queries": RQ, "L": RL, "ms_fm_range": round(range_ms, 3), "lf_pairs_per_s": range_rate},
        "search_over_range_kernel": rate / range_rate,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")
    f.close()


if __name__ == "__main__":
    main()
