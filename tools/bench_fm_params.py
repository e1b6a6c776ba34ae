#!/usr/bin/env python3
"""FM-index instantiations FMIndex<SA_INTV>{.LOOKUP_LEN} side by side on one device-resident text: one JSON line per
configuration with
  - build ms on the device (KISS_HIP_K_FM_BUILD kernel-class events; the k = 32 sort is done once and excluded): the
    FM arrays (the same SA_INTV at LOOKUP_LEN = 0) and the lookup table (the rest of the LOOKUP_LEN build);
  - index bytes (the .fmi size);
  - queries/s of 1 M x 32-base patterns (90 % sampled from the text, 10 % with one substitution): batched get_range +
    get_offsets (wall clock per batch, patterns and results in HBM) and ranges only (range-kernel device time);
  - parity against the (4, 0) index built in the same run: the non-empty ranges and the (hits, checksum) totals.
usage: bench_fm_params.py [--n N] [--configs 4:0,4:14,1:14,8:14] [--queries Q] [--steps K] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402


def index_bytes(f):
    sz = fm.FMIndex._sizes(f.N, f.sa_intv, f.lookup_len)
    total = 20 + 8 * (7 if f.sa_intv != 1 else 5)
    total += sz["bwt"] + sz["occ1"] * 4 + sz["occ2"] + sz["sa"] * 4 + sz["lookup"] * 4 + sz["b"] * 8 + sz["b_occ"] * 4
    return total


def build(ctx, S, SA, sa_intv, lookup_len):
    """-> index, device ms of its build (KISS_HIP_K_FM_BUILD), on the shared ctx"""
    f = fm.FMIndex(sa_intv=sa_intv, lookup_len=lookup_len)
    f._ctx = ctx
    k0 = ctx.stats()["kernels"]["fm_build"]["ms"]
    f.build(S, sa=SA)
    torch.cuda.synchronize()
    return f, ctx.stats()["kernels"]["fm_build"]["ms"] - k0


def run_queries(f, d_p, steps):
    ctx = f._ctx
    r = f.query_batch(None, want_offsets=False, d_patterns=d_p)  # warm-up; also the parity sample
    torch.cuda.synchronize()
    st0 = ctx.stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        f.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    st1 = ctx.stats()
    range_ms = (st1["ms_fm_range"] - st0["ms_fm_range"]) / steps
    locate_ms = (st1["ms_fm_locate"] - st0["ms_fm_locate"]) / steps
    return r, el, range_ms, locate_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--configs", default="4:0,4:14,1:14,8:14")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    configs = [tuple(int(x) for x in c.split(":")) for c in args.configs.split(",")]
    dev = torch.device("cuda", 0)
    n, Q, L = args.n, args.queries, 32
    S = gen_text_device(n, args.seed, dev)
    ctx = kiss_amd.Context(max_n=max(n + 1, 4 * Q), device=0)  # (FMIndex._context asks for N = n + 1)
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=fm.SORT_LEN)
    torch.cuda.synchronize()
    sort_s = time.perf_counter() - t0
    ctx.set_profiling(True)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    pos = torch.randint(0, n - L, (Q,), device=dev, generator=g)
    pats = S[pos[:, None] + torch.arange(L, device=dev)[None, :]]
    mut = torch.rand(Q, device=dev, generator=g) < 0.1
    col = torch.randint(0, L, (Q,), device=dev, generator=g)
    rows = torch.nonzero(mut).flatten()
    pats[rows, col[rows]] = (pats[rows, col[rows]] + 1) % 4
    d_p = pats.contiguous()
    base_r = None
    out = open(args.out, "a") if args.out else None
    for sa_intv, lookup_len in [(4, 0)] + [c for c in configs if c != (4, 0)]:
        f, fm_ms = build(ctx, S, SA, sa_intv, 0)  # the FM arrays alone
        lookup_ms = 0.0
        if lookup_len:
            del f
            torch.cuda.empty_cache()
            f, ms = build(ctx, S, SA, sa_intv, lookup_len)
            lookup_ms = ms - fm_ms
        r, el, range_ms, locate_ms = run_queries(f, d_p, args.steps)
        if base_r is None:
            base_r = r  # (4, 0): the CLI's instantiation
        hit = base_r["end"] > base_r["beg"]
        line = {
            "metric": "FM-index build + 1 M x 32-base queries, FMIndex<%d>{.LOOKUP_LEN = %d}" % (sa_intv, lookup_len),
            "sa_intv": sa_intv, "lookup_len": lookup_len, "n": n, "queries": Q, "steps": args.steps,
            "sort_k32_s_once": sort_s,
            "build_fm_ms": fm_ms, "build_lookup_ms": lookup_ms,
            "index_bytes": index_bytes(f),
            "queries_per_s_with_locate": Q / el, "ms_per_batch": 1e3 * el,
            "range_kernel_ms": range_ms, "locate_kernel_ms": locate_ms,
            "queries_per_s_ranges_only": Q / (1e-3 * range_ms) if range_ms > 0 else None,
            "hits": r["total_hits"], "checksum": r["checksum"],
            "parity_vs_4_0": {
                "nonempty_ranges_equal": bool(np.array_equal(r["beg"][hit], base_r["beg"][hit])
                                              and np.array_equal(r["end"][hit], base_r["end"][hit])),
                "counts_equal": bool(np.array_equal(r["end"] - r["beg"], base_r["end"] - base_r["beg"])),
                "totals_equal": r["total_hits"] == base_r["total_hits"] and r["checksum"] == base_r["checksum"],
            },
        }
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
        del f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
