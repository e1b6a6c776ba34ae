#!/usr/bin/env python3
"""Time of the LCP array (kiss_hip_ctx_lcp_dna_u32_dev / kiss_hip_ctx_lcp_u8_dev) beside the exact sort it follows, text and
SA resident on the device.  One JSON line per text:
  chm13     the seeded chm13-size stand-in of bench.py (bench.gen_text_device, seed 2)
  harsh     the same with bench.py's --harsh satellite profile
  allA      10^8 A's: one irreducible pair, of lcp n - 1 (the grid-wide compare)
  bytes     2 * 10^8 uniform random bytes
Each line: the exact-sort and LCP times (best of --steps), the report's phases and counters, and the LCP time against a
byte + random-sector model: 3 random 4-byte accesses per base (Phi scatter, the chunk gathered at Phi(i) - 1, the PLCP
gather) at RANDOM_SECTORS_PER_S, plus the streamed bytes at STREAM_BYTES_PER_S.  usage: bench_lcp.py [--steps K] [--only NAME]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import kiss_amd  # noqa: E402
from bench import CHM13_N, gen_text_device  # noqa: E402

RANDOM_SECTORS_PER_S = 45e9  # random 64-byte sector reads of HBM, measured for the refinement walks
STREAM_BYTES_PER_S = 4.0e12  # what the streaming kernels of the library reach (about 3/4 of the HBM peak)
# streamed bytes per base: Phi fill 4, SA read 4 + 4 (scatter, gather), X read + write 4 + 4 (short compare), the max-scan
# 4 + 4 + 4, LCP write 4, the text read once by the packing / padded copy (1) and its chunks (~1 for the lane's own chunk)
STREAM_BYTES_PER_BASE = 42


def model_ms(n):
    return 1e3 * (3 * n / RANDOM_SECTORS_PER_S + STREAM_BYTES_PER_BASE * n / STREAM_BYTES_PER_S)


def best_of(steps, fn):
    best = float("inf")
    out = None
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return 1e3 * best, out


def run(name, desc, S, alphabet, steps, ctx):
    n = S.numel()
    dev = S.device
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    LCP = torch.empty(n + 1, dtype=torch.int32, device=dev)
    if alphabet == "dna":
        sort = lambda: ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), kiss_amd.K_UNBOUNDED,  # noqa: E731
                                           kiss_amd.ALGO_PREFIX_DOUBLING)
    else:
        sort = lambda: kiss_amd.sorter._check(ctx._lib.kiss_hip_ctx_suffix_sort_u8_dev(  # noqa: E731
            ctx._ctx, S.data_ptr(), n, SA.data_ptr(), None), "kiss_hip_ctx_suffix_sort_u8_dev")
    sort()  # first-use allocations
    sort_ms, _ = best_of(steps, sort)
    ver = ctx.verify_sa_dev(S.data_ptr(), n, SA.data_ptr(), 0xFFFFFFFF)
    ws = ctx.workspace_bytes()
    lcp = lambda: ctx.lcp_dev(S.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), alphabet=alphabet)  # noqa: E731
    lcp_ms, rep = best_of(steps, lcp)
    host_sum = int(LCP[1:].to(torch.int64).sum().item())
    m = model_ms(n)
    line = {"bench": "lcp", "text": name, "desc": desc, "alphabet": alphabet, "n": n, "steps": steps,
            "sort_exact_ms": round(sort_ms, 3), "sa_verified": bool(ver["ok"]), "lcp_ms": round(lcp_ms, 3),
            "lcp_over_sort": round(lcp_ms / sort_ms, 3),
            "phases_ms": {k: round(rep[k], 3) for k in ("ms_total", "ms_phi", "ms_short", "ms_long", "ms_scan_gather")},
            "irreducible": rep["irreducible"], "irreducible_per_base": round(rep["irreducible"] / max(1, n), 4),
            "long_pairs": rep["long_pairs"], "max_lcp": rep["max_lcp"], "lcp_sum": rep["lcp_sum"],
            "lcp_sum_matches_device_sum": host_sum == rep["lcp_sum"], "lcp0_zero": int(LCP[0].item()) == 0,
            "workspace_unchanged_by_lcp": ctx.workspace_bytes() == ws,
            "model": {"ms": round(m, 3), "rule": "3 random 4-B accesses/base at %.0f G sectors/s + %d streamed B/base at %.1f TB/s"
                      % (RANDOM_SECTORS_PER_S / 1e9, STREAM_BYTES_PER_BASE, STREAM_BYTES_PER_S / 1e12),
                      "lcp_ms_over_model": round(lcp_ms / m, 3)},
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    del SA, LCP
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated subset of chm13,harsh,allA,bytes")
    ap.add_argument("--n", type=int, default=CHM13_N, help="length of the genome-like texts")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    dev = torch.device("cuda", 0)
    texts = [("chm13", "genome-like synthetic, chm13 size (bench.gen_text_device)", "dna",
              lambda: gen_text_device(args.n, args.seed, dev)),
             ("harsh", "genome-like synthetic, chm13 size, --harsh satellite profile", "dna",
              lambda: gen_text_device(args.n, args.seed, dev, harsh=True)),
             ("allA", "10^8 A", "dna", lambda: torch.zeros(100_000_000, dtype=torch.uint8, device=dev)),
             ("bytes", "2*10^8 uniform random bytes", "bytes",
              lambda: torch.randint(0, 256, (200_000_000,), dtype=torch.uint8, device=dev,
                                    generator=torch.Generator(device=dev).manual_seed(args.seed)))]
    texts = [t for t in texts if not only or t[0] in only]
    ctx = None
    for name, desc, alphabet, make in texts:
        S = make()
        if ctx is None or ctx.max_n < S.numel():
            if ctx is not None:
                ctx.close()
            ctx = kiss_amd.Context(max_n=max(S.numel(), 200_000_000))
        run(name, desc, S, alphabet, args.steps, ctx)
        del S
        torch.cuda.empty_cache()
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
