#!/usr/bin/env python3
"""FM-index over byte texts (kiss_hip_fmi8_*) on one device-resident text, one JSON line per text:
  - "zipf": 2 * 10^8 bytes, Zipf over 64 symbols with planted copies (tools/bench_general.py's text-like shape);
    "dna": the dm-size text of bench.py (seed 1) written as the bytes A C G T;
  - 10^6 patterns of 32 bytes cut from the text (a tenth of them with one byte changed);
  - build ms (text + exact suffix array resident -> index resident), ms_search / ms_locate / ms_sort of the report (best of
    --steps), queries/s with and without positions (device time of the calls), LF pairs/s;
  - yardstick (a), "dna" only: the shipped DNA index on the same text and patterns -- query_batch's ms_fm_range -- as LF
    pairs per second, nominal (Q x 32) and as walked (the lf_pairs the byte search counted: both stop at an empty range);
  - yardstick (b): a byte model of the layout.  One LF pair reads, per end of the range, 4 bytes of occ1, 2 bytes of occ2 and
    the 64-byte pieces of the block in front of the row (2.49 of them on average for a row anywhere in its block), one
    end when both fall into one block: sectors and bytes per pair from the ranges the search really walked are not known
    to the host, so the model takes two ends and says so; against the 8600 GB/s of bench.py's roofline (random rows out of
    the Infinity Cache) this gives a ceiling in LF pairs per second.  An index larger than the 256 MiB cache (the zipf
    text) is held against the same figure: the ceiling is then generous;
  - with --ab (needs libkiss_hip_hooks.so): the search with one lane per pattern and with 16 lanes per pattern
    (KISS_HIP_FM8_GROUP), alternating, same index and patterns.
One process; run it under one `timeout`.  --out FILE: the lines as one JSON array.
usage: bench_fm8.py [--texts zipf,dna] [--n N] [--queries Q] [--steps K] [--ab] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import FMIndexBytes, _lib  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402

IC_GATHER_GBS = 8600.0  # bench.py's roofline: uniformly random rows out of the Infinity Cache
PIECES_PER_END = sum(-(-r // 64) for r in range(256)) / 256.0  # 64-byte pieces of a block in front of a row: 2.49
MODEL_SECTORS_PER_PAIR = 2 * (2 + PIECES_PER_END)
MODEL_BYTES_PER_PAIR = 2 * (4 + 2 + 64 * PIECES_PER_END)


def zipf_text(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    w = 1.0 / torch.arange(1, 65, dtype=torch.float64, device=dev)
    S = (torch.multinomial(w / w.sum(), n, replacement=True, generator=g).to(torch.uint8) + 32)
    for _ in range(200):
        a, b, ln = (int(x) for x in torch.randint(0, n - 300_000, (3,), generator=g, device=dev).tolist())
        ln = 1000 + ln % 200_000
        S[b:b + ln] = S[a:a + ln].clone()
    return S


def query(f, d_pat, d_pidx, Q, positions):
    """one batch through kiss_hip_fmi8_query_dev on f's context -> report dict (positions: one call, the context is sized for it)"""
    lib = _lib.load(f._hooks)
    dev = d_pat.device
    vp = ctypes.c_void_p
    view = f._view()
    beg = torch.empty(Q, dtype=torch.int32, device=dev)
    end = torch.empty(Q, dtype=torch.int32, device=dev)
    tot, chk, rep = ctypes.c_uint64(), ctypes.c_uint64(), _lib.Fmi8Report()
    rc = lib.kiss_hip_fmi8_query_dev(f._ctx._ctx, ctypes.byref(view), vp(d_pat.data_ptr()), vp(d_pidx.data_ptr()), Q, vp(beg.data_ptr()),
                                     vp(end.data_ptr()), ctypes.byref(tot), ctypes.byref(chk), None, None, 0, ctypes.byref(rep), None)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi8_query_dev", f._ctx._ctx)
    if positions:
        total = int(tot.value)
        if total > 0.3 * f._ctx.max_n:  # one call sorts its hits in the context's LMS arrays: a context sized for them
            f._context(int(3.3 * total) + (1 << 20))
        pos = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        idx = torch.empty(Q + 1, dtype=torch.int64, device=dev)
        rc = lib.kiss_hip_fmi8_query_dev(f._ctx._ctx, ctypes.byref(view), vp(d_pat.data_ptr()), vp(d_pidx.data_ptr()), Q,
                                         vp(beg.data_ptr()), vp(end.data_ptr()), ctypes.byref(tot), ctypes.byref(chk), vp(pos.data_ptr()),
                                         vp(idx.data_ptr()), total, ctypes.byref(rep), None)
        kiss_amd.sorter._check(rc, "kiss_hip_fmi8_query_dev", f._ctx._ctx)
    return rep.as_dict()


def best(steps, fn, key):
    return min((fn() for _ in range(steps)), key=lambda r: r[key])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", default="zipf,dna")
    ap.add_argument("--n", type=int, default=0, help="text length (default: 2e8 for zipf, the dm size for dna)")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sa-intv", type=int, default=4)
    ap.add_argument("--ab", action="store_true", help="also the two lane layouts of the search (hooks build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    Q, L = args.queries, 32
    lines = []
    for name in args.texts.split(","):
        n = args.n or (200_000_000 if name == "zipf" else DM_N)
        codes = None
        if name == "zipf":
            S = zipf_text(n, dev)
        else:
            codes = gen_text_device(n, 1, dev)
            S = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[codes.long()]
        lib = _lib.load()
        f = FMIndexBytes(sa_intv=args.sa_intv)
        ctx = f._context(max(n + 1, 4 * Q))
        SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
        rc = lib.kiss_hip_ctx_suffix_sort_u8_dev(ctx._ctx, ctypes.c_void_p(S.data_ptr()), n, ctypes.c_void_p(SA.data_ptr()), None)
        kiss_amd.sorter._check(rc, "kiss_hip_ctx_suffix_sort_u8_dev", ctx._ctx)
        f.build(S, sa=SA)  # (first build: allocations)
        build_ms = float("inf")
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.build(S, sa=SA)
            torch.cuda.synchronize()
            build_ms = min(build_ms, 1e3 * (time.perf_counter() - t0))
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        pos = torch.randint(0, n - L, (Q,), device=dev, generator=g)
        pats = S[pos[:, None] + torch.arange(L, device=dev)[None, :]]
        rows = torch.nonzero(torch.rand(Q, device=dev, generator=g) < 0.1).flatten()
        col = torch.randint(0, L, (rows.numel(),), device=dev, generator=g)
        other = S[torch.randint(0, n, (rows.numel(),), device=dev, generator=g)]  # a byte of the text's own alphabet
        pats[rows, col] = other
        d_pat = pats.contiguous().flatten()
        d_pidx = torch.arange(0, (Q + 1) * L, L, dtype=torch.int64, device=dev)
        query(f, d_pat, d_pidx, Q, True)  # warm-up
        search = best(args.steps, lambda: query(f, d_pat, d_pidx, Q, False), "ms_search")
        full = best(args.steps, lambda: query(f, d_pat, d_pidx, Q, True), "ms_total")
        rate = search["lf_pairs"] / (1e-3 * search["ms_search"])
        index_bytes = sum(int(t.numel() * t.element_size()) for t in (f.bwt, f.occ1, f.occ2, f.sa, f.b, f.b_occ) if t is not None)
        model_rate = IC_GATHER_GBS * 1e9 / MODEL_BYTES_PER_PAIR
        line = {
            "bench": "fm8", "text": name, "n": n, "sigma": f.sigma, "sa_intv": args.sa_intv, "L": L, "queries": Q, "steps": args.steps,
            "index_bytes": index_bytes, "build_ms": round(build_ms, 3),
            "ms_search": round(search["ms_search"], 3), "ms_locate": round(full["ms_locate"], 3), "ms_sort": round(full["ms_sort"], 3),
            "ms_total_with_positions": round(full["ms_total"], 3),
            "queries_per_s_counts_only": Q / (1e-3 * search["ms_total"]), "queries_per_s_with_positions": Q / (1e-3 * full["ms_total"]),
            "lf_pairs": search["lf_pairs"], "lf_pairs_per_s": rate, "hits": full["hits"], "checksum": full["checksum"],
            "walk_failures": full["walk_failures"],
            "byte_model": {"bytes_per_lf_pair": MODEL_BYTES_PER_PAIR, "sectors_64B_per_lf_pair": MODEL_SECTORS_PER_PAIR,
                           "dependent_load_levels_per_lf_pair": 1, "peak_GBs": IC_GATHER_GBS,
                           "index_fits_infinity_cache": index_bytes <= 256 << 20,
                           "lf_pairs_per_s_ceiling": model_rate, "rate_over_ceiling": rate / model_rate},
            "device": torch.cuda.get_device_name(0),
        }
        if codes is not None:  # yardstick (a): the DNA index on the same text and patterns
            d = fm.FMIndex()
            ctx = d._ctx = f._ctx
            d.build(codes, sa=SA, exact_sa=True)
            lut = torch.zeros(256, dtype=torch.uint8, device=dev)
            lut[torch.tensor(list(b"ACGT"), device=dev).long()] = torch.arange(4, dtype=torch.uint8, device=dev)
            d_p = lut[pats.long()].contiguous()
            ctx.set_profiling(True)
            d.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
            range_ms = float("inf")
            for _ in range(args.steps):
                s0 = ctx.stats()["ms_fm_range"]
                d.query_batch(None, want_offsets=False, d_patterns=d_p, keep_on_device=True)
                range_ms = min(range_ms, ctx.stats()["ms_fm_range"] - s0)
            ctx.set_profiling(False)
            nominal, walked = Q * L / (1e-3 * range_ms), search["lf_pairs"] / (1e-3 * range_ms)
            line["dna_path"] = {"ms_fm_range": round(range_ms, 3), "lf_pairs_per_s_nominal_Qx32": nominal,
                                "lf_pairs_per_s_walked": walked, "rate_over_dna_nominal": rate / nominal,
                                "rate_over_dna_walked": rate / walked}
            d._ctx = None
        if args.ab:
            fh = FMIndexBytes(sa_intv=args.sa_intv, hooks=True)
            fh._context(max(n + 1, 4 * Q))
            fh.build(S, sa=SA)
            ab = {"lane": [], "group16": []}
            for _ in range(args.steps):  # alternating
                for key, env in (("lane", None), ("group16", "1")):
                    os.environ.pop("KISS_HIP_FM8_GROUP", None)
                    if env:
                        os.environ["KISS_HIP_FM8_GROUP"] = env
                    query(fh, d_pat, d_pidx, Q, False)
                    ab[key].append(query(fh, d_pat, d_pidx, Q, False))
            os.environ.pop("KISS_HIP_FM8_GROUP", None)
            line["ab_lane_layout"] = {
                k: {"ms_search": [round(r["ms_search"], 3) for r in v], "best_ms_search": round(min(r["ms_search"] for r in v), 3),
                    "lf_pairs_per_s": v[0]["lf_pairs"] / (1e-3 * min(r["ms_search"] for r in v)), "hits": v[0]["hits"]}
                for k, v in ab.items()}
            fh.close()
        lines.append(line)
        print(json.dumps(line), flush=True)
        if args.out:  # (rewritten after every text: a run that is cut short leaves what it has)
            with open(args.out, "w") as out:
                out.write("[\n" + ",\n".join(json.dumps(x) for x in lines) + "\n]\n")
        f.close()
        del S, SA, pats, d_pat


if __name__ == "__main__":
    main()
