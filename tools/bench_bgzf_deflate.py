#!/usr/bin/env python3
"""BGZF blocks compressed on the device (kiss_hip_bgzf_deflate_dev) on the two batches of tools/bench_bam.py: the
dm-size text of bench.py (seed 1) as one record, its exact index (SA_INTV = 4), --pairs (5 * 10^4) pairs and --reads (10^5) single
reads of --read-len (150) bases with --sub-rate (2 %) substitutions, with MD and (uniformly random) qualities.  Each batch is mapped
once with bam=True (the record call's time of THAT run is listed); its unframed records go back to the device and, one warm-up and
--steps timed calls each, in the same run: the compressing call (ms_total and its three passes, GB/s of payload, the shares of
stored / fixed / dynamic blocks, output bytes over payload bytes), kiss_hip_bgzf_dev on the same buffer, the copy of the blocks to
pinned host memory stored against compressed, and zlib.compress(level 1 and 6) over the same payloads of 65280 bytes on one host
thread for time and bytes.  The best and all steps are listed.  No hardware counters are read.
Run it under one `timeout`.  --out FILE: the JSON (profiles/bgzf_deflate_dm_size.json).
usage: bench_bgzf_deflate.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import gzip
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from kiss_amd.bam_writer import bgzf_deflate_dev, bgzf_dev  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402


def rounded(xs, digits=3):
    return [round(float(x), digits) for x in xs]


def d2h_ms(d_blocks, steps):
    host = torch.empty(d_blocks.numel(), dtype=torch.uint8).pin_memory()
    ms = []
    for _ in range(steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(d_blocks)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:]


def time_framing(f, res, steps, dev):
    payload = gzip.decompress(res["bam"])
    total = len(payload)
    d_pay = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
    lib = _lib.load(f._hooks)
    packed, stored = [], []
    for _ in range(steps + 1):  # (the first one warms the pool up)
        d_small, d_index, rep = bgzf_deflate_dev(lib, f._ctx, f.device, d_pay, total)
        packed.append(rep.as_dict())
        d_blocks, frep = bgzf_dev(lib, f._ctx, f.device, d_pay, total)
        stored.append(frep.as_dict())
    packed, stored = packed[1:], stored[1:]
    small = d_small.cpu().numpy().tobytes()
    assert gzip.decompress(small) == payload and d_blocks.cpu().numpy().tobytes() == res["bam"]
    best, sbest = min(packed, key=lambda r: r["ms_total"]), min(stored, key=lambda r: r["ms_total"])
    host = {}
    for level in (1, 6):
        ms, size = [], 0
        for _ in range(2):
            t0 = time.perf_counter()
            size = 0
            for at in range(0, total, 65280):
                c = zlib.compressobj(level, zlib.DEFLATED, -15)
                size += len(c.compress(payload[at:at + 65280]) + c.flush())
            ms.append((time.perf_counter() - t0) * 1e3)
        host["host_zlib_level_%d_one_thread_ms_best" % level] = round(min(ms), 1)
        host["host_zlib_level_%d_one_thread_GB_per_s" % level] = round(total / (1e-3 * min(ms)) / 1e9, 4)
        host["host_zlib_level_%d_stream_bytes" % level] = size
    d2h_small, d2h_stored = d2h_ms(d_small, steps), d2h_ms(d_blocks, steps)
    blocks = best["blocks"]
    return dict(payload_bytes=total, blocks=blocks, out_bytes=best["out_bytes"], out_over_payload=round(best["out_bytes"] / total, 4),
                stream_bytes=best["out_bytes"] - 26 * blocks, stored_out_bytes=sbest["out_bytes"],
                share_stored=round(best["stored_blocks"] / blocks, 4), share_fixed=round(best["fixed_blocks"] / blocks, 4),
                share_dynamic=round(best["dynamic_blocks"] / blocks, 4), literals=best["literals"], matches=best["matches"], match_bytes=best["match_bytes"],
                deflate_ms_total=round(best["ms_total"], 3), deflate_ms_block=round(best["ms_block"], 3), deflate_ms_scan=round(best["ms_scan"], 3),
                deflate_ms_copy=round(best["ms_copy"], 3), deflate_ms_total_all_steps=rounded(r["ms_total"] for r in packed),
                deflate_ms_block_all_steps=rounded(r["ms_block"] for r in packed),
                deflate_payload_GB_per_s=round(total / (1e-3 * best["ms_total"]) / 1e9, 3),
                stored_framing_ms_total_same_run=round(sbest["ms_total"], 4), stored_framing_ms_total_all_steps=rounded((r["ms_total"] for r in stored), 4),
                records_call_ms_total_same_run=round(res["bam_report"]["ms_total"], 3), align_call_ms_total_same_run=round(res["align_report"]["ms_total"], 3),
                d2h_compressed_ms_best=round(min(d2h_small), 3), d2h_compressed_ms_all_steps=rounded(d2h_small),
                d2h_stored_ms_best=round(min(d2h_stored), 3), d2h_stored_ms_all_steps=rounded(d2h_stored), **host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, L = args.n, args.read_len
    line = {"bench": "bgzf_deflate", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    ctx = f._context(max(n + 1, 4 * (2 * max(2 * args.pairs, args.reads) * L + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    rng = np.random.default_rng(5)
    records = dict(ref_names=["dm"], bounds=[0, n])
    for what, paired, Q in (("pairs", True, 2 * args.pairs), ("reads", False, args.reads)):
        if not Q:
            continue
        flat = (cut_pairs(S, n, Q // 2, L, args.sub_rate, 400, 50, dev, 3)[0] if paired else cut_reads(S, n, Q, L, args.sub_rate, dev, 3)).cpu().numpy()
        index = np.arange(0, (Q + 1) * L, L, dtype=np.uint64)
        qual = rng.integers(33, 127, Q * L).astype(np.uint8)
        if paired:
            mates = flat.reshape(Q // 2, 2, L)
            res = f.map_pairs((mates[:, 0].reshape(-1), index[:Q // 2 + 1]), (mates[:, 1].reshape(-1), index[:Q // 2 + 1]), S, want_md=True, bam=True,
                              qual=(list(qual.reshape(Q // 2, 2, L)[:, 0]), list(qual.reshape(Q // 2, 2, L)[:, 1])), **records)
        else:
            res = f.map((flat, index), S, both_strands=True, want_md=True, bam=True, qual=qual, **records)
        line[what] = time_framing(f, res, args.steps, dev)
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
