#!/usr/bin/env python3
"""The reads parser (kiss_hip_reads_parse_dev) on synthetic FASTQ, one JSON line, for --records (10^5 and 10^6) records of
--read-len (150) bases cut from the dm-size text of bench.py (seed 1) with --sub-rate (2 %) substitutions, names r00000000 ...,
random qualities:
  (a) the device call on the file's bytes resident on the device: ms_total and the time per pass (lines / reads / copy) from the
      report's device events, GB/s of file bytes; and, because that is what the command line calls, kiss_hip_reads_parse_host on
      the same bytes in host memory (size call + fill call: upload, parse, download; wall clock);
  (b) the yardstick: the command line's former loader, kiss_cli::read_file, unchanged, on the same sequences written one per line,
      timed on this box's host by tools/read_file_timer.cpp (compiled here with the command line's flags);
  (c) for scale, kiss_hip_fmi_seeds_dev on the parsed batch as it comes out of (a) (min_len 19, max_occ 500, both strands, with
      positions), for up to --seeds-records-max records.
Every timing: a warm-up, then --steps (>= 5) timed calls; the best, the median and the worst are reported.
One process; run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/reads_parse.json).
usage: bench_reads.py [--records Q[,Q...]] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402

NAME = 10  # '@' 'r' and eight digits


def spread(values):
    return {"best": round(min(values), 3), "median": round(statistics.median(values), 3), "worst": round(max(values), 3), "steps": len(values)}


def make_files(S, n, Q, L, sub_rate, dev, seed):
    """-> the FASTQ file (uint8 tensor), the same sequences one per line (uint8 tensor), the codes of the reads (Q x L)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    at = torch.randint(0, n - L, (Q,), device=dev, generator=g)
    codes = S[at[:, None] + torch.arange(L, device=dev)[None, :]]
    sub = torch.rand((Q, L), device=dev, generator=g) < sub_rate
    other = (codes + 1 + torch.randint(0, 3, (Q, L), device=dev, generator=g).to(torch.uint8)) & 3
    codes = torch.where(sub, other, codes).contiguous()
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[codes.long()]
    rec = torch.full((Q, NAME + 1 + L + 1 + 2 + L + 1), 10, dtype=torch.uint8, device=dev)  # (every other byte: '\n')
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    number = torch.arange(Q, device=dev)
    for d in range(8):
        rec[:, 2 + d] = (48 + (number // 10 ** (7 - d)) % 10).to(torch.uint8)
    rec[:, NAME + 1:NAME + 1 + L] = letters
    rec[:, NAME + 2 + L] = ord("+")
    rec[:, NAME + 4 + L:NAME + 4 + 2 * L] = torch.randint(33, 127, (Q, L), device=dev, generator=g).to(torch.uint8)
    lines = torch.full((Q, L + 1), 10, dtype=torch.uint8, device=dev)
    lines[:, :L] = letters
    return rec.flatten().contiguous(), lines.flatten().contiguous(), codes


def timed_dev(lib, ctx, d_raw, outs, caps, steps):
    vp = ctypes.c_void_p
    reps = []
    for step in range(steps + 1):  # (the first is the warm-up)
        rep = _lib.ReadsReport()
        rc = lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.data_ptr()), d_raw.numel(), _lib.READS_AUTO, vp(outs["codes"].data_ptr()),
                                          vp(outs["qual"].data_ptr()), caps[0], vp(outs["index"].data_ptr()), vp(outs["noff"].data_ptr()),
                                          vp(outs["nlen"].data_ptr()), caps[1], ctypes.byref(rep), None)
        kiss_amd.sorter._check(rc, "kiss_hip_reads_parse_dev", ctx._ctx)
        if step:
            reps.append(rep.as_dict())
    return reps


def timed_host(lib, raw, Q, B, steps):
    """the entry the command line calls: the size call and the fill call on host arrays, wall clock"""
    vp = ctypes.c_void_p
    codes, qual, index = np.zeros(B + 1, np.uint8), np.zeros(B + 1, np.uint8), np.zeros(Q + 1, np.uint64)
    noff, nlen = np.zeros(Q + 1, np.uint64), np.zeros(Q + 1, np.uint32)
    ms = []
    for step in range(steps + 1):
        rep = _lib.ReadsReport()
        t0 = time.perf_counter()
        for bases_cap, reads_cap in ((0, 0), (B, Q)):
            rc = lib.kiss_hip_reads_parse_host(vp(raw.ctypes.data), raw.size, _lib.READS_AUTO, vp(codes.ctypes.data), vp(qual.ctypes.data), bases_cap,
                                               vp(index.ctypes.data), vp(noff.ctypes.data), vp(nlen.ctypes.data), reads_cap, ctypes.byref(rep), 0)
        kiss_amd.sorter._check(rc, "kiss_hip_reads_parse_host")
        if step:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, codes[:B]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--records", default="100000,1000000")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--seeds-records-max", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 5
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    n, L = args.n, args.read_len
    sizes = [int(x) for x in args.records.split(",")]
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    seed_sizes = [q for q in sizes if q <= args.seeds_records_max]
    ctx = f._context(max(n + 1, 4 * (2 * max(seed_sizes + [0]) * L + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    tmp = tempfile.mkdtemp(prefix="bench_reads_")
    timer = os.path.join(tmp, "read_file_timer")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tools", "read_file_timer.cpp"), "-o", timer])
    line = {"bench": "reads_parse", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0),
            "host_cpus_used": 1, "sizes": {}}
    for Q in sizes:
        d_raw, d_lines, codes = make_files(S, n, Q, L, args.sub_rate, dev, 3)
        nbytes, B = d_raw.numel(), Q * L
        with kiss_amd.Context(max_n=4 * nbytes + (1 << 20)) as pctx:
            outs = {"codes": torch.empty(B, dtype=torch.uint8, device=dev), "qual": torch.empty(B, dtype=torch.uint8, device=dev),
                    "index": torch.empty(Q + 1, dtype=torch.int64, device=dev), "noff": torch.empty(Q, dtype=torch.int64, device=dev),
                    "nlen": torch.empty(Q, dtype=torch.int32, device=dev)}
            reps = timed_dev(lib, pctx, d_raw, outs, (B, Q), args.steps)
        assert torch.equal(outs["codes"].reshape(Q, L), codes) and reps[0]["reads"] == Q and reps[0]["bases"] == B, "the parse is wrong"
        assert bool((outs["nlen"] == NAME - 1).all()) and int(outs["index"][-1]) == B
        best = min(reps, key=lambda r: r["ms_total"])
        res = {"records": Q, "file_bytes": nbytes, "bases": B,
               "a_parse_dev": {"ms_total": spread([r["ms_total"] for r in reps]), "ms_lines": round(best["ms_lines"], 3),
                               "ms_reads": round(best["ms_reads"], 3), "ms_copy": round(best["ms_copy"], 3),
                               "GB_per_s": round(nbytes / (1e6 * best["ms_total"]), 2), "reads_per_s": Q / (1e-3 * best["ms_total"])}}
        raw = d_raw.cpu().numpy()
        host_ms, host_codes = timed_host(lib, raw, Q, B, args.steps)
        assert np.array_equal(host_codes.reshape(Q, L), codes.cpu().numpy())
        res["a_parse_host_entry"] = {"ms_size_and_fill_calls": spread(host_ms), "GB_per_s": round(nbytes / (1e6 * min(host_ms)), 2)}
        path = os.path.join(tmp, "lines_%d.txt" % Q)
        d_lines.cpu().numpy().tofile(path)
        out = subprocess.check_output([timer, path, str(args.steps)]).split()
        assert (int(out[0]), int(out[1])) == (Q, B)
        rf_ms = [float(x) for x in out[2:]]
        res["b_read_file_host"] = {"ms": spread(rf_ms), "file_bytes": d_lines.numel(), "reads_per_s": Q / (1e-3 * min(rf_ms))}
        os.remove(path)
        res["a_over_b"] = round(best["ms_total"] / min(rf_ms), 4)
        res["a_host_entry_over_b"] = round(min(host_ms) / min(rf_ms), 4)
        if Q in seed_sizes:
            bases = 2 * B
            d_index = outs["index"]
            bufs = {"seeds": torch.empty((bases, 4), dtype=torch.int32, device=dev), "sidx": torch.empty(2 * Q + 1, dtype=torch.int64, device=dev)}
            params = (19, 0, 500, 1)
            first = seeds_call(f, outs["codes"], d_index, Q, bases, params, False, bufs)  # warm-up; sizes the positions
            if first["positions"] > 0.3 * f._ctx.max_n:
                f._context(int(3.3 * first["positions"]) + (1 << 20))
            bufs["pos"] = torch.empty(max(first["positions"], 1), dtype=torch.int32, device=dev)
            bufs["pidx"] = torch.empty(first["seeds"] + 1, dtype=torch.int64, device=dev)
            seeds_call(f, outs["codes"], d_index, Q, bases, params, True, bufs)  # warm-up
            runs = [seeds_call(f, outs["codes"], d_index, Q, bases, params, True, bufs) for _ in range(args.steps)]
            sbest = min(r["ms_total"] for r in runs)
            res["c_seeds_call"] = {"ms_total": spread([r["ms_total"] for r in runs]), "seeds": runs[0]["seeds"], "positions": runs[0]["positions"],
                                   "reads_per_s": Q / (1e-3 * sbest)}
            res["a_over_c"] = round(best["ms_total"] / sbest, 4)
            del bufs
        line["sizes"][str(Q)] = res
        del d_raw, d_lines, codes, outs
        torch.cuda.empty_cache()
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
