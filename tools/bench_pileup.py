#!/usr/bin/env python3
"""The pileup counts (kiss_hip_fmi_pileup_dev) on ONE batch each of tools/bench_sam.py's workload: the dm-size text of bench.py
(seed 1), its exact index (SA_INTV = 4), tools/bench_pair.py's --pairs (5 * 10^4) pairs and tools/bench_select.py's --reads
(10^5) single reads of --read-len (150) bases with --sub-rate (2 %) substitutions, default parameters everywhere, the window
the whole text.  Each batch goes through FMIndex.map / map_pairs once (the select and align calls' times of that run are
recorded beside the pileup's); then the returned arrays go back to the device and the call is made once to warm up and --steps
times onto one tensor (accumulate: the walk alone; device events of the report, all listed), once more with accumulate = 0, and
the zeroing of the 32 n bytes is timed on its own.  atomic_bytes = 4 x the adds; over ms_walk it stands beside the 1.3 TB/s that
the kernel guides measured for contiguous FLOAT atomics -- an unverified yardstick: integer adds of this shape are unmeasured
there.
Run it under one `timeout`.  --out FILE: the JSON (profiles/fm_pileup_dm_size.json).
usage: bench_pileup.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from kiss_amd.fm_pileup import REPORT_COUNTS, pileup_dev  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402

FLOAT_ATOMICS_YARDSTICK_GBPS = 1300.0


def time_pileup(f, S, n, res, reads, index, paired, steps, dev):
    up = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a).view(t) if t else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    Q, H = index.size - 1, int(res["hits"].size)
    t = dict(d_reads=up(reads), d_ridx=up(index, np.int64), d_alns=up(res["alignments"].view(np.uint32), np.int32),
             d_cidx=up(res["chain_index"], np.int64), d_cigar=up(res["cigar"] if res["cigar"].size else np.zeros(1, np.uint32), np.int32),
             d_oidx=up(res["cigar_index"], np.int64), d_hits=up(res["hits"].view(np.uint32), np.int32),
             d_pairs=up(res["pairs"].view(np.uint32), np.int32) if paired else None)
    lib = _lib.load(f._hooks)
    counts = torch.zeros((8, n), dtype=torch.int32, device=dev)

    def call(d_counts):
        out = pileup_dev(lib, f._ctx, f.device, S, n, t["d_reads"], t["d_ridx"], Q, True, t["d_alns"], t["d_cidx"], t["d_cigar"], t["d_oidx"],
                         t["d_hits"], H, t["d_pairs"], Q // 2 if paired else 0, 0, n, d_counts)
        return out["rep"].as_dict()

    runs = [call(counts) for _ in range(steps + 1)][1:]  # (the first one warms the pool up)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), (steps + 1) * res["pileup"]), "the timed calls count other than map(pileup=True)"
    del counts
    fresh = call(None)  # accumulate = 0: a new tensor, zeroed by the call
    zero = torch.empty((8, n), dtype=torch.int32, device=dev)
    zero_ms = []
    for _ in range(steps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        zero.zero_()
        e1.record()
        torch.cuda.synchronize()
        zero_ms.append(e0.elapsed_time(e1))
    best = min(runs, key=lambda r: r["ms_total"])
    adds = best["columns"] + best["alt_columns"] + best["deleted_bases"] + best["insertions"] - best["clipped"]
    walk_s = 1e-3 * best["ms_walk"]
    out = {"reads": Q, "hits": H}
    out.update({k: best[k] for k in REPORT_COUNTS})
    out.update(ms_total=round(best["ms_total"], 3), ms_check=round(best["ms_check"], 3), ms_walk=round(best["ms_walk"], 3),
               ms_total_all_steps=[round(r["ms_total"], 3) for r in runs], ms_walk_all_steps=[round(r["ms_walk"], 3) for r in runs],
               adds=adds, atomic_bytes=4 * adds, atomic_gbps_over_ms_walk=round(4 * adds / walk_s / 1e9, 2) if walk_s > 0 else 0.0,
               float_atomics_yardstick_gbps_unverified=FLOAT_ATOMICS_YARDSTICK_GBPS,
               ms_total_with_zeroing=round(fresh["ms_total"], 3), ms_walk_with_zeroing=round(fresh["ms_walk"], 3),
               zeroing_bytes=32 * n, zeroing_alone_ms_all_steps=[round(x, 3) for x in zero_ms[1:]], zeroing_alone_ms_best=round(min(zero_ms[1:]), 3),
               select_call_ms_total_same_run=round(res["select_report"]["ms_total"], 3),
               align_call_ms_total_same_run=round(res["align_report"]["ms_total"], 3))
    out["pileup_over_select_plus_align"] = round(out["ms_total"] / (out["select_call_ms_total_same_run"] + out["align_call_ms_total_same_run"]), 4)
    return out


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
    line = {"bench": "fm_pileup", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    ctx = f._context(max(n + 1, 4 * (2 * max(2 * args.pairs, args.reads) * L + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    for what, paired, Q in (("reads", False, args.reads), ("pairs", True, 2 * args.pairs)):
        if not Q:
            continue
        flat = (cut_pairs(S, n, Q // 2, L, args.sub_rate, 400, 50, dev, 3)[0] if paired else cut_reads(S, n, Q, L, args.sub_rate, dev, 3)).cpu().numpy()
        index = np.arange(0, (Q + 1) * L, L, dtype=np.uint64)
        if paired:
            mates = flat.reshape(Q // 2, 2, L)
            res = f.map_pairs((mates[:, 0].reshape(-1), index[:Q // 2 + 1]), (mates[:, 1].reshape(-1), index[:Q // 2 + 1]), S, pileup=True)
        else:
            res = f.map((flat, index), S, both_strands=True, pileup=True)
        line[what] = time_pileup(f, S, n, res, flat, index, paired, args.steps, dev)
        del res
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
