#!/usr/bin/env python3
"""A read file mapped in batches (kiss_amd.batches), one JSON line, one process:
  (a) the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), --pairs (5 * 10^4) pairs of --read-len (150) base mates
      with --sub-rate (2 %) substitutions, fragments of --frag-mean (400) +- --frag-sd (50) bases, written as two FASTQ files:
      map_file() over them at every --batch-reads (10^4 and 5 * 10^4 pairs), wall clock from the first byte read to the last
      batch's result, against parse_reads() of the two files and ONE map_pairs() call on them in this same run -- boxes differ.
      The proper pairs of every way are reported: they are equal.
  (b) a FASTQ file of --records (10^6) records made as tools/bench_reads.py makes it, resident on the device:
      kiss_hip_reads_parse_part_dev with `final` and every record taken, and cut at half the records without `final`, against
      kiss_hip_reads_parse_dev on the same bytes: ms_total and ms_lines of the reports (device events; the part call's include the
      passes that find the cut).
Every timing: a warm-up, then --steps timed runs, the best and all of them.  Run it under one `timeout`.
--out FILE: the line as a JSON file (profiles/map_file_dm_size.json).
usage: bench_map_file.py [--n N] [--pairs P] [--batch-reads B[,B...]] [--records Q] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, batches  # noqa: E402
from kiss_amd.reads import parse_reads  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_reads import NAME, make_files  # noqa: E402


def fastq_bytes(codes, dev):
    """Q x L codes -> the bytes of a FASTQ file with names r00000000 ... and one quality letter"""
    Q, L = codes.shape
    rec = torch.full((Q, NAME + 1 + L + 1 + 2 + L + 1), 10, dtype=torch.uint8, device=dev)
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    number = torch.arange(Q, device=dev)
    for d in range(8):
        rec[:, 2 + d] = (48 + (number // 10 ** (7 - d)) % 10).to(torch.uint8)
    rec[:, NAME + 1:NAME + 1 + L] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[codes.long()]
    rec[:, NAME + 2 + L] = ord("+")
    rec[:, NAME + 4 + L:NAME + 4 + 2 * L] = ord("I")
    return rec.flatten().contiguous()


def pair_files(S, n, P, L, sub_rate, frag_mean, frag_sd, dev, tmp):
    """two FASTQ files of P mates each: forward-then-reverse pairs cut from S"""
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    frag = (frag_mean + frag_sd * torch.randn(P, device=dev, generator=g)).round().long().clamp(L, 4 * frag_mean)
    at = (torch.rand(P, device=dev, generator=g) * (n - 4 * frag_mean - 1)).long()
    span = torch.arange(L, device=dev)[None, :]
    m1 = S[at[:, None] + span]
    m2 = 3 - S[(at + frag - 1)[:, None] - span]  # the reverse complement of the fragment's last L bases
    paths = []
    for which, codes in enumerate((m1, m2)):
        sub = torch.rand((P, L), device=dev, generator=g) < sub_rate
        other = (codes + 1 + torch.randint(0, 3, (P, L), device=dev, generator=g).to(torch.uint8)) & 3
        paths.append(os.path.join(tmp, "mates%d.fastq" % (which + 1)))
        fastq_bytes(torch.where(sub, other, codes).contiguous(), dev).cpu().numpy().tofile(paths[-1])
    return paths


def timed(run, steps):
    out, ms = None, []
    for step in range(steps + 1):  # (the first is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        if step:
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out, {"best_ms": min(ms), "all_ms": ms}


def proper_of(res):
    return int(res["pair_report"]["proper"]) if "pair_report" in res else int(res["report"]["proper"])


def part_a(args, dev):
    S = gen_text_device(args.n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    ctx = f._context(args.n + 1)
    SA = torch.empty(args.n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), args.n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    tmp = tempfile.mkdtemp(prefix="bench_map_file_")
    paths = pair_files(S, args.n, args.pairs, args.read_len, args.sub_rate, args.frag_mean, args.frag_sd, dev, tmp)
    res = {"n": args.n, "pairs": args.pairs, "read_len": args.read_len, "file_bytes": [os.path.getsize(p) for p in paths]}

    def whole():
        a, b = (parse_reads(p, want_names=False, device=0) for p in paths)
        t1 = time.perf_counter()
        out = f.map_pairs((a["reads"], a["read_index"]), (b["reads"], b["read_index"]), S)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t1) * 1e3

    (out, _), res["parse_reads_and_one_map_pairs_call"] = timed(whole, args.steps)
    res["one_map_pairs_call_alone_best_ms"] = round(min(whole()[1] for _ in range(args.steps)), 3)
    res["proper_pairs_one_call"] = proper_of(out)
    res["map_file"] = {}
    for B in [int(x) for x in args.batch_reads.split(",")]:
        got, t = timed(lambda: list(batches.map_file(f, paths[0], S, paths[1], batch_reads=B)), args.steps)
        t.update(batches=len(got), proper_pairs=sum(proper_of(r) for r in got), over_one_call=round(t["best_ms"] / res["parse_reads_and_one_map_pairs_call"]["best_ms"], 4))
        res["map_file"][str(B)] = t
    for p in paths:
        os.remove(p)
    os.rmdir(tmp)
    f.close()
    return res


def part_b(args, dev):
    lib, vp, Q, L = _lib.load(), ctypes.c_void_p, args.records, args.read_len
    S = gen_text_device(1 << 22, 1, dev)
    d_raw, _, _ = make_files(S, 1 << 22, Q, L, args.sub_rate, dev, 3)
    B, nbytes = Q * L, d_raw.numel()
    outs = [torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(Q + 1, dtype=torch.int64, device=dev),
            torch.empty(Q, dtype=torch.int64, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)]
    ptr = [vp(t.data_ptr()) for t in outs]
    res = {"records": Q, "file_bytes": nbytes}
    with kiss_amd.Context(max_n=4 * nbytes + (1 << 20)) as ctx:
        def parse():
            rep = _lib.ReadsReport()
            rc = lib.kiss_hip_reads_parse_dev(ctx._ctx, vp(d_raw.data_ptr()), nbytes, _lib.READS_AUTO, ptr[0], ptr[1], B, ptr[2], ptr[3], ptr[4], Q,
                                              ctypes.byref(rep), None)
            kiss_amd.sorter._check(rc, "kiss_hip_reads_parse_dev", ctx._ctx)
            return rep

        def part(final, max_records):
            rep = _lib.ReadsPartReport()
            rc = lib.kiss_hip_reads_parse_part_dev(ctx._ctx, vp(d_raw.data_ptr()), nbytes, _lib.READS_AUTO, final, max_records, ptr[0], ptr[1], B, ptr[2],
                                                   ptr[3], ptr[4], Q, ctypes.byref(rep), None)
            kiss_amd.sorter._check(rc, "kiss_hip_reads_parse_part_dev", ctx._ctx)
            return rep

        for name, run in (("parse_dev", parse), ("part_dev_final_all_records", lambda: part(1, 0).parsed),
                          ("part_dev_cut_at_half", lambda: part(0, Q // 2).parsed)):
            run()  # warm-up
            reps = [run() for _ in range(args.steps)]
            best = min(reps, key=lambda r: r.ms_total)
            res[name] = {"ms_total": round(best.ms_total, 3), "ms_lines": round(best.ms_lines, 3), "ms_reads": round(best.ms_reads, 3),
                         "ms_copy": round(best.ms_copy, 3), "reads": int(best.reads), "ms_total_all_steps": [round(r.ms_total, 3) for r in reps]}
    p = res["parse_dev"]
    res["part_final_over_parse"] = round(res["part_dev_final_all_records"]["ms_total"] / p["ms_total"], 4)
    res["part_final_minus_parse_minus_its_ms_lines"] = round(res["part_dev_final_all_records"]["ms_total"] - p["ms_total"] - p["ms_lines"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--batch-reads", default="10000,50000")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--frag-mean", type=int, default=400)
    ap.add_argument("--frag-sd", type=int, default=50)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    line = {"bench": "map_file", "steps": args.steps, "device": torch.cuda.get_device_name(0), "library": os.environ.get("KISS_AMD_LIB_PATH", "")}
    line["part_call"] = part_b(args, dev)
    torch.cuda.empty_cache()
    line["dm_size"] = part_a(args, dev)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
