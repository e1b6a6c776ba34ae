#!/usr/bin/env python3
"""The BAM records and the BGZF framing written on the device (kiss_hip_fmi_bam_dev, kiss_hip_bgzf_dev) on the two batches of
tools/bench_sam.py: the dm-size text of bench.py (seed 1) as ONE record, its exact index (SA_INTV = 4), --pairs (5 * 10^4) pairs
and --reads (10^5) single reads of --read-len (150) bases with --sub-rate (2 %) substitutions, with MD and qualities, default
parameters everywhere.  Each batch goes through FMIndex.map / map_pairs once (sam=True, bam=True: the warm-up, and the align
call's time of that run); then the returned arrays go back to the device and, one warm-up and --steps timed calls each: the record
call (device events of the report: ms_total, ms_count, ms_emit), the framing call over its bytes (ms_total, GB/s of payload), the
device SAM call on the same arrays, and the copy of the blocks to pinned host memory.  As the host yardstick for the framing,
zlib.crc32 over the same payloads of 65280 bytes on one host thread.  All steps are listed.
Run it under one `timeout`.  --out FILE: the JSON (profiles/fm_bam_dm_size.json).
usage: bench_bam.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
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
from kiss_amd.bam_writer import bam_records_dev, bgzf_dev  # noqa: E402
from kiss_amd.sam_writer import default_names, name_index, pack_names, sam_lines_dev  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402


def rounded(xs):
    return [round(float(x), 3) for x in xs]


def time_writers(f, res, reads, index, qual, names, paired, steps, dev, n):
    up = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a).view(t) if t else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    raw, noff, nlen = pack_names(names)
    rn, rnidx = name_index(["dm"])
    source = res.get("aln_source")
    t = dict(reads=up(reads), read_index=up(index, np.int64), qual=up(qual), names=up(raw), name_off=up(noff, np.int64), name_len=up(nlen, np.int32),
             alns=up(res["alignments"].view(np.uint32), np.int32), cigar=up(res["cigar"] if res["cigar"].size else np.zeros(1, np.uint32), np.int32),
             cigar_index=up(res["cigar_index"], np.int64), hits=up(res["hits"].view(np.uint32), np.int32), hit_index=up(res["hit_index"], np.int64),
             pairs=up(res["pairs"].view(np.uint32), np.int32) if paired else None,
             source=up(np.ascontiguousarray(source, dtype=np.uint32), np.int32) if source is not None else None,
             md=up(res["md"] if res["md"].size else np.zeros(1, np.uint8)), md_index=up(res["md_index"], np.int64),
             ref_names=up(rn), ref_name_index=up(rnidx, np.int64), bounds=up(np.array([0, n], np.uint64), np.int64))
    Q, C = index.size - 1, res["alignments"].size
    first = res["first_pass"]["alignments"] if source is not None else 0
    lib = _lib.load(f._hooks)
    recs, frames, sams = [], [], []
    for _ in range(steps + 1):  # (the first one warms the pool up)
        out = bam_records_dev(lib, f._ctx, f.device, Q, C, 1, first, **t)
        recs.append(out["rep"].as_dict())
        total = int(out["rep"].bam_bytes)
        d_blocks, frep = bgzf_dev(lib, f._ctx, f.device, out["d_bam"], total)
        frames.append(frep.as_dict())
        sams.append(sam_lines_dev(lib, f._ctx, f.device, Q, C, 1, first, **t)["rep"].as_dict())
    recs, frames, sams = recs[1:], frames[1:], sams[1:]
    blocks = d_blocks.cpu().numpy().tobytes()
    assert blocks == res["bam"], "the timed calls write other bytes than map(bam=True)"
    payload = gzip.decompress(blocks)
    assert len(payload) == total
    host = torch.empty(len(blocks), dtype=torch.uint8).pin_memory()
    d2h, crc = [], []
    for _ in range(steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(d_blocks)
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for at in range(0, total, 65280):
            zlib.crc32(payload[at:at + 65280])
        crc.append((time.perf_counter() - t0) * 1e3)
    d2h, crc = d2h[1:], crc[1:]
    best, fbest, sbest = (min(x, key=lambda r: r["ms_total"]) for x in (recs, frames, sams))
    return {"reads": Q, "alignments": C, "hits": int(res["hits"].size), "records": best["records"], "bam_bytes": best["bam_bytes"],
            "bgzf_bytes": fbest["out_bytes"], "bgzf_blocks": fbest["blocks"], "sam_bytes": sbest["sam_bytes"],
            "bam_over_sam_bytes": round(fbest["out_bytes"] / sbest["sam_bytes"], 4), "longest_record": best["longest"],
            "records_ms_total": round(best["ms_total"], 3), "records_ms_count": round(best["ms_count"], 3), "records_ms_emit": round(best["ms_emit"], 3),
            "records_ms_total_all_steps": rounded(r["ms_total"] for r in recs), "records_ms_count_all_steps": rounded(r["ms_count"] for r in recs),
            "records_ms_emit_all_steps": rounded(r["ms_emit"] for r in recs),
            "framing_ms_total": round(fbest["ms_total"], 4), "framing_ms_total_all_steps": [round(r["ms_total"], 4) for r in frames],
            "framing_payload_GB_per_s": round(total / (1e-3 * fbest["ms_total"]) / 1e9, 2),
            "sam_call_ms_total_same_run": round(sbest["ms_total"], 3), "sam_call_ms_total_all_steps": rounded(r["ms_total"] for r in sams),
            "align_call_ms_total_same_run": round(res["align_report"]["ms_total"], 3),
            "d2h_blocks_ms_best": round(min(d2h), 3), "d2h_blocks_ms_all_steps": rounded(d2h),
            "host_zlib_crc32_one_thread_ms_best": round(min(crc), 3), "host_zlib_crc32_one_thread_ms_all_steps": rounded(crc),
            "host_zlib_crc32_GB_per_s": round(total / (1e-3 * min(crc)) / 1e9, 2)}


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
    line = {"bench": "fm_bam", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
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
        names = default_names(Q, paired)
        if paired:
            mates = flat.reshape(Q // 2, 2, L)
            res = f.map_pairs((mates[:, 0].reshape(-1), index[:Q // 2 + 1]), (mates[:, 1].reshape(-1), index[:Q // 2 + 1]), S, want_md=True, sam=True,
                              bam=True, qual=(list(qual.reshape(Q // 2, 2, L)[:, 0]), list(qual.reshape(Q // 2, 2, L)[:, 1])), **records)
        else:
            res = f.map((flat, index), S, both_strands=True, want_md=True, sam=True, bam=True, qual=qual, **records)
        line[what] = time_writers(f, res, flat, index, qual, names, paired, args.steps, dev, n)
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
