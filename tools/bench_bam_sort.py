#!/usr/bin/env python3
"""The coordinate sort of BAM records on the device (kiss_hip_bam_sort_dev) on the two batches of tools/bench_bam.py:
the dm-size text of bench.py (seed 1) as ONE record, its exact index (SA_INTV = 4), --pairs (5 * 10^4) pairs and --reads (10^5)
single reads of --read-len (150) bases with --sub-rate (2 %) substitutions, with MD and qualities, default parameters everywhere.
Each batch goes through FMIndex.map / map_pairs once (bam=True: the warm-up); then the returned arrays go back to the device and, one
warm-up and --steps timed rounds, every round in this order: the record call (kiss_hip_fmi_bam_dev, the report's ms_total), the
sort of its records (ms_key / ms_sort / ms_copy / ms_total of the report: device events), a plain device-to-device copy of the same
bytes (two events around one copy_ of bam_bytes: the yardstick of the gather, which reads and writes the same bytes), and the
framing of the sorted bytes (kiss_hip_bgzf_dev).  The gather's GB/s counts bam_bytes read plus bam_bytes written over ms_copy, which
also holds the sizes pass and the scan; the copy's GB/s counts the same bytes over its own time.  The sorted bytes are held against
numpy's stable argsort over the keys before anything is timed.  Host alternative, in the same process on ONE thread: Python's
sorted() over the decoded records with the key (rk, pos + 1), then b"".join.  All steps are listed.
Run it under one `timeout`.  --out FILE: the JSON (profiles/fm_bam_sort_dm_size.json).
usage: bench_bam_sort.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import gzip
import json
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from kiss_amd.bam_writer import bam_records_dev, bam_sort_dev, bgzf_dev  # noqa: E402
from kiss_amd.sam_writer import default_names, name_index, pack_names  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402


def rounded(xs, digits=4):
    return [round(float(x), digits) for x in xs]


def host_sort(raw, index):
    """sorted() over the decoded records on one thread -> (ms, the sorted bytes)"""
    t0 = time.perf_counter()
    recs = [raw[int(index[r]):int(index[r + 1])] for r in range(index.size - 1)]

    def key(rec):
        ref, pos = struct.unpack_from("<ii", rec, 4)
        return (1 if ref == -1 else ref, pos + 1)  # (one reference: rk = n_ref = 1 for a record without a place)

    out = b"".join(sorted(recs, key=key))
    return (time.perf_counter() - t0) * 1e3, out


def time_sort(f, res, reads, index, qual, names, paired, steps, dev, n):
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
    payload = gzip.decompress(res["bam"])
    ri = res["bam_rec_index"]
    # the yardstick of correctness, before anything is timed
    heads = np.frombuffer(payload, np.uint8)[(ri[:-1].astype(np.int64)[:, None] + np.arange(4, 12)[None, :])].copy().view("<i4")
    rk = np.where(heads[:, 0] == -1, 1, heads[:, 0]).astype(np.int64)
    want_order = np.argsort(rk * (1 << 32) + heads[:, 1].astype(np.int64) + 1, kind="stable")
    recs, sorts, copies, frames = [], [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for step in range(steps + 1):  # (the first round warms the pool up)
        out = bam_records_dev(lib, f._ctx, f.device, Q, C, 1, first, **t)
        total, records = int(out["rep"].bam_bytes), int(out["rep"].records)
        got = bam_sort_dev(lib, f._context_to_sort(f._ctx, records), f.device, out["d_bam"], total, out["d_rec_index"], records, 1)
        d_copy = torch.empty(total, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        e0.record()
        d_copy.copy_(out["d_bam"][:total])
        e1.record()
        torch.cuda.synchronize()
        d_blocks, frep = bgzf_dev(lib, f._ctx, f.device, got["d_bam"], total)
        if step == 0:
            assert np.array_equal(got["d_order"].cpu().numpy().view(np.uint32), want_order.astype(np.uint32)), "the order is not numpy's stable one"
            assert out["d_bam"][:total].cpu().numpy().tobytes() == payload, "the timed record call writes other bytes than map(bam=True)"
            sorted_bytes = got["d_bam"].cpu().numpy().tobytes()
            continue
        recs.append(out["rep"].as_dict())
        sorts.append(got["rep"].as_dict())
        copies.append(e0.elapsed_time(e1))
        frames.append(frep.as_dict())
    host_ms, host_bytes = zip(*(host_sort(payload, ri) for _ in range(3)))
    assert host_bytes[0] == sorted_bytes, "sorted() on the host gives other bytes than the device"
    best = min(sorts, key=lambda r: r["ms_total"])
    gbs = lambda ms: round(2 * total / (1e-3 * ms) / 1e9, 1)  # noqa: E731 (read plus write)
    return {"reads": Q, "records": records, "bam_bytes": total, "unplaced": best["unplaced"], "longest_record": best["longest"],
            "sort_ms_total": round(best["ms_total"], 4), "sort_ms_key": round(best["ms_key"], 4), "sort_ms_sort": round(best["ms_sort"], 4),
            "sort_ms_copy": round(best["ms_copy"], 4),
            **{"sort_%s_all_steps" % k: rounded(r[k] for r in sorts) for k in ("ms_total", "ms_key", "ms_sort", "ms_copy")},
            "gather_GB_per_s_read_plus_write": gbs(best["ms_copy"]),
            "plain_d2d_copy_ms_best": round(min(copies), 4), "plain_d2d_copy_ms_all_steps": rounded(copies),
            "plain_d2d_copy_GB_per_s_read_plus_write": gbs(min(copies)),
            "gather_over_plain_copy": round(best["ms_copy"] / min(copies), 2),
            "records_call_ms_total_same_run": round(min(r["ms_total"] for r in recs), 4), "records_call_ms_total_all_steps": rounded(r["ms_total"] for r in recs),
            "framing_ms_total_same_run": round(min(r["ms_total"] for r in frames), 4), "framing_ms_total_all_steps": rounded(r["ms_total"] for r in frames),
            "host_alternative": "Python sorted() over the decoded records, key (rk, pos + 1), then join; one thread, same process",
            "host_sorted_one_thread_ms_best": round(min(host_ms), 2), "host_sorted_one_thread_ms_all": rounded(host_ms, 2),
            "host_over_device_sort": round(min(host_ms) / best["ms_total"], 1)}


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
    line = {"bench": "fm_bam_sort", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
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
            res = f.map_pairs((mates[:, 0].reshape(-1), index[:Q // 2 + 1]), (mates[:, 1].reshape(-1), index[:Q // 2 + 1]), S, want_md=True, bam=True,
                              qual=(list(qual.reshape(Q // 2, 2, L)[:, 0]), list(qual.reshape(Q // 2, 2, L)[:, 1])), **records)
        else:
            res = f.map((flat, index), S, both_strands=True, want_md=True, bam=True, qual=qual, **records)
        line[what] = time_sort(f, res, flat, index, qual, names, paired, args.steps, dev, n)
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
