#!/usr/bin/env python3
"""Duplicate marking of BAM records on the device (kiss_hip_bam_markdup_dev) on the two batches of
tools/bench_bam_sort.py with planted copies: the dm-size text of bench.py (seed 1) as ONE record, its exact index (SA_INTV = 4),
--pairs (5 * 10^4) pairs and --reads (10^5) single reads of --read-len (150) bases with --sub-rate (2 %) substitutions, with MD and
qualities, default parameters everywhere; one pair or read in ten stands a second time at the end of the batch, with qualities of
its own (as they stand the batches hold almost no duplicates).  Each batch goes through FMIndex.map / map_pairs once (bam=True: the
warm-up); then the returned arrays go back to the device and, one warm-up and --steps timed rounds, every round in this order: the
record call (kiss_hip_fmi_bam_dev, the report's ms_total), the marking of its records in place (ms_record / ms_class / ms_sort /
ms_mark / ms_total of the report: device events), and the sort of the marked records (kiss_hip_bam_sort_dev, ms_total).  The marked
bytes and every count are held against tests/markdup_model.py before anything is timed; that model, timed once on ONE host thread in
the same process, is the host alternative.  All steps are listed.
Run it under one `timeout`.  --out FILE: the JSON (profiles/fm_bam_markdup_dm_size.json).
usage: bench_bam_markdup.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib  # noqa: E402
from kiss_amd.bam_writer import bam_markdup_dev, bam_records_dev, bam_sort_dev  # noqa: E402
from kiss_amd.sam_writer import default_names, name_index, pack_names  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402
from tests import markdup_model  # noqa: E402

COUNTS = ("records", "templates", "pairs", "fragments", "unmapped_templates", "ambiguous", "dup_pairs", "dup_fragments", "dup_records", "bad",
          "first_bad")
PHASES = ("ms_total", "ms_record", "ms_class", "ms_sort", "ms_mark")


def rounded(xs, digits=4):
    return [round(float(x), digits) for x in xs]


def time_markdup(f, res, reads, index, qual, names, paired, steps, dev, n):
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
    # the yardstick of correctness, and the host alternative: the model, once, on one thread
    t0 = time.perf_counter()
    want = markdup_model.markdup_model(payload, ri, 1, 15, decide=markdup_model.duplicates_by_dicts)
    host_ms = (time.perf_counter() - t0) * 1e3
    recs, marks, sorts = [], [], []
    for step in range(steps + 1):  # (the first round warms the pool up)
        out = bam_records_dev(lib, f._ctx, f.device, Q, C, 1, first, **t)
        total, records = int(out["rep"].bam_bytes), int(out["rep"].records)
        ctx = f._context_to_sort(f._ctx, records)
        got = bam_markdup_dev(lib, ctx, f.device, out["d_bam"], total, out["d_rec_index"], records, 1)
        srt = bam_sort_dev(lib, ctx, f.device, out["d_bam"], total, out["d_rec_index"], records, 1, want_order=False)
        if step == 0:
            assert out["d_bam"][:total].cpu().numpy().tobytes() == want["bam"].tobytes(), "the device marks other records than the model"
            assert np.array_equal(got["d_dup"].cpu().numpy(), want["dup"]), "dup differs from the model"
            assert {k: int(getattr(got["rep"], k)) for k in COUNTS} == want["report"], "the counts differ from the model"
            continue
        recs.append(out["rep"].as_dict())
        marks.append(got["rep"].as_dict())
        sorts.append(srt["rep"].as_dict())
    best = min(marks, key=lambda r: r["ms_total"])
    sort_best = min(r["ms_total"] for r in sorts)
    return {"reads": Q, "bam_bytes": total, **{k: want["report"][k] for k in COUNTS},
            **{"markdup_%s" % k: round(best[k], 4) for k in PHASES},
            **{"markdup_%s_all_steps" % k: rounded(r[k] for r in marks) for k in PHASES},
            "sort_call_ms_total_same_run": round(sort_best, 4), "sort_call_ms_total_all_steps": rounded(r["ms_total"] for r in sorts),
            "markdup_over_sort_call": round(best["ms_total"] / sort_best, 2),
            "records_call_ms_total_same_run": round(min(r["ms_total"] for r in recs), 4), "records_call_ms_total_all_steps": rounded(r["ms_total"] for r in recs),
            "host_alternative": "tests/markdup_model.py (dictionaries for the groups) over the same records; one thread, same process, timed once",
            "host_model_one_thread_ms": round(host_ms, 1), "host_over_device_markdup": round(host_ms / best["ms_total"], 1)}


def planted(flat, per, tenth):
    """rows of `per` bases: every `tenth` row once more, behind the others"""
    rows = flat.reshape(-1, per)
    return np.concatenate((rows, rows[::tenth])).reshape(-1)


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
    line = {"bench": "fm_bam_markdup", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "repeated": "one in ten, once",
            "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    ctx = f._context(max(n + 1, 4 * (3 * max(2 * args.pairs, args.reads) * L + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    rng = np.random.default_rng(5)
    records = dict(ref_names=["dm"], bounds=[0, n])
    for what, paired, Q0 in (("pairs", True, 2 * args.pairs), ("reads", False, args.reads)):
        if not Q0:
            continue
        flat = (cut_pairs(S, n, Q0 // 2, L, args.sub_rate, 400, 50, dev, 3)[0] if paired else cut_reads(S, n, Q0, L, args.sub_rate, dev, 3)).cpu().numpy()
        flat = planted(flat, 2 * L if paired else L, 10)
        Q = flat.size // L
        index = np.arange(0, (Q + 1) * L, L, dtype=np.uint64)
        qual = rng.integers(33, 127, Q * L).astype(np.uint8)
        names = default_names(Q, paired)
        if paired:
            mates = flat.reshape(Q // 2, 2, L)
            res = f.map_pairs((mates[:, 0].reshape(-1), index[:Q // 2 + 1]), (mates[:, 1].reshape(-1), index[:Q // 2 + 1]), S, want_md=True, bam=True,
                              qual=(list(qual.reshape(Q // 2, 2, L)[:, 0]), list(qual.reshape(Q // 2, 2, L)[:, 1])), **records)
        else:
            res = f.map((flat, index), S, both_strands=True, want_md=True, bam=True, qual=qual, **records)
        line[what] = time_markdup(f, res, flat, index, qual, names, paired, args.steps, dev, n)
    f.close()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
