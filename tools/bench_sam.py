#!/usr/bin/env python3
"""The SAM lines written on the device (kiss_hip_fmi_sam_dev) against the host writer of the command line, on ONE batch each:
the dm-size text of bench.py (seed 1), its exact index (SA_INTV = 4), tools/bench_pair.py's --pairs (5 * 10^4) pairs and
tools/bench_select.py's --reads (10^5) single reads of --read-len (150) bases with --sub-rate (2 %) substitutions, with MD and
qualities, default parameters everywhere.  Each batch goes through FMIndex.map / map_pairs once (sam=True: the warm-up of the
writer; the select and align calls' times of that run are recorded beside the writer's); then the returned arrays go back to
the device and the sam call is timed --steps times (device events of the report: ms_total, ms_count, ms_emit; best, and all of
them), and so is the copy of `sam` to pinned host memory.  --dump DIR: the batch as a State file in the format
tests/cli_sam_check.cpp reads, for tools/sam_host_time.cpp, which times the host writer on that same batch; its line (--host
FILE, one per batch, in the order pairs, reads) is merged in.  bytes_to_download_for_host_writer: the records the host writer
needs on the host and the device writer does not.
Run it under one `timeout`.  --out FILE: the JSON (profiles/fm_sam_dm_size.json).
usage: bench_sam.py [--n N] [--pairs P] [--reads Q] [--read-len L] [--steps K] [--dump DIR] [--host FILE] [--out FILE]"""
import argparse
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
from kiss_amd.sam_writer import default_names, pack_names, sam_lines_dev  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_chain import cut_reads  # noqa: E402
from bench_pair import cut_pairs  # noqa: E402


def dump_state(path, res, reads, index, qual, names, paired):
    """one batch in the format of tests/cli_sam_check.cpp"""
    Q, C, H = index.size - 1, res["alignments"].size, res["hits"].size
    text = lambda s: struct.pack("<Q", len(s)) + s  # noqa: E731
    source = res.get("aln_source")
    with open(path, "wb") as o:
        o.write(struct.pack("<10Q", 1, int(paired), 1, 1, int(source is not None), res["first_pass"]["alignments"] if source is not None else 0,
                            0, Q, C, H))
        for part in (index, reads, qual):
            o.write(np.ascontiguousarray(part).tobytes())
        o.write(b"".join(text(x) for x in names))
        o.write(res["alignments"].tobytes() + res["cigar_index"].tobytes() + res["cigar"].tobytes() + res["hits"].tobytes() + res["hit_index"].tobytes())
        if paired:
            o.write(res["pairs"].tobytes())
        if source is not None:
            o.write(np.ascontiguousarray(source, dtype=np.uint32).tobytes())
        o.write(res["md_index"].tobytes() + np.ascontiguousarray(res["md"]).tobytes())
        o.write(struct.pack("<Q", 0))  # (R = 0: bounds is its one entry)


def time_writer(f, res, reads, index, qual, names, paired, steps, dev):
    up = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a).view(t) if t else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    raw, noff, nlen = pack_names(names)
    source = res.get("aln_source")
    t = dict(reads=up(reads), read_index=up(index, np.int64), qual=up(qual), names=up(raw), name_off=up(noff, np.int64), name_len=up(nlen, np.int32),
             alns=up(res["alignments"].view(np.uint32), np.int32), cigar=up(res["cigar"] if res["cigar"].size else np.zeros(1, np.uint32), np.int32),
             cigar_index=up(res["cigar_index"], np.int64), hits=up(res["hits"].view(np.uint32), np.int32), hit_index=up(res["hit_index"], np.int64),
             pairs=up(res["pairs"].view(np.uint32), np.int32) if paired else None,
             source=up(np.ascontiguousarray(source, dtype=np.uint32), np.int32) if source is not None else None,
             md=up(res["md"] if res["md"].size else np.zeros(1, np.uint8)), md_index=up(res["md_index"], np.int64))
    Q, C = index.size - 1, res["alignments"].size
    first = res["first_pass"]["alignments"] if source is not None else 0
    lib = _lib.load(f._hooks)
    runs = []
    for _ in range(steps + 1):  # (the first one warms the pool up)
        out = sam_lines_dev(lib, f._ctx, f.device, Q, C, 0, first, want_line_index=True, **t)
        runs.append(out["rep"].as_dict())
    runs = runs[1:]
    total = int(out["rep"].sam_bytes)
    assert out["d_sam"][:total].cpu().numpy().tobytes() == res["sam"], "the timed call writes other bytes than map(sam=True)"
    host = torch.empty(total, dtype=torch.uint8).pin_memory()
    d2h = []
    for _ in range(steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(out["d_sam"][:total])
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e3)
    d2h = d2h[1:]
    best = min(runs, key=lambda r: r["ms_total"])
    records = sum(res[k].nbytes for k in ("alignments", "cigar", "cigar_index", "hits", "hit_index", "md", "md_index")) + (res["pairs"].nbytes if paired else 0)
    return {"reads": Q, "alignments": C, "hits": int(res["hits"].size), "lines": best["lines"], "sam_bytes": best["sam_bytes"],
            "unmapped_lines": best["unmapped_lines"], "longest": best["longest"], "ms_total": round(best["ms_total"], 3),
            "ms_count": round(best["ms_count"], 3), "ms_emit": round(best["ms_emit"], 3),
            "ms_total_all_steps": [round(r["ms_total"], 3) for r in runs], "bytes_per_s": best["sam_bytes"] / (1e-3 * best["ms_total"]),
            "d2h_sam_ms_best": round(min(d2h), 3), "d2h_sam_ms_all_steps": [round(x, 3) for x in d2h],
            "device_call_plus_d2h_ms": round(best["ms_total"] + min(d2h), 3),
            "select_call_ms_total_same_run": round(res["select_report"]["ms_total"], 3),
            "align_call_ms_total_same_run": round(res["align_report"]["ms_total"], 3), "bytes_to_download_for_host_writer": int(records)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--host", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, L = args.n, args.read_len
    line = {"bench": "fm_sam", "n": n, "read_len": L, "sub_rate": args.sub_rate, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(n, 1, dev)
    f = fm.FMIndex(sa_intv=4)
    ctx = f._context(max(n + 1, 4 * (2 * max(2 * args.pairs, args.reads) * L + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    rng = np.random.default_rng(5)
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
                              qual=(list(qual.reshape(Q // 2, 2, L)[:, 0]), list(qual.reshape(Q // 2, 2, L)[:, 1])))
        else:
            res = f.map((flat, index), S, both_strands=True, want_md=True, sam=True, qual=qual)
        line[what] = time_writer(f, res, flat, index, qual, names, paired, args.steps, dev)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            dump_state(os.path.join(args.dump, what + ".state"), res, flat, index, qual, names, paired)
    f.close()
    if args.host and os.path.exists(args.host):
        with open(args.host) as h:
            for what, text in zip([w for w in ("pairs", "reads") if w in line], h.read().splitlines()):
                line[what]["host_writer"] = json.loads(text)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
