#!/usr/bin/env python3
"""Pairing of mates (kiss_hip_fmi_pair_dev) after the seeds, chain, align and select calls, in one process, one JSON line:
tools/bench_select.py's workload with the reads cut as pairs -- the dm-size text of bench.py (seed 1), its exact index
(SA_INTV = 4), --pairs (5 * 10^4) pairs of --read-len (150) base mates, so as many reads as the earlier benches, with
--sub-rate (2 %) substitutions, fragments of --frag-mean (400) +- --frag-sd (50) bases, mate 2 reverse-complemented, every
second pair with its mates swapped; min_len 19, max_occ 500, both strands, default parameters everywhere.  Reads 2 p and
2 p + 1 of the batch are the mates of pair p.  The reads, the seeds, the chains, the alignments and the hits stay on the device
and go straight into the pair call.
Best ms_total of --steps pair calls after a warm-up (device events of the report) with its phase times, the counts of the
report, what the pairs say against where the fragments were cut, and the select call's time in this same run (best of --steps)
to hold the pair time against -- boxes differ -- beside the seeds, chain and align calls'.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_pair_dm_size.json).
usage: bench_pair.py [--n N] [--pairs P] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain, fm_pair, fm_select  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_align import align_call  # noqa: E402
from bench_chain import chain_call  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402
from bench_select import select_call  # noqa: E402


def pair_call(f, hits, hidx, Q, alns, C, params, pairs):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.PairReport()
    rc = lib.kiss_hip_fmi_pair_dev(f._ctx._ctx, vp(hits.data_ptr()), vp(hidx.data_ptr()), Q, vp(alns.data_ptr()), C, ctypes.byref(params),
                                   vp(pairs.data_ptr()), ctypes.byref(rep), None)
    return rc, rep.as_dict()


def cut_pairs(S, n, P, L, sub_rate, frag_mean, frag_sd, dev, seed):
    """-> the 2 P reads as one flat tensor (read 2 p: mate 1, read 2 p + 1: mate 2), the fragment starts and lengths, and which
    pairs have their mates swapped (mate 1 is then the reverse-complemented one)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    frag = (frag_mean + frag_sd * torch.randn(P, device=dev, generator=g)).round().to(torch.int64).clamp(L, frag_mean + 8 * frag_sd)
    at = torch.randint(0, n - (frag_mean + 8 * frag_sd), (P,), device=dev, generator=g)
    cols = torch.arange(L, device=dev)[None, :]
    left = S[at[:, None] + cols]
    right = 3 - S[(at + frag)[:, None] - 1 - cols]  # the reverse complement of the last L bases of the fragment
    swapped = (torch.arange(P, device=dev) & 1) == 1
    mates = torch.stack([torch.where(swapped[:, None], right, left), torch.where(swapped[:, None], left, right)], dim=1).reshape(2 * P, L)
    sub = torch.rand((2 * P, L), device=dev, generator=g) < sub_rate
    other = (mates + 1 + torch.randint(0, 3, (2 * P, L), device=dev, generator=g).to(torch.uint8)) & 3
    return torch.where(sub, other, mates).contiguous().flatten(), at, frag, swapped


def best_of(steps, call, name, f):
    runs = []
    for _ in range(steps):
        rc, rep = call()
        kiss_amd.sorter._check(rc, name, f._ctx._ctx)
        runs.append(rep)
    return min(runs, key=lambda r: r["ms_total"]), runs


def workload(S, n, P, L, sub_rate, frag_mean, frag_sd, min_len, max_occ, sa_intv, steps, dev, after_pair=None):
    """after_pair(f, state) -> dict: a later stage timed on the buffers of this run (tools/bench_insert.py); its result is merged in"""
    f = fm.FMIndex(sa_intv=sa_intv)
    Q = 2 * P
    bases = 2 * Q * L
    ctx = f._context(max(n + 1, 4 * (bases + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    reads, at, frag, swapped = cut_pairs(S, n, P, L, sub_rate, frag_mean, frag_sd, dev, 3)
    d_index = torch.arange(0, (Q + 1) * L, L, dtype=torch.int64, device=dev)
    sp = (min_len, 0, max_occ, 1)
    V = 2 * Q
    bufs = {"seeds": torch.empty((bases, 4), dtype=torch.int32, device=dev), "sidx": torch.empty(V + 1, dtype=torch.int64, device=dev)}
    first = seeds_call(f, reads, d_index, Q, bases, sp, False, bufs)  # warm-up; sizes the positions
    if first["positions"] > 0.3 * f._ctx.max_n:
        f._context(int(3.3 * first["positions"]) + (1 << 20))
    bufs["pos"] = torch.empty(max(first["positions"], 1), dtype=torch.int32, device=dev)
    bufs["pidx"] = torch.empty(first["seeds"] + 1, dtype=torch.int64, device=dev)
    seeds_call(f, reads, d_index, Q, bases, sp, True, bufs)  # warm-up
    seeds = min((seeds_call(f, reads, d_index, Q, bases, sp, True, bufs) for _ in range(steps)), key=lambda r: r["ms_total"])
    cparams = fm_chain.chain_params()
    ch = {"chains": torch.empty((1, 6), dtype=torch.int32, device=dev), "cidx": torch.empty(V + 1, dtype=torch.int64, device=dev),
          "anc": torch.empty((1, 3), dtype=torch.int32, device=dev), "aidx": torch.empty(2, dtype=torch.int64, device=dev)}
    rc, rep = chain_call(f, bufs, V, cparams, ch)  # warm-up; sizes the output
    if rc == _lib.KISS_HIP_E_INVALID and rep["chains"]:
        ch["chains"] = torch.empty((rep["chains"], 6), dtype=torch.int32, device=dev)
        ch["anc"] = torch.empty((max(rep["chain_anchors"], 1), 3), dtype=torch.int32, device=dev)
        ch["aidx"] = torch.empty(rep["chains"] + 1, dtype=torch.int64, device=dev)
        rc, rep = chain_call(f, bufs, V, cparams, ch)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_chain_dev", f._ctx._ctx)
    chain, _ = best_of(steps, lambda: chain_call(f, bufs, V, cparams, ch), "kiss_hip_fmi_chain_dev", f)
    C = int(chain["chains"])
    aparams = fm_align.align_params()
    out = {"alns": torch.empty((max(C, 1), 12), dtype=torch.int32, device=dev), "cigar": torch.empty(1, dtype=torch.int32, device=dev),
           "oidx": torch.empty(C + 1, dtype=torch.int64, device=dev), "C": C}
    ocap = 0
    rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], aparams, out, ocap)  # sizes the ops
    if rc == _lib.KISS_HIP_E_UNSUPPORTED and rep["cells"]:  # a context whose traceback store holds the batch
        f._context(rep["cells"] // fm_align.ALIGN_CELLS_PER_N + (1 << 20))
        rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], aparams, out, ocap)
    if rc == _lib.KISS_HIP_E_INVALID and rep["cigar_ops"]:
        ocap = rep["cigar_ops"]
        out["cigar"] = torch.empty(ocap, dtype=torch.int32, device=dev)
        rc, rep = align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], aparams, out, ocap)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_align_dev", f._ctx._ctx)
    align, _ = best_of(steps, lambda: align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], aparams, out, ocap),
                       "kiss_hip_fmi_align_dev", f)
    sparams = fm_select.select_params()
    hidx = torch.empty(Q + 1, dtype=torch.int64, device=dev)
    hits = torch.empty((max(C, 1), 8), dtype=torch.int32, device=dev)
    rc, rep = select_call(f, out["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, C)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_select_dev", f._ctx._ctx)
    select, _ = best_of(steps, lambda: select_call(f, out["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, C),
                        "kiss_hip_fmi_select_dev", f)
    pparams = fm_pair.pair_params()
    pairs = torch.empty((P, 10), dtype=torch.int32, device=dev)
    rc, rep = pair_call(f, hits, hidx, Q, out["alns"], C, pparams, pairs)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_pair_dev", f._ctx._ctx)
    best, runs = best_of(steps, lambda: pair_call(f, hits, hidx, Q, out["alns"], C, pparams, pairs), "kiss_hip_fmi_pair_dev", f)
    # what the pairs say, against where the fragments were cut
    pr = pairs.to(torch.int64) & 0xFFFFFFFF
    proper = (pr[:, 2] & fm_pair.PAIR_PROPER) != 0
    h64, a64 = hits.to(torch.int64) & 0xFFFFFFFF, out["alns"].to(torch.int64) & 0xFFFFFFFF
    first_hit = hidx[:-1].reshape(P, 2)
    has = hidx[1:].reshape(P, 2) > first_hit
    own0 = torch.where(has, h64[first_hit.clamp(max=max(int(select["hits"]) - 1, 0)), 2], torch.zeros_like(first_hit))  # select's MAPQ
    fwd_hit = torch.where(swapped, pr[:, 1], pr[:, 0]).clamp(max=max(int(select["hits"]) - 1, 0))  # the mate that was cut forward
    tbeg_fwd = a64[h64[fwd_hit, 0].clamp(max=max(C - 1, 0)), 4]
    res = {
        "n": n, "pairs": P, "reads": Q, "read_len": L, "sub_rate": sub_rate, "frag_mean": frag_mean, "frag_sd": frag_sd, "min_len": min_len,
        "max_occ": max_occ, "alignments": C, "hits": select["hits"], "mapped_reads": select["mapped"],
        "eligible": best["eligible"], "combinations": best["combinations"], "concordant": best["concordant"], "proper": best["proper"],
        "promoted": best["promoted"], "lifted": best["lifted"], "bad_input": best["bad_input"], "max_combinations": best["max_combinations"],
        "proper_at_the_true_start_within_32": int((proper & ((tbeg_fwd - at).abs() <= 32)).sum()),
        "proper_with_tlen_within_64_of_the_fragment": int((proper & ((pr[:, 3] - frag).abs() <= 64)).sum()),
        "mates_with_select_mapq_0": int((has & (own0 == 0)).sum()),
        "mates_with_pair_mapq_0": int(((pr[:, 7:9] == 0) & has).sum()),
        "mates_with_pair_mapq_max": int((pr[:, 7:9] == pparams.mapq_max).sum()),
        "ms_total": round(best["ms_total"], 3), "ms_check": round(best["ms_check"], 3), "ms_pair": round(best["ms_pair"], 3),
        "ms_total_all_steps": [round(r["ms_total"], 3) for r in runs],
        "pairs_per_s": P / (1e-3 * best["ms_total"]) if best["ms_total"] > 0 else 0.0,
        "seeds_call_ms_total_same_run": round(seeds["ms_total"], 3), "chain_call_ms_total_same_run": round(chain["ms_total"], 3),
        "align_call_ms_total_same_run": round(align["ms_total"], 3), "select_call_ms_total_same_run": round(select["ms_total"], 3),
        "pair_over_select_call": best["ms_total"] / select["ms_total"] if select["ms_total"] > 0 else 0.0,
    }
    if after_pair:
        res.update(after_pair(f, dict(hits=hits, hidx=hidx, Q=Q, P=P, alns=out["alns"], C=C, pairs=pairs, frag=frag, steps=steps, dev=dev)))
    f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=DM_N)
    ap.add_argument("--pairs", type=int, default=50_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.02)
    ap.add_argument("--frag-mean", type=int, default=400)
    ap.add_argument("--frag-sd", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sa-intv", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    line = {"bench": "fm_pair", "sa_intv": args.sa_intv, "steps": args.steps, "pair_params": dict(fm_pair.PAIR_DEFAULTS),
            "select_params": dict(fm_select.SELECT_DEFAULTS), "align_params": dict(fm_align.ALIGN_DEFAULTS),
            "chain_params": dict(fm_chain.CHAIN_DEFAULTS), "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(args.n, 1, dev)
    line["dm_size"] = workload(S, args.n, args.pairs, args.read_len, args.sub_rate, args.frag_mean, args.frag_sd, 19, 500, args.sa_intv,
                               args.steps, dev)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
