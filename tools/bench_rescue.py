#!/usr/bin/env python3
"""Mate rescue (kiss_hip_fmi_rescue_dev, the align call on the rescue chains, kiss_hip_fmi_aln_merge_dev, then select and pair
once more) after the first pass, in one process, one JSON line: tools/bench_pair.py's workload -- the dm-size text of
bench.py (seed 1), its exact index (SA_INTV = 4), --pairs (5 * 10^4) pairs of --read-len (150) base mates with --sub-rate
(2 %) substitutions, fragments of --frag-mean (400) +- --frag-sd (50), every second pair with its mates swapped -- in which
one mate of every tenth pair carries a substitution every 12th base on top, so that it has no seed.  min_len 19, max_occ 500,
default parameters everywhere.  Everything stays on the device from the reads to the second pair call.
Per step the best ms_total of --steps calls after a warm-up (device events of the reports): plan, the rescue align call with
its cells and cells/s, merge, second select, second pair, beside the first-pass calls of the same run -- boxes differ --; the
proper pairs of either pass, `rescued`, and how many rescued mates lie within 32 bases of where they were cut.
Run it under one `timeout`.  --out FILE: the line as a JSON file (profiles/fm_rescue_dm_size.json).
usage: bench_rescue.py [--n N] [--pairs P] [--read-len L] [--steps K] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import kiss_amd  # noqa: E402
import kiss_amd.fm_index as fm  # noqa: E402
from kiss_amd import _lib, fm_align, fm_chain, fm_pair, fm_rescue, fm_select  # noqa: E402
from bench import DM_N, gen_text_device  # noqa: E402
from bench_align import align_call  # noqa: E402
from bench_chain import chain_call  # noqa: E402
from bench_pair import best_of, cut_pairs, pair_call  # noqa: E402
from bench_seeds import seeds_call  # noqa: E402
from bench_select import select_call  # noqa: E402


def plan_call(f, pairs, hits, hidx, Q, alns, C, d_index, n, params, out, cap):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.RescueReport()
    rc = lib.kiss_hip_fmi_rescue_dev(f._ctx._ctx, vp(pairs.data_ptr()), vp(hits.data_ptr()), vp(hidx.data_ptr()), Q, vp(alns.data_ptr()), C,
                                     vp(d_index.data_ptr()), n, None, 0, ctypes.byref(params), vp(out["chains"].data_ptr()),
                                     vp(out["cidx"].data_ptr()), vp(out["origin"].data_ptr()), cap, ctypes.byref(rep), None)
    return rc, rep.as_dict()


def merge_call(f, a, ia, ca, oa, b, ib, cb, ob, V, out, acap, ocap):
    lib = _lib.load(f._hooks)
    vp = ctypes.c_void_p
    rep = _lib.MergeReport()
    rc = lib.kiss_hip_fmi_aln_merge_dev(f._ctx._ctx, vp(a.data_ptr()), vp(ia.data_ptr()), vp(ca.data_ptr()), vp(oa.data_ptr()),
                                        vp(b.data_ptr()), vp(ib.data_ptr()), vp(cb.data_ptr()), vp(ob.data_ptr()), V,
                                        vp(out["alns"].data_ptr()), acap, vp(out["cidx"].data_ptr()), vp(out["source"].data_ptr()),
                                        vp(out["cigar"].data_ptr()), vp(out["oidx"].data_ptr()), ocap, ctypes.byref(rep), None)
    return rc, rep.as_dict()


def sized_align(f, S, n, reads, d_index, Q, chains, cidx, C, params, dev):
    """the align call's buffers sized by its own reports (cells: a context that holds them; ops) -> out, ocap"""
    out = {"alns": torch.empty((max(C, 1), 12), dtype=torch.int32, device=dev), "cigar": torch.empty(1, dtype=torch.int32, device=dev),
           "oidx": torch.empty(C + 1, dtype=torch.int64, device=dev), "C": C}
    ocap = 0
    rc, rep = align_call(f, S, n, reads, d_index, Q, chains, cidx, params, out, ocap)
    if rc == _lib.KISS_HIP_E_UNSUPPORTED and rep["cells"]:  # a context whose traceback store holds the batch
        f._context(rep["cells"] // fm_align.ALIGN_CELLS_PER_N + (1 << 20))
        rc, rep = align_call(f, S, n, reads, d_index, Q, chains, cidx, params, out, ocap)
    if rc == _lib.KISS_HIP_E_INVALID and rep["cigar_ops"]:
        ocap = rep["cigar_ops"]
        out["cigar"] = torch.empty(ocap, dtype=torch.int32, device=dev)
        rc, rep = align_call(f, S, n, reads, d_index, Q, chains, cidx, params, out, ocap)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_align_dev", f._ctx._ctx)
    return out, ocap


def workload(S, n, P, L, sub_rate, frag_mean, frag_sd, min_len, max_occ, sa_intv, steps, dev):
    f = fm.FMIndex(sa_intv=sa_intv)
    Q = 2 * P
    V = 2 * Q
    bases = 2 * Q * L
    ctx = f._context(max(n + 1, 4 * (bases + 1)))
    SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ctx.suffix_sort_dev(S.data_ptr(), n, SA.data_ptr(), k=kiss_amd.K_UNBOUNDED)
    f.build(S, sa=SA, exact_sa=True)
    del SA
    reads, at, frag, swapped = cut_pairs(S, n, P, L, sub_rate, frag_mean, frag_sd, dev, 3)
    # one mate of every tenth pair -- mate 1 and mate 2 in turns -- gets a substitution every 12th base: no seed of min_len
    hurt_pair = torch.arange(0, P, 10, device=dev)
    hurt_mate = (torch.arange(hurt_pair.numel(), device=dev) & 1)
    hurt_read = 2 * hurt_pair + hurt_mate
    rows = reads.view(Q, L)
    cols = torch.arange(5, L, 12, device=dev)
    rows[hurt_read[:, None], cols[None, :]] = (rows[hurt_read[:, None], cols[None, :]] + 1) & 3
    d_index = torch.arange(0, (Q + 1) * L, L, dtype=torch.int64, device=dev)

    # ---- pass 1, as tools/bench_pair.py ----
    sp = (min_len, 0, max_occ, 1)
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
    CA = int(chain["chains"])
    aparams = fm_align.align_params()
    al1, ocap1 = sized_align(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], CA, aparams, dev)
    align, _ = best_of(steps, lambda: align_call(f, S, n, reads, d_index, Q, ch["chains"], ch["cidx"], aparams, al1, ocap1),
                       "kiss_hip_fmi_align_dev", f)
    sparams = fm_select.select_params()
    hidx = torch.empty(Q + 1, dtype=torch.int64, device=dev)
    hits = torch.empty((max(CA, 1), 8), dtype=torch.int32, device=dev)
    rc, rep = select_call(f, al1["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, CA)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_select_dev", f._ctx._ctx)
    select, _ = best_of(steps, lambda: select_call(f, al1["alns"], ch["cidx"], d_index, Q, sparams, hits, hidx, CA),
                        "kiss_hip_fmi_select_dev", f)
    pparams = fm_pair.pair_params()
    pairs = torch.empty((P, 10), dtype=torch.int32, device=dev)
    rc, rep = pair_call(f, hits, hidx, Q, al1["alns"], CA, pparams, pairs)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_pair_dev", f._ctx._ctx)
    pair, _ = best_of(steps, lambda: pair_call(f, hits, hidx, Q, al1["alns"], CA, pparams, pairs), "kiss_hip_fmi_pair_dev", f)

    # ---- rescue ----
    rparams = fm_rescue.rescue_params(ins_min=pparams.ins_min, ins_max=pparams.ins_max)
    pl = {"chains": torch.empty((1, 6), dtype=torch.int32, device=dev), "cidx": torch.empty(V + 1, dtype=torch.int64, device=dev),
          "origin": torch.empty(1, dtype=torch.int32, device=dev)}
    rc, rep = plan_call(f, pairs, hits, hidx, Q, al1["alns"], CA, d_index, n, rparams, pl, 0)  # warm-up; sizes the chains
    CB = 0
    if rc == _lib.KISS_HIP_E_INVALID and rep["chains"]:
        CB = int(rep["chains"])
        pl["chains"] = torch.empty((CB, 6), dtype=torch.int32, device=dev)
        pl["origin"] = torch.empty(CB, dtype=torch.int32, device=dev)
        rc, rep = plan_call(f, pairs, hits, hidx, Q, al1["alns"], CA, d_index, n, rparams, pl, CB)
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_rescue_dev", f._ctx._ctx)
    plan, plan_runs = best_of(steps, lambda: plan_call(f, pairs, hits, hidx, Q, al1["alns"], CA, d_index, n, rparams, pl, CB),
                              "kiss_hip_fmi_rescue_dev", f)
    al2, ocap2 = sized_align(f, S, n, reads, d_index, Q, pl["chains"], pl["cidx"], CB, aparams, dev)
    ralign, ralign_runs = best_of(steps, lambda: align_call(f, S, n, reads, d_index, Q, pl["chains"], pl["cidx"], aparams, al2, ocap2),
                                  "kiss_hip_fmi_align_dev", f)
    C = CA + CB
    mg = {"alns": torch.empty((max(C, 1), 12), dtype=torch.int32, device=dev), "cidx": torch.empty(V + 1, dtype=torch.int64, device=dev),
          "source": torch.empty(max(C, 1), dtype=torch.int32, device=dev), "cigar": torch.empty(max(ocap1 + ocap2, 1), dtype=torch.int32, device=dev),
          "oidx": torch.empty(C + 1, dtype=torch.int64, device=dev)}
    margs = (f, al1["alns"], ch["cidx"], al1["cigar"], al1["oidx"], al2["alns"], pl["cidx"], al2["cigar"], al2["oidx"], V, mg, C, ocap1 + ocap2)
    rc, rep = merge_call(*margs)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_aln_merge_dev", f._ctx._ctx)
    merge, _ = best_of(steps, lambda: merge_call(*margs), "kiss_hip_fmi_aln_merge_dev", f)

    # ---- pass 2 ----
    if C > 0.3 * f._ctx.max_n:
        f._context(int(3.3 * C) + (1 << 20))
    hidx2 = torch.empty(Q + 1, dtype=torch.int64, device=dev)
    hits2 = torch.empty((max(C, 1), 8), dtype=torch.int32, device=dev)
    rc, rep = select_call(f, mg["alns"], mg["cidx"], d_index, Q, sparams, hits2, hidx2, C)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_select_dev", f._ctx._ctx)
    select2, _ = best_of(steps, lambda: select_call(f, mg["alns"], mg["cidx"], d_index, Q, sparams, hits2, hidx2, C),
                         "kiss_hip_fmi_select_dev", f)
    pairs2 = torch.empty((P, 10), dtype=torch.int32, device=dev)
    rc, rep = pair_call(f, hits2, hidx2, Q, mg["alns"], C, pparams, pairs2)  # warm-up
    kiss_amd.sorter._check(rc, "kiss_hip_fmi_pair_dev", f._ctx._ctx)
    pair2, _ = best_of(steps, lambda: pair_call(f, hits2, hidx2, Q, mg["alns"], C, pparams, pairs2), "kiss_hip_fmi_pair_dev", f)

    # what the second pass says, against where the fragments were cut
    p1, p2 = pairs.to(torch.int64) & 0xFFFFFFFF, pairs2.to(torch.int64) & 0xFFFFFFFF
    proper1, proper2 = (p1[:, 2] & fm_pair.PAIR_PROPER) != 0, (p2[:, 2] & fm_pair.PAIR_PROPER) != 0
    rescued = proper2 & ~proper1
    h64, a64 = hits2.to(torch.int64) & 0xFFFFFFFF, mg["alns"].to(torch.int64) & 0xFFFFFFFF
    src = mg["source"].to(torch.int64) & 0xFFFFFFFF
    # the damaged mate of a damaged pair: cut forward at `at` iff it is mate 1 of a pair that is not swapped, or mate 2 of one that is
    hp = hurt_pair
    its_hit = torch.where(hurt_mate == 1, p2[hp, 1], p2[hp, 0]).clamp(max=max(int(select2["hits"]) - 1, 0))
    its_aln = h64[its_hit, 0].clamp(max=max(C - 1, 0))
    was_forward = (hurt_mate == 1) == swapped[hp]
    true_start = torch.where(was_forward, at[hp], at[hp] + frag[hp] - L)
    near = (a64[its_aln, 4] - true_start).abs() <= 32
    stage = plan["ms_total"] + ralign["ms_total"] + merge["ms_total"] + select2["ms_total"] + pair2["ms_total"]
    per_s = lambda rep: rep["cells"] / (1e-3 * rep["ms_total"]) if rep["ms_total"] > 0 else 0.0  # noqa: E731
    res = {
        "n": n, "pairs": P, "reads": Q, "read_len": L, "sub_rate": sub_rate, "frag_mean": frag_mean, "frag_sd": frag_sd, "min_len": min_len,
        "max_occ": max_occ, "damaged_pairs": int(hp.numel()),
        "first_pass": {"alignments": CA, "hits": select["hits"], "proper": int(proper1.sum()),
                       "damaged_pairs_proper": int(proper1[hp].sum()),
                       "seeds_ms_total": round(seeds["ms_total"], 3), "chain_ms_total": round(chain["ms_total"], 3),
                       "align_ms_total": round(align["ms_total"], 3), "align_cells": align["cells"], "align_cells_per_s": per_s(align),
                       "align_max_band": align["max_band"], "select_ms_total": round(select["ms_total"], 3),
                       "pair_ms_total": round(pair["ms_total"], 3)},
        "plan": {k: plan[k] for k in ("pairs_planned", "anchors", "chains", "split", "empty", "bad_input", "max_chains")},
        "second_pass": {"alignments": C, "hits": select2["hits"], "proper": int(proper2.sum()), "damaged_pairs_proper": int(proper2[hp].sum())},
        "rescued": int(rescued.sum()),
        "rescued_damaged_pairs": int(rescued[hp].sum()),
        "rescued_damaged_mates_within_32_of_their_true_start": int((rescued[hp] & near & (src[its_aln] >= CA)).sum()),
        "ms": {"plan": round(plan["ms_total"], 3), "plan_count": round(plan["ms_count"], 3), "plan_emit": round(plan["ms_emit"], 3),
               "rescue_align": round(ralign["ms_total"], 3), "rescue_align_dp": round(ralign["ms_dp"], 3),
               "rescue_align_trace": round(ralign["ms_trace"], 3), "rescue_align_emit": round(ralign["ms_emit"], 3),
               "merge": round(merge["ms_total"], 3), "second_select": round(select2["ms_total"], 3), "second_pair": round(pair2["ms_total"], 3),
               "rescue_stage": round(stage, 3)},
        "rescue_align_cells": ralign["cells"], "rescue_align_cells_per_s": per_s(ralign), "rescue_align_max_band": ralign["max_band"],
        "rescue_align_too_wide": ralign["too_wide"],
        "rescue_align_ms_total_all_steps": [round(r["ms_total"], 3) for r in ralign_runs],
        "plan_ms_total_all_steps": [round(r["ms_total"], 3) for r in plan_runs],
        "rescue_cells_per_s_over_first_pass": per_s(ralign) / per_s(align) if per_s(align) > 0 else 0.0,
        "rescue_stage_over_first_pass_align_call": stage / align["ms_total"] if align["ms_total"] > 0 else 0.0,
    }
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
    line = {"bench": "fm_rescue", "sa_intv": args.sa_intv, "steps": args.steps, "rescue_params": dict(fm_rescue.RESCUE_DEFAULTS),
            "pair_params": dict(fm_pair.PAIR_DEFAULTS), "select_params": dict(fm_select.SELECT_DEFAULTS),
            "align_params": dict(fm_align.ALIGN_DEFAULTS), "chain_params": dict(fm_chain.CHAIN_DEFAULTS),
            "device": torch.cuda.get_device_name(0)}
    S = gen_text_device(args.n, 1, dev)
    line["dm_size"] = workload(S, args.n, args.pairs, args.read_len, args.sub_rate, args.frag_mean, args.frag_sd, 19, 500, args.sa_intv,
                               args.steps, dev)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as out:
            out.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
