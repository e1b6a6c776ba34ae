"""The numpy entries of the read-mapping stages without a device and without a built library: kiss_amd._lib.load is replaced by a
stub whose kiss_hip_*_host functions record what they are handed -- the scalars, the bytes of every input array, the fields of
the parameter struct, which output pointers are NULL, the capacities -- and answer as the library would (a call with too little
room: KISS_HIP_E_INVALID and the totals in the report; otherwise a fixed pattern in the outputs and fixed report fields).  The
calls, and the returned dict or the exception, are compared with tests/golden/py_entries_recording.json, which `record()` below
wrote on commit 4b01d7c, where every stage had its own copy of the argument, sizing and record plumbing: what is copied from an
input, what an empty array hands over, how a result is sliced and which of two broken rules is reported is behaviour."""
import contextlib
import ctypes
import inspect
import json
import os

import numpy as np

import kiss_amd
from kiss_amd import _lib, fm_align, fm_chain, fm_insert, fm_md, fm_pair, fm_rescue, fm_sam, fm_select, reads
from kiss_amd.fm_index import FMIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "py_entries_recording.json")
U32 = 0xFFFFFFFF
STAGES = (fm_chain, fm_align, fm_select, fm_pair, fm_rescue, fm_md, fm_insert, fm_sam, reads)
# the record layouts where they are defined, and where the tests of the rescue stage look for them
LAYOUTS = ((fm_chain, ("CHAIN_DTYPE", "ANCHOR_DTYPE", "SEED_DTYPE")), (fm_align, ("ALN_DTYPE",)), (fm_select, ("HIT_DTYPE",)),
           (fm_pair, ("PAIR_DTYPE",)), (fm_rescue, ("CHAIN_DTYPE", "ALN_DTYPE", "HIT_DTYPE", "PAIR_DTYPE")))


# ---- the stub library ------------------------------------------------------------------------------------------------------
def _span(idx):
    return max(int(idx[-1]) - int(idx[0]), 0) if len(idx) else 0


def _asc(idx):
    return bool(np.all(idx[1:] >= idx[:-1]))


def _top(idx):
    return int(idx.max()) if len(idx) else 0


def _V(e):
    return 2 * e.Q if e.both_strands else e.Q


def _H(e):
    """the hits a hit index spans (the wrappers let an index that decreases through: the library flags it)"""
    return int(e.hit_index[-1]) if _asc(e.hit_index) else 0


# per host entry: its arguments in order as (name, kind, element type, count); kind s: scalar, p: parameter struct, r: report,
# i / o: input / output pointer whose count of elements is count(e), e holding the scalars and the inputs read so far (an input
# whose count needs a later one waits for it); then (output, capacity, report field) of what a first call sizes, and the report
# fields that follow from the arguments
S, P, R = (None, None), ("p", None, None), ("report", "r", None, None)
ENTRIES = {
    "kiss_hip_fmi_chain_host": ([
        ("seeds", "i", "u4", lambda e: 4 * _top(e.seed_index)), ("seed_index", "i", "u8", lambda e: e.V + 1), ("V", "s") + S,
        ("positions", "i", "u4", lambda e: _top(e.pos_index)), ("pos_index", "i", "u8", lambda e: _top(e.seed_index) + 1),
        ("params",) + P, ("chains", "o", "u4", lambda e: 6 * e.ccap), ("chain_index", "o", "u8", lambda e: e.V + 1), ("ccap", "s") + S,
        ("anchors", "o", "u4", lambda e: 3 * e.acap), ("anchor_index", "o", "u8", lambda e: e.ccap + 1), ("acap", "s") + S, R,
        ("device", "s") + S],
        [("chains", "ccap", "chains"), ("anchors", "acap", "chain_anchors")], lambda e: {}),
    "kiss_hip_fmi_align_host": ([
        ("text", "i", "u1", lambda e: e.n), ("n", "s") + S, ("reads", "i", "u1", lambda e: _top(e.read_index)),
        ("read_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S, ("both_strands", "s") + S,
        ("chains", "i", "u4", lambda e: 6 * _top(e.chain_index)), ("chain_index", "i", "u8", lambda e: _V(e) + 1), ("params",) + P,
        ("alignments", "o", "u4", lambda e: 12 * e.C), ("C", "s") + S, ("cigar", "o", "u4", lambda e: e.ocap),
        ("cigar_index", "o", "u8", lambda e: e.C + 1), ("ocap", "s") + S, R, ("device", "s") + S],
        [("cigar", "ocap", "cigar_ops")], lambda e: {}),
    "kiss_hip_fmi_select_host": ([
        ("alignments", "i", "u4", lambda e: 12 * _span(e.chain_index)), ("chain_index", "i", "u8", lambda e: _V(e) + 1),
        ("read_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S, ("both_strands", "s") + S,
        ("bounds", "i", "u8", lambda e: e.R + 1), ("R", "s") + S, ("params",) + P, ("hits", "o", "u4", lambda e: 8 * e.cap),
        ("hit_index", "o", "u8", lambda e: e.Q + 1), ("cap", "s") + S, R, ("device", "s") + S],
        [], lambda e: {"hits": min(e.cap, 2)}),
    "kiss_hip_fmi_pair_host": ([
        ("hits", "i", "u4", lambda e: 8 * _H(e)), ("hit_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S,
        ("alignments", "i", "u4", lambda e: 12 * e.aln_count), ("aln_count", "s") + S, ("params",) + P,
        ("pairs", "o", "u4", lambda e: 10 * (e.Q // 2)), R, ("device", "s") + S],
        [], lambda e: {"P": e.Q // 2}),
    "kiss_hip_fmi_rescue_host": ([
        ("pairs", "i", "u4", lambda e: 10 * (e.Q // 2)), ("hits", "i", "u4", lambda e: 8 * _H(e)),
        ("hit_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S, ("alignments", "i", "u4", lambda e: 12 * e.aln_count),
        ("aln_count", "s") + S, ("read_index", "i", "u8", lambda e: e.Q + 1), ("n", "s") + S,
        ("bounds", "i", "u8", lambda e: e.R + 1), ("R", "s") + S, ("params",) + P, ("chains", "o", "u4", lambda e: 6 * e.cap),
        ("chain_index", "o", "u8", lambda e: 2 * e.Q + 1), ("origin", "o", "u4", lambda e: e.cap), ("cap", "s") + S, R,
        ("device", "s") + S],
        [("chains", "cap", "chains")], lambda e: {}),
    "kiss_hip_fmi_aln_merge_host": ([
        ("alignments_a", "i", "u4", lambda e: 12 * _span(e.chain_index_a)), ("chain_index_a", "i", "u8", lambda e: e.V + 1),
        ("cigar_a", "i", "u4", lambda e: _top(e.cigar_index_a)), ("cigar_index_a", "i", "u8", lambda e: _span(e.chain_index_a) + 1),
        ("alignments_b", "i", "u4", lambda e: 12 * _span(e.chain_index_b)), ("chain_index_b", "i", "u8", lambda e: e.V + 1),
        ("cigar_b", "i", "u4", lambda e: _top(e.cigar_index_b)), ("cigar_index_b", "i", "u8", lambda e: _span(e.chain_index_b) + 1),
        ("V", "s") + S, ("alignments", "o", "u4", lambda e: 12 * e.C), ("C", "s") + S, ("chain_index", "o", "u8", lambda e: e.V + 1),
        ("source", "o", "u4", lambda e: e.C), ("cigar", "o", "u4", lambda e: e.ops), ("cigar_index", "o", "u8", lambda e: e.C + 1),
        ("ops", "s") + S, R, ("device", "s") + S],
        [], lambda e: {"cigar_ops": e.ops, "alignments": e.C}),
    "kiss_hip_fmi_md_host": ([
        ("text", "i", "u1", lambda e: e.n), ("n", "s") + S, ("reads", "i", "u1", lambda e: _top(e.read_index)),
        ("read_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S, ("both_strands", "s") + S,
        ("alignments", "i", "u4", lambda e: 12 * (_span(e.chain_index) if _asc(e.chain_index) else 0)),
        ("chain_index", "i", "u8", lambda e: _V(e) + 1), ("cigar", "i", "u4", lambda e: _top(e.cigar_index)),
        ("cigar_index", "i", "u8", lambda e: (_span(e.chain_index) if _asc(e.chain_index) else 0) + 1),
        ("hits", "i", "u4", lambda e: 8 * e.H), ("H", "s") + S, ("md", "o", "u1", lambda e: e.cap),
        ("md_index", "o", "u8", lambda e: e.items + 1), ("md_counts", "o", "u4", lambda e: 2 * e.items), ("cap", "s") + S, R,
        ("device", "s") + S],
        [("md", "cap", "md_bytes")], lambda e: {}),
    "kiss_hip_fmi_insert_host": ([
        ("hits", "i", "u4", lambda e: 8 * _H(e)), ("hit_index", "i", "u8", lambda e: e.Q + 1), ("Q", "s") + S,
        ("alignments", "i", "u4", lambda e: 12 * e.aln_count), ("aln_count", "s") + S, ("params",) + P,
        ("hist", "o", "u4", lambda e: e.params["max_insert"] + 1), R, ("device", "s") + S],
        [], lambda e: {}),
    "kiss_hip_reads_interleave_host": ([
        ("reads_a", "i", "u1", lambda e: int(e.index_a[-1])), ("index_a", "i", "u8", lambda e: e.Pa + 1),
        ("qual_a", "i", "u1", lambda e: int(e.index_a[-1])), ("Pa", "s") + S, ("reads_b", "i", "u1", lambda e: int(e.index_b[-1])),
        ("index_b", "i", "u8", lambda e: e.Pb + 1), ("qual_b", "i", "u1", lambda e: int(e.index_b[-1])), ("Pb", "s") + S,
        ("reads", "o", "u1", lambda e: e.total), ("read_index", "o", "u8", lambda e: e.Pa + e.Pb + 1),
        ("qual", "o", "u1", lambda e: e.total), ("total", "s") + S, ("got", "r", None, None), ("device", "s") + S],
        [], lambda e: {}),
}
TOTALS = {"chains": 3, "chain_anchors": 5, "cigar_ops": 4, "md_bytes": 7}


class Env:
    pass


class Stub:
    """what _lib.load returns: totals -- what the sized entries answer a first call with; rc -- a status to fail with"""

    def __init__(self, totals=None, rc=None):
        self.calls, self.totals, self.rc = [], dict(TOTALS, **(totals or {})), rc

    @staticmethod
    def kiss_hip_strerror(status):
        return b"status %d of the stub" % status

    def __getattr__(self, name):
        if name not in ENTRIES:
            raise AttributeError(name)
        return lambda *args: self._call(name, *args)

    def _call(self, name, *args):
        table, sizing, follows = ENTRIES[name]
        assert len(args) == len(table), (name, len(args))
        e, rec = Env(), {"entry": name, "scalars": {}, "in": {}, "out_null": {}}
        addr, rep = {}, None
        for (arg, kind, _, _), a in zip(table, args):
            a = getattr(a, "_obj", a)  # (byref)
            if kind == "s":
                rec["scalars"][arg] = int(a)
                setattr(e, arg, int(a))
            elif kind == "p":
                e.params = rec["params"] = {k: int(getattr(a, k)) for k, _ in a._fields_}
            elif kind == "r":
                rep = a
            else:
                addr[arg] = (a.value if isinstance(a, ctypes.c_void_p) else a) or None
        if name == "kiss_hip_fmi_md_host":
            cidx = np.frombuffer(ctypes.string_at(addr["chain_index"], 8 * (_V(e) + 1)), "u8")
            e.items = e.H if addr["hits"] else _span(cidx) if _asc(cidx) else 0
        waiting = [t for t in table if t[1] == "i"]
        while waiting:
            before = len(waiting)
            for t in list(waiting):
                arg, _, dtype, count = t
                if addr[arg] is None:
                    got = None
                else:
                    try:
                        got = np.frombuffer(ctypes.string_at(addr[arg], count(e) * np.dtype(dtype).itemsize), dtype)
                    except AttributeError:
                        continue
                setattr(e, arg, got if got is not None else np.zeros(0, dtype))
                rec["in"][arg] = None if got is None else got.tolist()
                waiting.remove(t)
            assert len(waiting) < before, (name, [t[0] for t in waiting])
        rec["out_null"] = {t[0]: addr[t[0]] is None for t in table if t[1] == "o"}
        if isinstance(rep, ctypes.Structure):
            for i, (k, t) in enumerate(rep._fields_):
                if not k.startswith("reserved"):
                    setattr(rep, k, 0.25 * (i + 1) if t is ctypes.c_float else i + 1)
            for _, _, field in sizing:
                setattr(rep, field, self.totals[field])
            for k, v in follows(e).items():
                setattr(rep, k, v)
        short = [out for out, cap, field in sizing if addr[out] is not None and getattr(e, cap) < self.totals[field]]
        if self.rc is not None:
            rc = self.rc
        elif short:
            rc = _lib.KISS_HIP_E_INVALID
        else:
            rc = _lib.KISS_HIP_OK
            for j, (arg, kind, dtype, count) in enumerate(table):
                if kind == "o" and addr[arg] is not None:
                    fill = ((np.arange(count(e)) * 3 + 17 * j + 1) & 0x7F).astype(dtype)
                    ctypes.memmove(addr[arg], fill.tobytes(), fill.nbytes)
        rec["rc"] = rc
        self.calls.append(rec)
        return rc


@contextlib.contextmanager
def stubbed(stub):
    real = _lib.load
    _lib.load = lambda hooks=None: stub
    try:
        yield stub
    finally:
        _lib.load = real


# ---- the cases -------------------------------------------------------------------------------------------------------------
LIMITS = {
    "chain": (fm_chain.chain_params, dict(max_gap=0x7FFFFFFF, band=0x7FFFFFFF, gap_cost=65535, max_lookback=U32, min_score=U32)),
    "align": (fm_align.align_params, dict(match=65535, mismatch=65535, gap_open=65535, gap_extend=65535, band=0x7FFFFFFF)),
    "select": (fm_select.select_params, dict(min_score=U32, overlap=256, mapq_coef=65535, mapq_max=255, max_hits=U32)),
    "pair": (fm_pair.pair_params, dict(ins_min=U32, ins_max=U32, ins_mean=U32, pen_coef=65535, pen_max=65535, mapq_coef=65535,
                                       mapq_max=255)),
    "rescue": (fm_rescue.rescue_params, dict(ins_min=U32, ins_max=U32, max_anchors=U32, min_anchor_score=U32, max_width=1024)),
    "insert": (fm_insert.insert_params, dict(min_mapq=U32, max_insert=65535, min_samples=U32, out_mult=255, map_mult=255,
                                             sd_mult=255)),
}
TWO_RULES = {
    "chain": [dict(max_gap=-1, bogus=1), dict(bogus=1, max_gap=-1), dict(band=1 << 31, min_score=-1), dict(gap_cost=65536, max_gap=1 << 32),
              dict(max_gap="x", bogus=1), dict(max_gap=1 << 31, gap_cost=65536)],
    "align": [dict(match=0, bogus=1), dict(match=0, band=-1), dict(match=0, mismatch=65536), dict(band=1 << 31, gap_open=1 << 32),
              dict(gap_extend="1", band="2")],
    "select": [dict(overlap=257, mapq_max=256), dict(mapq_max=256, mapq_coef=65536), dict(overlap=257, max_hits=-1),
               dict(nothing=0, overlap=257), dict(overlap=257, min_score=1 << 32)],
    "pair": [dict(pen_coef=65536, ins_min=2000), dict(mapq_max=256, pen_max=65536), dict(ins_min=5, ins_max=4, mapq_max=256),
             dict(ins_min=-1, ins_max=-2), dict(ins_min=2000, wrong=1), dict(ins_min=1000, ins_max=1000)],
    "rescue": [dict(ins_min=2, ins_max=1, max_anchors=0), dict(max_anchors=0, max_width=0), dict(max_width=1025, ins_min=2000),
               dict(max_width=0), dict(max_width=1025, max_anchors=-1), dict(max_anchors=0, extra=3)],
    "insert": [dict(max_insert=65536, out_mult=256), dict(max_insert=0, sd_mult=256), dict(max_insert=0), dict(map_mult=256, min_mapq=-1),
               dict(sd_mult=256, map_mult=256, out_mult=256), dict(max_insert=0, other=1)],
}


def param_cases():
    """every key at its limit, one past it and negative; an unknown key; two broken rules at once"""
    for kind, (build, limits) in LIMITS.items():
        yield "params/%s/defaults" % kind, build, {}
        yield "params/%s/unknown" % kind, build, {"no_such_key": 1}
        for k, top in limits.items():
            yield "params/%s/%s=limit" % (kind, k), build, {k: top}
            yield "params/%s/%s=limit+1" % (kind, k), build, {k: top + 1}
            yield "params/%s/%s=-1" % (kind, k), build, {k: -1}
        for j, kw in enumerate(TWO_RULES[kind]):
            yield "params/%s/two%d" % (kind, j), build, kw


def _data():
    d = Env()
    d.text = np.array([0, 1, 2, 3] * 4, np.uint8)
    d.rlist = [np.array([0, 1, 2, 3, 0], np.uint8), [3, 3, 1]]
    d.rtuple = (np.array([0, 1, 2, 3, 0, 3, 3, 1], np.uint8), np.array([0, 5, 8]))
    d.seeds = np.zeros(3, fm_chain.SEED_DTYPE)
    d.seeds["start"], d.seeds["len"], d.seeds["sa_beg"], d.seeds["sa_end"] = [0, 2, 1], [3, 3, 2], [7, 8, 9], [8, 10, 10]
    d.seed_rows = [[0, 3], [2, 3], [1, 2]]
    d.seed_index, d.positions, d.pos_index = [0, 2, 3], [5, 9, 20, 31], [0, 1, 3, 4]
    d.chain_rows = np.arange(18).reshape(3, 6) + 2
    d.chains = np.ascontiguousarray(d.chain_rows.astype(np.uint32)).view(fm_chain.CHAIN_DTYPE).reshape(3)
    d.quads = d.chain_rows[:, 2:].copy()
    d.cidx, d.cidx2, d.cidx_off = [0, 2, 3], [0, 1, 2, 2, 3], [1, 3, 4]
    d.aln_rows = np.arange(36).reshape(3, 12) + 1
    d.alns = np.ascontiguousarray(d.aln_rows.astype(np.uint32)).view(fm_align.ALN_DTYPE).reshape(3)
    d.wide = np.zeros(3, [(k, np.uint64) for k in fm_align.ALN_FIELDS[::-1]] + [("more", np.uint8)])  # (other types, order, a field more)
    for j, k in enumerate(fm_align.ALN_FIELDS):
        d.wide[k] = d.aln_rows[:, j]
    d.cigar, d.oidx = [80, 33, 48, 48], [0, 2, 3, 4]
    d.hit_rows = np.arange(24).reshape(3, 8) % 3
    d.hits = np.ascontiguousarray(d.hit_rows.astype(np.uint32)).view(fm_select.HIT_DTYPE).reshape(3)
    d.hidx = [0, 2, 3]
    d.pair_rows = np.arange(10).reshape(1, 10)
    d.pairs = np.ascontiguousarray(d.pair_rows.astype(np.uint32)).view(fm_pair.PAIR_DTYPE).reshape(1)
    d.none = np.zeros((0, 12), np.int64)
    return d


def entry_cases():
    """(name, function, args, kwargs, stub settings)"""
    d = _data()
    ok0 = {"totals": {k: 0 for k in TOTALS}}  # (the first call already returns OK)
    neg, big = [[0, -1]], [[1 << 32, 0]]
    f = fm_chain.chain_seeds
    base = (d.seeds, d.seed_index, d.positions, d.pos_index)
    yield "chain/structured", f, base, {}, {}
    yield "chain/rows", f, (d.seed_rows,) + base[1:], {}, {}
    yield "chain/rows-array-params", f, (np.array(d.seed_rows, np.uint16),) + base[1:], dict(max_gap=100, min_score=1, device=2), {}
    yield "chain/no-anchors", f, base, dict(want_anchors=False), {}
    yield "chain/ok-first", f, base, {}, ok0
    yield "chain/ok-first-no-anchors", f, base, dict(want_anchors=False), ok0
    yield "chain/no-anchors-at-all", f, base, {}, {"totals": {"chain_anchors": 0}}
    yield "chain/empty-batch", f, ([], [0], [], [0]), {}, ok0
    yield "chain/empty-batch-sized", f, (np.zeros(0, fm_chain.SEED_DTYPE), [0], [], [0]), {}, {}
    yield "chain/empty-seeds", f, (np.zeros((0, 2)), [0, 0, 0], [], [0]), {}, ok0
    yield "chain/no-positions", f, (d.seeds, d.seed_index, [], [0, 0, 0, 0]), {}, {}
    yield "chain/unsupported", f, base, {}, {"rc": _lib.KISS_HIP_E_UNSUPPORTED}
    yield "chain/fails", f, base, {}, {"rc": _lib.KISS_HIP_E_NOMEM}
    yield "chain/bad-rows-negative", f, (neg,) + base[1:], {}, {}
    yield "chain/bad-rows-big", f, (big,) + base[1:], {}, {}
    yield "chain/bad-seed-index-2d", f, (d.seeds, [[0, 2, 3]], d.positions, d.pos_index), {}, {}
    yield "chain/bad-seed-index-empty", f, (d.seeds, [], d.positions, d.pos_index), {}, {}
    yield "chain/bad-pos-index-2d", f, (d.seeds, d.seed_index, d.positions, [d.pos_index]), {}, {}
    yield "chain/bad-seed-index-past", f, (d.seeds, [0, 2, 4], d.positions, d.pos_index), {}, {}
    yield "chain/bad-pos-index-short", f, (d.seeds, d.seed_index, d.positions, [0, 1, 3]), {}, {}
    yield "chain/bad-pos-index-past", f, (d.seeds, d.seed_index, d.positions, [0, 1, 3, 5]), {}, {}
    yield "chain/bad-param-and-rows", f, (neg,) + base[1:], dict(gap_cost=65536), {}
    yield "chain/bad-rows-and-index", f, (neg, [], d.positions, d.pos_index), {}, {}
    yield "chain/bad-unknown-and-index", f, (d.seeds, [], d.positions, d.pos_index), dict(bogus=1), {}

    f = fm_align.align_chains
    yield "align/structured-list", f, (d.text, d.rlist, d.chains, d.cidx), {}, {}
    yield "align/quads-tuple", f, (d.text, d.rtuple, d.quads, d.cidx), {}, {}
    yield "align/quads-list-of-lists", f, (d.text.tolist(), d.rlist, d.quads.tolist(), d.cidx), dict(band=8, match=2, device=1), {}
    yield "align/both-strands", f, (d.text, d.rlist, d.chains, d.cidx2), dict(both_strands=True), {}
    yield "align/no-cigar", f, (d.text, d.rtuple, d.chains, d.cidx), dict(want_cigar=False), {}
    yield "align/ok-first", f, (d.text, d.rlist, d.chains, d.cidx), {}, ok0
    yield "align/index-from-1", f, (d.text, d.rlist, d.chains, [1, 2, 3]), {}, {}
    yield "align/index-descends", f, (d.text, d.rlist, d.chains, [3, 2, 1]), {}, {}
    yield "align/empty-batch", f, ([], [], np.zeros((0, 4)), [0]), {}, ok0
    yield "align/empty-batch-tuple", f, ([], ([], [0]), np.zeros(0, fm_chain.CHAIN_DTYPE), [0]), dict(want_cigar=False), {}
    yield "align/empty-text", f, ([], d.rlist, d.chains, d.cidx), {}, {}
    yield "align/empty-chains", f, (d.text, d.rlist, [], [0, 0, 0]), {}, ok0
    yield "align/text-2d", f, (d.text.reshape(4, 4), d.rlist, d.chains, d.cidx), {}, {}
    yield "align/unsupported", f, (d.text, d.rlist, d.chains, d.cidx), {}, {"rc": _lib.KISS_HIP_E_UNSUPPORTED}
    yield "align/bad-quads-negative", f, (d.text, d.rlist, [[0, 1, 2, -3]], d.cidx), {}, {}
    yield "align/bad-quads-big", f, (d.text, d.rlist, [[0, 1, 2, 1 << 32]], d.cidx), {}, {}
    yield "align/bad-read-index-2d", f, (d.text, (d.rtuple[0], [[0, 5, 8]]), d.chains, d.cidx), {}, {}
    yield "align/bad-read-index-empty", f, (d.text, (d.rtuple[0], []), d.chains, d.cidx), {}, {}
    yield "align/bad-chain-index-2d", f, (d.text, d.rlist, d.chains, [d.cidx]), {}, {}
    yield "align/bad-chain-index-size", f, (d.text, d.rlist, d.chains, d.cidx2), {}, {}
    yield "align/bad-chain-index-size-both", f, (d.text, d.rlist, d.chains, d.cidx), dict(both_strands=True), {}
    yield "align/bad-read-index-past", f, (d.text, (d.rtuple[0], [0, 5, 9]), d.chains, d.cidx), {}, {}
    yield "align/bad-chain-index-past", f, (d.text, d.rlist, d.chains, [0, 2, 4]), {}, {}
    yield "align/bad-param-and-quads", f, (d.text, d.rlist, [[0, 1, 2, -3]], d.cidx), dict(match=0), {}
    yield "align/bad-quads-and-index", f, (d.text, d.rlist, [[0, 1, 2, -3]], d.cidx2), {}, {}
    yield "align/bad-size-and-past", f, (d.text, (d.rtuple[0], [0, 5, 9]), d.chains, d.cidx2), {}, {}

    f = fm_select.select_alignments
    yield "select/structured-lengths", f, (d.alns, d.cidx, [5, 3]), {}, {}
    yield "select/rows-index", f, (d.aln_rows, d.cidx, ("index", [0, 5, 8])), {}, {}
    yield "select/wide-structured", f, (d.wide, d.cidx, [5, 3]), {}, {}
    yield "select/rows-list-params", f, (d.aln_rows.tolist(), d.cidx, np.array([5, 3], np.int32)), dict(min_score=10, max_hits=2, device=3), {}
    yield "select/both-strands", f, (d.alns, d.cidx2, [5, 3]), dict(both_strands=True), {}
    yield "select/bounds", f, (d.alns, d.cidx, [5, 3]), dict(bounds=[0, 8, 16]), {}
    yield "select/bounds-2d", f, (d.alns, d.cidx, [5, 3]), dict(bounds=np.array([[0, 8], [12, 16]])), {}
    yield "select/index-from-1", f, (np.concatenate([d.alns, d.alns]), d.cidx_off, ("index", [2, 7, 10])), {}, {}
    yield "select/index-descends", f, (d.alns, [3, 2, 1], [5, 3]), {}, {}
    yield "select/more-alignments-than-spanned", f, (d.alns, [0, 1, 1], [5, 3]), {}, {}
    yield "select/empty-batch", f, (d.none, [0], []), {}, {}
    yield "select/empty-batch-structured", f, (d.alns[:0], [0], ("index", [0])), dict(bounds=[0, 16]), {}
    yield "select/empty-alignments", f, ([], [0, 0, 0], [5, 3]), {}, {}
    yield "select/fails", f, (d.alns, d.cidx, [5, 3]), {}, {"rc": _lib.KISS_HIP_E_HIP}
    yield "select/bad-rows-negative", f, (-d.aln_rows, d.cidx, [5, 3]), {}, {}
    yield "select/bad-rows-big", f, (d.aln_rows << 30, d.cidx, [5, 3]), {}, {}
    yield "select/bad-tuple", f, (d.alns, d.cidx, ("lengths", [5, 3])), {}, {}
    yield "select/bad-read-index-empty", f, (d.alns, d.cidx, ("index", [])), {}, {}
    yield "select/bad-chain-index-size", f, (d.alns, d.cidx2, [5, 3]), {}, {}
    yield "select/bad-chain-index-spans", f, (d.alns, [0, 2, 4], [5, 3]), {}, {}
    yield "select/bad-bounds-short", f, (d.alns, d.cidx, [5, 3]), dict(bounds=[0]), {}
    yield "select/bad-bounds-start", f, (d.alns, d.cidx, [5, 3]), dict(bounds=[1, 16]), {}
    yield "select/bad-bounds-order", f, (d.alns, d.cidx, [5, 3]), dict(bounds=[0, 8, 8]), {}
    yield "select/bad-param-and-rows", f, (-d.aln_rows, d.cidx, [5, 3]), dict(overlap=257), {}
    yield "select/bad-rows-and-tuple", f, (-d.aln_rows, d.cidx, ("lengths", [5, 3])), {}, {}
    yield "select/bad-tuple-and-size", f, (d.alns, d.cidx2, ("lengths", [5, 3])), {}, {}
    yield "select/bad-spans-and-bounds", f, (d.alns, [0, 2, 4], [5, 3]), dict(bounds=[0]), {}

    for tag, f, kw in (("pair", fm_pair.pair_hits, {}), ("insert", fm_insert.estimate_insert, dict(max_insert=8))):
        yield tag + "/structured", f, (d.hits, d.hidx, d.alns), kw, {}
        yield tag + "/rows", f, (d.hit_rows, d.hidx, d.aln_rows), kw, {}
        yield tag + "/mixed-params", f, (d.hit_rows.tolist(), np.array(d.hidx, np.int16), d.wide), dict(kw, device=1, **(
            dict(ins_max=500, mapq_max=40) if tag == "pair" else dict(min_mapq=0, sd_mult=3))), {}
        yield tag + "/four-reads", f, (d.hits, [0, 1, 1, 2, 3], d.alns), kw, {}
        yield tag + "/index-descends", f, (d.hits, [0, 9, 3], d.alns), kw, {}
        yield tag + "/empty-batch", f, ([], [0], []), kw, {}
        yield tag + "/empty-records", f, (d.hits[:0], [0, 0, 0], d.none), kw, {}
        yield tag + "/fails", f, (d.hits, d.hidx, d.alns), kw, {"rc": _lib.KISS_HIP_E_INTERNAL}
        yield tag + "/bad-hits", f, (-d.hit_rows, d.hidx, d.alns), kw, {}
        yield tag + "/bad-alignments", f, (d.hits, d.hidx, d.aln_rows << 30), kw, {}
        yield tag + "/bad-index-empty", f, (d.hits, [], d.alns), kw, {}
        yield tag + "/bad-odd", f, (d.hits, [0, 3], d.alns), kw, {}
        yield tag + "/bad-spans", f, (d.hits, [0, 2, 4], d.alns), kw, {}
        yield tag + "/bad-param-and-hits", f, (-d.hit_rows, d.hidx, d.alns), dict(mapq_max=256) if tag == "pair" else dict(max_insert=0), {}
        yield tag + "/bad-both-records", f, (-d.hit_rows, d.hidx, -d.aln_rows), kw, {}
        yield tag + "/bad-alignments-and-odd", f, (d.hits, [0, 3], -d.aln_rows), kw, {}
        yield tag + "/bad-odd-and-spans", f, (d.hits, [0, 1, 2, 4], d.alns), kw, {}

    f = fm_rescue.plan_rescue
    base = (d.pairs, d.hits, d.hidx, d.alns, [5, 3], 16)
    yield "rescue/structured", f, base, {}, {}
    yield "rescue/rows", f, (d.pair_rows, d.hit_rows, d.hidx, d.aln_rows, np.array([5, 3]), 16.0), {}, {}
    yield "rescue/bounds-params", f, base, dict(bounds=[0, 8, 16], ins_max=300, max_width=64, device=1), {}
    yield "rescue/ok-first", f, base, {}, ok0
    yield "rescue/more-pairs", f, (np.concatenate([d.pairs, d.pairs]),) + base[1:], {}, {}
    yield "rescue/index-descends", f, (d.pairs, d.hits, [0, 9, 3]) + base[3:], {}, {}
    yield "rescue/empty-batch", f, ([], [], [0], [], [], 0), {}, ok0
    yield "rescue/empty-batch-sized", f, (d.pairs[:0], d.hits[:0], [0], d.none, [], 16), {}, {}
    yield "rescue/empty-records", f, (d.pairs, [], [0, 0, 0], [], [5, 3], 16), {}, ok0
    yield "rescue/fails", f, base, {}, {"rc": _lib.KISS_HIP_E_NOMEM}
    yield "rescue/bad-pairs", f, (-d.pair_rows - 1,) + base[1:], {}, {}
    yield "rescue/bad-hits", f, (d.pairs, d.hit_rows << 32) + base[2:], {}, {}
    yield "rescue/bad-alignments", f, (d.pairs, d.hits, d.hidx, -d.aln_rows, [5, 3], 16), {}, {}
    yield "rescue/bad-index-size", f, (d.pairs, d.hits, [0, 3]) + base[3:], {}, {}
    yield "rescue/bad-odd", f, (d.pairs, d.hits, [0, 1, 2, 3], d.alns, [5, 3, 4], 16), {}, {}
    yield "rescue/bad-few-pairs", f, (d.pairs[:0],) + base[1:], {}, {}
    yield "rescue/bad-spans", f, (d.pairs, d.hits, [0, 2, 4]) + base[3:], {}, {}
    yield "rescue/bad-bounds", f, base, dict(bounds=[0, 0]), {}
    yield "rescue/bad-param-and-pairs", f, (-d.pair_rows - 1,) + base[1:], dict(max_anchors=0), {}
    yield "rescue/bad-pairs-and-hits", f, (-d.pair_rows - 1, -d.hit_rows - 1) + base[2:], {}, {}
    yield "rescue/bad-size-and-odd", f, (d.pairs, d.hits, [0, 3], d.alns, [5, 3, 4], 16), {}, {}
    yield "rescue/bad-few-pairs-and-spans", f, (d.pairs[:0], d.hits, [0, 2, 4]) + base[3:], {}, {}
    yield "rescue/bad-spans-and-bounds", f, (d.pairs, d.hits, [0, 2, 4]) + base[3:], dict(bounds=[0, 0]), {}

    f = fm_rescue.merge_alignments
    ops = dict(cigar_a=d.cigar, cigar_index_a=d.oidx, cigar_b=[16, 32], cigar_index_b=[0, 1, 2])
    yield "merge/no-ops", f, (d.alns, d.cidx, d.aln_rows[:2], [0, 0, 2]), {}, {}
    yield "merge/ops", f, (d.alns, d.cidx, d.aln_rows[:2], [0, 0, 2]), dict(ops, device=1), {}
    yield "merge/ops-index-from-1", f, (np.concatenate([d.alns, d.alns]), d.cidx_off, d.alns[:2], [0, 0, 2]), dict(ops, cigar_index_a=[1, 2, 3, 4]), {}
    yield "merge/empty-a", f, ([], [0, 0, 0], d.alns, d.cidx), {}, {}
    yield "merge/empty-a-ops", f, (d.none, [0, 0, 0], d.alns, d.cidx), dict(cigar_a=[], cigar_index_a=[0], cigar_b=d.cigar, cigar_index_b=d.oidx), {}
    yield "merge/empty-batch", f, ([], [0], [], [0]), {}, {}
    yield "merge/empty-batch-ops", f, ([], [0], [], [0]), dict(cigar_a=[], cigar_index_a=[0], cigar_b=[], cigar_index_b=[0]), {}
    yield "merge/fails", f, (d.alns, d.cidx, d.aln_rows[:2], [0, 0, 2]), {}, {"rc": _lib.KISS_HIP_E_INVALID}
    yield "merge/bad-a", f, (-d.aln_rows, d.cidx, d.alns, d.cidx), {}, {}
    yield "merge/bad-b", f, (d.alns, d.cidx, -d.aln_rows, d.cidx), {}, {}
    yield "merge/bad-index-sizes", f, (d.alns, d.cidx, d.alns, d.cidx2), {}, {}
    yield "merge/bad-index-empty", f, (d.alns, [], d.alns, []), {}, {}
    yield "merge/bad-some-ops", f, (d.alns, d.cidx, d.alns, d.cidx), dict(cigar_a=d.cigar, cigar_index_a=d.oidx), {}
    yield "merge/bad-spans", f, (d.alns, d.cidx, d.alns[:2], d.cidx), {}, {}
    yield "merge/bad-cigar-index-short", f, (d.alns, d.cidx, d.aln_rows[:2], [0, 0, 2]), dict(ops, cigar_index_a=[0, 2, 3]), {}
    yield "merge/bad-cigar-index-past", f, (d.alns, d.cidx, d.aln_rows[:2], [0, 0, 2]), dict(ops, cigar_index_b=[0, 1, 3]), {}
    yield "merge/bad-a-and-sizes", f, (-d.aln_rows, d.cidx, d.alns, d.cidx2), {}, {}
    yield "merge/bad-sizes-and-some-ops", f, (d.alns, d.cidx, d.alns, d.cidx2), dict(cigar_a=d.cigar), {}
    yield "merge/bad-some-ops-and-spans", f, (d.alns, d.cidx, d.alns[:2], d.cidx), dict(cigar_b=d.cigar), {}

    f = fm_md.md_tags
    base = (d.text, d.rlist, d.alns, d.cidx, d.cigar, d.oidx)
    yield "md/list", f, base, {}, {}
    yield "md/tuple-rows", f, (d.text, d.rtuple, d.aln_rows) + base[3:], dict(device=1), {}
    yield "md/both-strands", f, (d.text, d.rlist, d.alns, d.cidx2, d.cigar, d.oidx), dict(both_strands=True), {}
    yield "md/hits-structured", f, base, dict(hits=d.hits), {}
    yield "md/hits-rows", f, base, dict(hits=d.hit_rows[:2]), {}
    yield "md/hits-numbers", f, base, dict(hits=[2, 0, 2, 1]), {}
    yield "md/hits-none-of-them", f, base, dict(hits=[]), {}
    yield "md/hits-no-rows", f, base, dict(hits=np.zeros((0, 8), np.int32)), ok0
    yield "md/ok-first", f, base, {}, ok0
    yield "md/index-from-1", f, (d.text, d.rlist, np.concatenate([d.alns, d.alns]), d.cidx_off, d.cigar, d.oidx), {}, {}
    yield "md/index-descends", f, (d.text, d.rlist, d.alns, [3, 2, 1], d.cigar, d.oidx), {}, {}
    yield "md/empty-batch", f, ([], [], [], [0], [], [0]), {}, ok0
    yield "md/empty-batch-tuple", f, ([], ([], [0]), d.none, [0], [], [0]), dict(hits=d.hits[:0]), {}
    yield "md/empty-alignments", f, (d.text, d.rlist, [], [0, 0, 0], [], [0]), {}, ok0
    yield "md/no-ops", f, (d.text, d.rlist, d.alns, d.cidx, [], [0, 0, 0, 0]), {}, {}
    yield "md/fails", f, base, {}, {"rc": _lib.KISS_HIP_E_HIP}
    yield "md/bad-alignments", f, (d.text, d.rlist, -d.aln_rows) + base[3:], {}, {}
    yield "md/bad-read-index-empty", f, (d.text, (d.rtuple[0], [])) + base[2:], {}, {}
    yield "md/bad-read-index-2d", f, (d.text, (d.rtuple[0], [[0, 5, 8]])) + base[2:], {}, {}
    yield "md/bad-chain-index-size", f, (d.text, d.rlist, d.alns, d.cidx2, d.cigar, d.oidx), {}, {}
    yield "md/bad-read-index-past", f, (d.text, (d.rtuple[0], [0, 5, 9])) + base[2:], {}, {}
    yield "md/bad-chain-index-spans", f, (d.text, d.rlist, d.alns, [0, 2, 4], d.cigar, [0, 1, 2, 3, 4]), {}, {}
    yield "md/bad-cigar-index-short", f, base[:5] + ([0, 2, 3],), {}, {}
    yield "md/bad-cigar-index-past", f, base[:5] + ([0, 2, 3, 5],), {}, {}
    yield "md/bad-hits-rows", f, base, dict(hits=-d.hit_rows), {}
    yield "md/bad-hits-numbers", f, base, dict(hits=[0, -1]), {}
    yield "md/bad-hits-numbers-big", f, base, dict(hits=[0, 1 << 32]), {}
    yield "md/bad-alignments-and-size", f, (d.text, d.rlist, -d.aln_rows, d.cidx2, d.cigar, d.oidx), {}, {}
    yield "md/bad-size-and-past", f, (d.text, (d.rtuple[0], [0, 5, 9]), d.alns, d.cidx2, d.cigar, d.oidx), {}, {}
    yield "md/bad-past-and-cigar", f, (d.text, (d.rtuple[0], [0, 5, 9]), d.alns, d.cidx, d.cigar, [0, 2, 3]), {}, {}
    yield "md/bad-cigar-and-hits", f, base[:5] + ([0, 2, 3],), dict(hits=[0, -1]), {}

    f = reads.interleave_reads
    qa, qb = np.arange(8, dtype=np.uint8) + 33, [40, 41, 42, 43, 44, 45]
    a, b = d.rtuple, (np.array([1, 1, 2, 2, 3, 3], np.uint8), [0, 2, 6])
    yield "interleave/tuples", f, (a, b), {}, {}
    yield "interleave/tuples-qual", f, (a + (qa,), b + (qb,)), dict(device=1), {}
    yield "interleave/dicts-names", f, (dict(reads=a[0], read_index=a[1], qual=qa, names=["x", "y"]),
                                        dict(reads=b[0], read_index=b[1], qual=qb, names=["x2", "y2"])), {}, {}
    yield "interleave/dicts-no-names", f, (dict(reads=a[0], read_index=a[1], names=None), dict(reads=b[0], read_index=b[1], names=["u", "v"])), {}, {}
    yield "interleave/dict-and-tuple", f, (dict(reads=a[0], read_index=a[1], names=["x", "y"]), b), {}, {}
    yield "interleave/empty-batch", f, (([], [0]), ([], [0])), {}, {}
    yield "interleave/empty-batch-qual", f, (([], [0], []), ([], [0], [])), {}, {}
    yield "interleave/empty-reads", f, (([], [0, 0]), b[:1] + ([0, 6],)), {}, {}
    yield "interleave/fails", f, (a, b), {}, {"rc": _lib.KISS_HIP_E_HIP}
    yield "interleave/bad-index-empty", f, ((a[0], []), b), {}, {}
    yield "interleave/bad-one-qual", f, (a + (qa,), b), {}, {}
    yield "interleave/bad-counts", f, (a, (b[0], [0, 2, 4, 6])), {}, {}
    yield "interleave/bad-index-past", f, (a, (b[0], [0, 2, 7])), {}, {}
    yield "interleave/bad-qual-short", f, (a + (qa[:7],), b + (qb,)), {}, {}
    yield "interleave/bad-empty-and-qual", f, ((a[0], [], qa), b), {}, {}
    yield "interleave/bad-qual-and-counts", f, (a + (qa,), (b[0], [0, 2, 4, 6])), {}, {}
    yield "interleave/bad-counts-and-past", f, ((a[0], [0, 9]), b), {}, {}


def plain(x):
    """a result as JSON holds it: arrays as lists with their dtype, long ones by their sum and ends"""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        d = {"dtype": [[k, x.dtype[k].str] for k in x.dtype.names] if x.dtype.names else x.dtype.str, "shape": list(x.shape)}
        if x.size > 64 and not x.dtype.names:
            d.update(sum=int(x.astype(np.int64).sum()), head=x.ravel()[:8].tolist(), tail=x.ravel()[-8:].tolist())
        else:
            d["data"] = x.tolist()
        return d
    if isinstance(x, ctypes.Structure):
        return {"struct": type(x).__name__, "fields": {k: plain(getattr(x, k)) for k, _ in x._fields_}}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def answer(f, args, kwargs, stub=None):
    """-> what is recorded for one case: the calls the stub saw, and the result or the exception"""
    with stubbed(Stub(**(stub or {}))) as s:
        try:
            got = {"returns": plain(f(*args, **kwargs))}
        except Exception as x:  # noqa: BLE001 (which exception, and its text, is what is recorded)
            got = {"raises": [type(x).__name__, str(x)]}
    got["calls"] = s.calls
    return json.loads(json.dumps(got))


def cases():
    out = {name: (f, (), kw, None) for name, f, kw in param_cases()}
    n = len(out)
    entries = list(entry_cases())
    out.update({name: (f, args, kw, stub) for name, f, args, kw, stub in entries})
    assert len(out) == n + len(entries), "two cases of one name"
    return out


def signatures():
    """every public function of the stage modules and of FMIndex, and the record layouts"""
    sig = {}
    for mod in STAGES:
        for name, f in sorted(vars(mod).items()):
            if inspect.isfunction(f) and f.__module__ == mod.__name__ and not name.startswith("_"):
                sig["%s.%s" % (mod.__name__, name)] = str(inspect.signature(f))
    for name, f in sorted(vars(FMIndex).items()):
        if not name.startswith("_") or name == "__init__":
            f = getattr(f, "__func__", f)
            if inspect.isfunction(f):
                sig["FMIndex.%s" % name] = str(inspect.signature(f))
    return sig


def constants():
    layouts = {"%s.%s" % (mod.__name__, k): plain(np.zeros(0, getattr(mod, k)))["dtype"] for mod, names in LAYOUTS for k in names}
    other = {"%s.%s" % (mod.__name__, k): plain(v) for mod in STAGES for k, v in sorted(vars(mod).items())
             if k.endswith(("_FIELDS", "_DEFAULTS", "_LIMITS")) or k.startswith(("HIT_", "PAIR_", "ALN_", "ALIGN_", "INSERT_"))
             and isinstance(v, (int, tuple))}
    return json.loads(json.dumps({"layouts": layouts, "values": other, "exported": sorted(k for k, v in vars(kiss_amd).items() if not k.startswith("_") and not inspect.ismodule(v))}))


def record():
    """writes the golden file from the tree it runs in"""
    got = {"signatures": signatures(), "constants": constants(), "answers": {name: answer(*c) for name, c in cases().items()}}
    with open(GOLDEN, "w") as g:
        json.dump(got, g, indent=None, separators=(",", ":"), sort_keys=True)
        g.write("\n")


def _recorded():
    with open(GOLDEN) as g:
        return json.load(g)


def test_the_entries_answer_as_they_did():
    recorded, now = _recorded()["answers"], cases()
    assert sorted(recorded) == sorted(now) and len(recorded) > 150
    wrong = [name for name, c in now.items() if answer(*c) != recorded[name]]
    assert not wrong, (wrong[:5], answer(*now[wrong[0]]), recorded[wrong[0]])


def test_the_recording_reaches_the_library_and_the_checks():
    """(the recording is of use only if its cases get where they are meant to)"""
    recorded = _recorded()["answers"]
    for entry in ENTRIES:
        of = [a for a in recorded.values() if a["calls"] and a["calls"][0]["entry"] == entry]
        assert len(of) > 5 and sum("returns" in a for a in of) > 4, entry
    sized = [a for a in recorded.values() if len(a["calls"]) == 2]
    assert len(sized) > 20 and all(a["calls"][0]["rc"] == _lib.KISS_HIP_E_INVALID and a["calls"][1]["rc"] == 0 for a in sized)
    refused = [a for name, a in recorded.items() if "/bad-" in name]
    assert len(refused) > 80 and all("raises" in a and not a["calls"] for a in refused)
    held = [a for a in recorded.values() if a["calls"] and any(v == [] for v in a["calls"][0]["in"].values())]
    assert len(held) > 20  # (an empty input handed over as a pointer that is not NULL)


def test_signatures_and_layouts_are_what_they_were():
    recorded = _recorded()
    assert signatures() == recorded["signatures"] and len(recorded["signatures"]) > 50
    assert constants() == recorded["constants"]
