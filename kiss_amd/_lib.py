"""ctypes binding of libkiss_hip.so (the C ABI declared in include/kiss_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or fails to
load, importing the entry points raises.  (The CPU oracle under oracle/ is test
infrastructure and is never imported from here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkiss_hip.so")
# the hooks build of the same sources (-DKISS_HIP_HOOKS: environment switches read at every call, fault injection,
# tracing -- kiss_amd/csrc/kiss_internal.hpp KissOpts).  Test infrastructure: only what asks for it (`load(hooks=True)`,
# `Context(..., hooks=True)`, or KISS_AMD_LIB=hooks for a whole process) ever loads it.
HOOKS_LIB_PATH = os.path.join(_HERE, "libkiss_hip_hooks.so")

KISS_HIP_OK = 0
KISS_HIP_E_INVALID, KISS_HIP_E_NO_DEVICE, KISS_HIP_E_HIP, KISS_HIP_E_NOMEM = -1, -2, -3, -4
KISS_HIP_E_UNSUPPORTED, KISS_HIP_E_INTERNAL, KISS_HIP_E_IO, KISS_HIP_E_DEEP = -5, -6, -7, -8
ALGO_PARALLEL_SORTING = 0
ALGO_PREFIX_DOUBLING = 1
MAX_N = 4294963200
# kiss_hip_stage_view: the ctx's own work arrays (include/kiss_hip.h)
VIEW_LOCAL_KEYS, VIEW_LOCAL_POS, VIEW_PART_KEYS, VIEW_PART_POS, VIEW_SORTED, VIEW_SORTED_CTX = range(6)

KERNEL_CLASSES = [
    "pack", "classify", "radix_hist", "radix_scatter", "scan", "keygather", "flag_compact",
    "place", "induce_count", "induce_scatter", "induce_small", "fm_query", "fm_build", "segrank",
    "group_heads", "isa",
]


class Report(ctypes.Structure):
    """what the library fills in for its caller: as_dict lists the fields but the reserved ones.  (A struct whose dict has
    more to it than that -- Stats, MultiStats, FmiMmReport -- has an as_dict of its own.)"""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class Stats(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64), ("m", ctypes.c_uint64), ("k", ctypes.c_uint32), ("depth", ctypes.c_uint32),
        ("lms_rounds", ctypes.c_uint32), ("induce_passes", ctypes.c_uint32), ("near_end", ctypes.c_uint64),
        ("sort_item_rounds", ctypes.c_uint64), ("big_item_rounds", ctypes.c_uint64),
        ("ms_total", ctypes.c_float), ("ms_pack", ctypes.c_float), ("ms_classify", ctypes.c_float),
        ("ms_lms_sort", ctypes.c_float), ("ms_place", ctypes.c_float), ("ms_induce", ctypes.c_float),
        ("ms_kernel", ctypes.c_float * 16), ("launches_kernel", ctypes.c_uint64 * 16),
        ("items_kernel", ctypes.c_uint64 * 16),
        ("refine_items", ctypes.c_uint64), ("refine_depth", ctypes.c_uint32), ("doubling_rounds", ctypes.c_uint32),
        ("ms_refine", ctypes.c_float), ("ms_h2d", ctypes.c_float), ("ms_d2h", ctypes.c_float),
        ("refine_form", ctypes.c_uint32), ("ms_fm_range", ctypes.c_float), ("ms_fm_locate", ctypes.c_float),
        ("tie_run_retries", ctypes.c_uint32), ("pair_records", ctypes.c_uint32),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if not k.endswith("_kernel")}
        d["kernels"] = {
            name: {"ms": self.ms_kernel[i], "launches": self.launches_kernel[i], "items": self.items_kernel[i]}
            for i, name in enumerate(KERNEL_CLASSES)
        }
        return d


class MultiStats(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64), ("m", ctypes.c_uint64), ("ndev", ctypes.c_uint32), ("refine_depth", ctypes.c_uint32),
        ("piece", ctypes.c_uint64 * 8),
        ("ms_total", ctypes.c_float), ("ms_pack", ctypes.c_float), ("ms_classify", ctypes.c_float),
        ("ms_partition", ctypes.c_float), ("ms_exchange", ctypes.c_float), ("ms_sort", ctypes.c_float),
        ("ms_gather", ctypes.c_float), ("ms_induce", ctypes.c_float),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "piece"}
        d["piece"] = [int(x) for x in self.piece][:max(1, min(8, self.ndev))]
        return d


class VerifyReport(Report):
    _fields_ = [
        ("n", ctypes.c_uint64), ("k", ctypes.c_uint32), ("exact", ctypes.c_uint32), ("ok", ctypes.c_uint32),
        ("sa0_ok", ctypes.c_uint32), ("out_of_range", ctypes.c_uint64), ("duplicates", ctypes.c_uint64),
        ("order_violations", ctypes.c_uint64), ("first_violation", ctypes.c_uint64), ("tied_pairs", ctypes.c_uint64),
        ("digest", ctypes.c_uint64), ("ms", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class LcpReport(Report):
    _fields_ = [
        ("n", ctypes.c_uint64), ("irreducible", ctypes.c_uint64), ("long_pairs", ctypes.c_uint64),
        ("lcp_sum", ctypes.c_uint64), ("max_lcp", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
        ("ms_total", ctypes.c_float), ("ms_phi", ctypes.c_float), ("ms_short", ctypes.c_float), ("ms_long", ctypes.c_float),
        ("ms_scan_gather", ctypes.c_float), ("reserved2_", ctypes.c_uint32),
    ]


class FmiView(ctypes.Structure):
    _fields_ = [
        ("n_sa", ctypes.c_uint64), ("cnt", ctypes.c_uint32 * 4), ("pri", ctypes.c_uint32),
        ("sa_intv", ctypes.c_uint32), ("bwt", ctypes.c_void_p), ("occ1", ctypes.c_void_p),
        ("occ2", ctypes.c_void_p), ("sa", ctypes.c_void_p), ("b", ctypes.c_void_p), ("b_occ", ctypes.c_void_p),
    ]


class FmiViewEx(ctypes.Structure):
    _fields_ = [("base", FmiView), ("lookup_len", ctypes.c_uint32), ("lookup", ctypes.c_void_p)]


class FmiSizes(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in ("n_sa", "bwt_bytes", "occ1_entries", "occ2_bytes", "sa_entries", "b_words",
                                               "b_occ_entries")]


class FmiSizesEx(ctypes.Structure):
    _fields_ = [("base", FmiSizes), ("lookup_entries", ctypes.c_uint64)]


class FmiMmReport(ctypes.Structure):
    """kiss_hip_fmi_mm_report"""
    _fields_ = [
        ("Q", ctypes.c_uint64), ("L", ctypes.c_uint32), ("max_mismatches", ctypes.c_uint32),
        ("hits", ctypes.c_uint64 * 4), ("ranges", ctypes.c_uint64), ("lf_pairs", ctypes.c_uint64),
        ("walk_failures", ctypes.c_uint64), ("checksum", ctypes.c_uint64),
        ("ms_total", ctypes.c_float), ("ms_search", ctypes.c_float), ("ms_locate", ctypes.c_float),
        ("ms_sort", ctypes.c_float),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "hits"}
        d["hits"] = [int(x) for x in self.hits]
        return d


class FmiSeed(ctypes.Structure):
    """kiss_hip_fmi_seed"""
    _fields_ = [("start", ctypes.c_uint32), ("len", ctypes.c_uint32), ("sa_beg", ctypes.c_uint32), ("sa_end", ctypes.c_uint32)]


class FmiSeedReport(Report):
    """kiss_hip_fmi_seed_report"""
    _fields_ = [
        ("Q", ctypes.c_uint64), ("V", ctypes.c_uint64), ("bases", ctypes.c_uint64), ("seeds", ctypes.c_uint64),
        ("located_seeds", ctypes.c_uint64), ("positions", ctypes.c_uint64), ("lf_pairs", ctypes.c_uint64),
        ("walk_failures", ctypes.c_uint64), ("checksum", ctypes.c_uint64), ("max_ms", ctypes.c_uint32),
        ("reserved_", ctypes.c_uint32), ("ms_total", ctypes.c_float), ("ms_search", ctypes.c_float),
        ("ms_compact", ctypes.c_float), ("ms_locate", ctypes.c_float), ("ms_sort", ctypes.c_float),
    ]


class ChainParams(ctypes.Structure):
    """kiss_hip_chain_params"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("max_gap", "band", "gap_cost", "max_lookback", "min_score")]


class Chain(ctypes.Structure):
    """kiss_hip_chain"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("score", "anchors", "rbeg", "rend", "tbeg", "tend")]


class ChainAnchor(ctypes.Structure):
    """kiss_hip_chain_anchor"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("rstart", "tpos", "len")]


class ChainReport(Report):
    """kiss_hip_chain_report"""
    _fields_ = [
        ("V", ctypes.c_uint64), ("anchors", ctypes.c_uint64), ("chains", ctypes.c_uint64), ("chain_anchors", ctypes.c_uint64),
        ("dp_pairs", ctypes.c_uint64), ("max_anchors", ctypes.c_uint32), ("best_score", ctypes.c_uint32),
        ("ms_total", ctypes.c_float), ("ms_sort", ctypes.c_float), ("ms_dp", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class AlignParams(ctypes.Structure):
    """kiss_hip_align_params"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("match", "mismatch", "gap_open", "gap_extend", "band")]


class Aln(ctypes.Structure):
    """kiss_hip_aln"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("score", "flags", "rbeg", "rend", "tbeg", "tend", "matches", "mismatches", "ins",
                                               "del", "gaps", "band")]


class AlignReport(Report):
    """kiss_hip_align_report"""
    _fields_ = [
        ("V", ctypes.c_uint64), ("chains", ctypes.c_uint64), ("aligned", ctypes.c_uint64), ("too_wide", ctypes.c_uint64),
        ("cells", ctypes.c_uint64), ("cigar_ops", ctypes.c_uint64), ("best_score", ctypes.c_uint32), ("max_band", ctypes.c_uint32),
        ("ms_total", ctypes.c_float), ("ms_dp", ctypes.c_float), ("ms_trace", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class SelectParams(ctypes.Structure):
    """kiss_hip_select_params"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("min_score", "overlap", "mapq_coef", "mapq_max", "max_hits")]


class Hit(ctypes.Structure):
    """kiss_hip_hit"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("aln", "flags", "mapq", "score", "sub", "n_sec", "head", "ref")]


class SelectReport(Report):
    """kiss_hip_select_report"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("Q", "V", "alignments", "candidates", "spanning", "redundant", "hits", "heads",
                                               "mapped")] + [
        ("max_candidates", ctypes.c_uint32), ("reserved_", ctypes.c_uint32), ("ms_total", ctypes.c_float),
        ("ms_sort", ctypes.c_float), ("ms_walk", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class PairParams(ctypes.Structure):
    """kiss_hip_pair_params"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("ins_min", "ins_max", "ins_mean", "pen_coef", "pen_max", "mapq_coef", "mapq_max")]


class Pair(ctypes.Structure):
    """kiss_hip_pair"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("hit1", "hit2", "flags", "tlen", "score", "sub1", "sub2", "mapq1", "mapq2", "n_conc")]


class PairReport(Report):
    """kiss_hip_pair_report"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("P", "eligible", "combinations", "concordant", "proper", "promoted", "lifted",
                                               "bad_input", "max_combinations")] + [
        ("ms_total", ctypes.c_float), ("ms_check", ctypes.c_float), ("ms_pair", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class RescueParams(ctypes.Structure):
    """kiss_hip_rescue_params"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("ins_min", "ins_max", "max_anchors", "min_anchor_score", "max_width")]


class RescueReport(Report):
    """kiss_hip_rescue_report"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("P", "pairs_planned", "anchors", "chains", "split", "empty", "bad_input",
                                               "max_chains")] + [
        ("ms_total", ctypes.c_float), ("ms_check", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float),
    ]


class MergeReport(Report):
    """kiss_hip_merge_report"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("V", "alignments_a", "alignments_b", "alignments", "cigar_ops")] + [
        ("ms_total", ctypes.c_float), ("ms_place", ctypes.c_float), ("ms_copy", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class ReadsReport(Report):
    """kiss_hip_reads_report (include/kiss_hip_reads.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("lines", "reads", "bases", "no_base", "empty_reads", "first_empty", "bad_records",
                                               "first_bad")] + [
        ("format", ctypes.c_uint32), ("has_qual", ctypes.c_uint32), ("first_bad_kind", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
        ("ms_total", ctypes.c_float), ("ms_lines", ctypes.c_float), ("ms_reads", ctypes.c_float), ("ms_copy", ctypes.c_float),
    ]


class ReadsPartReport(ctypes.Structure):
    """kiss_hip_reads_part_report (include/kiss_hip_reads_part.h)"""
    _fields_ = [("parsed", ReadsReport), ("records_complete", ctypes.c_uint64), ("records", ctypes.c_uint64), ("bytes_used", ctypes.c_uint64)]


class SamInput(ctypes.Structure):
    """kiss_hip_sam_input (include/kiss_hip_sam.h): 18 pointers, then the counts"""
    POINTERS = ("reads", "read_index", "qual", "names", "name_off", "name_len", "alns", "cigar", "cigar_index", "hits", "hit_index",
                "pairs", "source", "md", "md_index", "ref_names", "ref_name_index", "bounds")
    _fields_ = [(k, ctypes.c_void_p) for k in POINTERS] + [(k, ctypes.c_uint64) for k in ("Q", "C", "R", "first_alns")]


class SamReport(Report):
    """kiss_hip_sam_report (include/kiss_hip_sam.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("lines", "sam_bytes", "unmapped_lines", "longest", "bad", "first_bad")] + [
        ("ms_total", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class BamReport(Report):
    """kiss_hip_bam_report (include/kiss_hip_bam.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "bam_bytes", "unmapped_records", "longest", "bad", "first_bad")] + [
        ("ms_total", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class BgzfReport(Report):
    """kiss_hip_bgzf_report (include/kiss_hip_bam.h)"""
    _fields_ = [("blocks", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("ms_total", ctypes.c_float), ("reserved_", ctypes.c_uint32)]


class BgzfDeflateReport(Report):
    """kiss_hip_bgzf_deflate_report (include/kiss_hip_deflate.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("blocks", "out_bytes", "stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches",
                                               "match_bytes")] + [(k, ctypes.c_float) for k in ("ms_total", "ms_block", "ms_scan", "ms_copy")]


class BamSortReport(Report):
    """kiss_hip_bam_sort_report (include/kiss_hip_bam_sort.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "bam_bytes", "unplaced", "longest", "bad", "first_bad")] + [
        (k, ctypes.c_float) for k in ("ms_total", "ms_key", "ms_sort", "ms_copy")]


class BaiReport(Report):
    """kiss_hip_bai_report (include/kiss_hip_bai.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "bam_bytes", "bai_bytes", "chunks", "bins", "windows", "mapped", "unmapped_placed",
                                                "no_coor", "bad", "first_bad")] + [
        (k, ctypes.c_float) for k in ("ms_total", "ms_record", "ms_window", "ms_sort", "ms_emit")]


class MarkdupReport(Report):
    """kiss_hip_markdup_report (include/kiss_hip_markdup.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("records", "templates", "pairs", "fragments", "unmapped_templates", "ambiguous", "dup_pairs",
                                                "dup_fragments", "dup_records", "bad", "first_bad")] + [
        (k, ctypes.c_float) for k in ("ms_total", "ms_record", "ms_class", "ms_sort", "ms_mark")]


class MdReport(Report):
    """kiss_hip_md_report (include/kiss_hip_md.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("items", "bad", "md_bytes", "mismatch_columns", "deleted_bases", "longest")] + [
        ("ms_total", ctypes.c_float), ("ms_count", ctypes.c_float), ("ms_emit", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class PileupParams(ctypes.Structure):
    """kiss_hip_pileup_params (include/kiss_hip_pileup.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("min_mapq", "skip_flags", "proper_only", "reserved_")]


class PileupReport(Report):
    """kiss_hip_pileup_report (include/kiss_hip_pileup.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("items", "bad", "filtered", "unmapped", "counted", "columns", "alt_columns",
                                               "deleted_bases", "insertions", "clipped")] + [
        ("ms_total", ctypes.c_float), ("ms_check", ctypes.c_float), ("ms_walk", ctypes.c_float), ("reserved_", ctypes.c_uint32),
    ]


class InsertParams(ctypes.Structure):
    """kiss_hip_insert_params (include/kiss_hip_insert.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("min_mapq", "max_insert", "min_samples", "out_mult", "map_mult", "sd_mult")]


class InsertReport(Report):
    """kiss_hip_insert_report (include/kiss_hip_insert.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("P", "unmapped", "bad_input", "low_mapq", "discordant", "too_long", "samples", "used")] + [
        (k, ctypes.c_uint32) for k in ("flags", "q25", "q50", "q75", "mean", "sd", "ins_min", "ins_max", "ins_mean")] + [
        ("ms_total", ctypes.c_float), ("ms_hist", ctypes.c_float), ("ms_stats", ctypes.c_float),
    ]


class Fmi8View(ctypes.Structure):
    """kiss_hip_fmi8_view"""
    _fields_ = [
        ("n_sa", ctypes.c_uint64), ("pri", ctypes.c_uint32), ("sa_intv", ctypes.c_uint32), ("sigma", ctypes.c_uint32),
        ("reserved_", ctypes.c_uint32), ("C", ctypes.c_void_p), ("map", ctypes.c_void_p), ("bwt", ctypes.c_void_p),
        ("occ1", ctypes.c_void_p), ("occ2", ctypes.c_void_p), ("sa", ctypes.c_void_p), ("b", ctypes.c_void_p),
        ("b_occ", ctypes.c_void_p),
    ]


class Fmi8Sizes(Report):
    """kiss_hip_fmi8_sizes"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n_sa", "bwt_bytes", "occ1_entries", "occ2_entries", "sa_entries", "b_words",
                                               "b_occ_entries")]


class Fmi8Report(Report):
    """kiss_hip_fmi8_report"""
    _fields_ = [
        ("Q", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("lf_pairs", ctypes.c_uint64), ("walk_failures", ctypes.c_uint64),
        ("checksum", ctypes.c_uint64), ("ms_total", ctypes.c_float), ("ms_search", ctypes.c_float),
        ("ms_locate", ctypes.c_float), ("ms_sort", ctypes.c_float),
    ]


class KissHipError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = "%s failed: %s (%d)" % (where, strerror(status), status)
        if detail:
            msg += " [" + detail + "]"
        super().__init__(msg)


_libs = {}


def load(hooks=None):
    """Load libkiss_hip.so (hooks=True: libkiss_hip_hooks.so); raises (never falls back) when it is missing."""
    if hooks is None:
        hooks = os.environ.get("KISS_AMD_LIB", "") == "hooks"
    hooks = bool(hooks)
    if hooks in _libs:
        return _libs[hooks]
    path = HOOKS_LIB_PATH if hooks else LIB_PATH
    # A-B harnesses (tools/ab_libs.sh, tools/rx_ab.sh) name a variant build of the default library by path instead of
    # overwriting the shipped file
    if not hooks and os.environ.get("KISS_AMD_LIB_PATH"):
        path = os.environ["KISS_AMD_LIB_PATH"]
    if not os.path.exists(path):
        raise ImportError(
            "%s not built at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C kiss_amd/csrc`; there is no CPU fallback" % (os.path.basename(path), path))
    lib = ctypes.CDLL(path)
    if hasattr(lib, "kiss_hip_has_hooks"):  # (a variant named by KISS_AMD_LIB_PATH may be a build of an earlier round)
        lib.kiss_hip_has_hooks.restype = ctypes.c_int
        if bool(lib.kiss_hip_has_hooks()) != hooks and not os.environ.get("KISS_AMD_LIB_PATH"):
            raise ImportError("%s is not the %s build" % (path, "hooks" if hooks else "default"))
    elif hooks:
        raise ImportError("%s is not a hooks build" % path)
    vp, u8p = ctypes.c_void_p, ctypes.c_void_p
    lib.kiss_hip_version.restype = ctypes.c_int
    lib.kiss_hip_strerror.restype = ctypes.c_char_p
    lib.kiss_hip_strerror.argtypes = [ctypes.c_int]
    lib.kiss_hip_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.kiss_hip_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_uint64]
    lib.kiss_hip_ctx_create_sized.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    lib.kiss_hip_ctx_release_io_buffers.argtypes = [vp]
    ip = ctypes.POINTER(ctypes.c_int)
    lib.kiss_hip_multi_create.argtypes = [ctypes.POINTER(vp), ip, ctypes.c_int, ctypes.c_uint64]
    lib.kiss_hip_multi_destroy.argtypes = [vp]
    lib.kiss_hip_multi_suffix_sort_dna_u32.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp]
    lib.kiss_hip_multi_suffix_sort_dna_u32_dev.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp]
    lib.kiss_hip_multi_get_stats.argtypes = [vp, ctypes.POINTER(MultiStats)]
    lib.kiss_hip_multi_ctx.argtypes = [vp, ctypes.c_int]
    lib.kiss_hip_multi_ctx.restype = vp
    lib.kiss_hip_suffix_sort_dna_u32_multi.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp, ip, ctypes.c_int]
    lib.kiss_hip_stage_view.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64)]
    lib.kiss_hip_stage_reserve.argtypes = [vp, ctypes.c_uint64]
    lib.kiss_hip_debug_fail_alloc_over.argtypes = [vp, ctypes.c_uint64]
    lib.kiss_hip_debug_fail_alloc_over.restype = ctypes.c_int
    lib.kiss_hip_debug_splitters.argtypes = [vp, ctypes.c_uint64, ctypes.c_int, vp, vp]
    lib.kiss_hip_debug_splitters.restype = ctypes.c_int
    lib.kiss_hip_ctx_destroy.argtypes = [vp]
    lib.kiss_hip_ctx_set_profiling.argtypes = [vp, ctypes.c_int]
    lib.kiss_hip_ctx_set_profiling_mask.argtypes = [vp, ctypes.c_uint64]
    lib.kiss_hip_last_hip_error.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p)]
    lib.kiss_hip_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.kiss_hip_ctx_workspace_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.kiss_hip_suffix_sort_dna_u32.argtypes = [u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp, ctypes.c_int]
    lib.kiss_hip_ctx_suffix_sort_dna_u32.argtypes = [vp, u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp]
    lib.kiss_hip_ctx_suffix_sort_dna_u32_dev.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, vp, vp]
    lib.kiss_hip_ctx_get_stage_outputs.argtypes = [vp, vp, vp, vp]
    lib.kiss_hip_ctx_verify_sa_dev.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp, ctypes.POINTER(VerifyReport), vp]
    lib.kiss_hip_ctx_verify_sa_dev.restype = ctypes.c_int
    lib.kiss_hip_sa_digest_host.argtypes = [vp, ctypes.c_uint64]
    lib.kiss_hip_sa_digest_host.restype = ctypes.c_uint64
    lib.kiss_hip_fnv1a64_host.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64]
    lib.kiss_hip_fnv1a64_host.restype = ctypes.c_uint64
    lib.kiss_hip_debug_radix_sort.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int]
    lib.kiss_hip_debug_radix_sort_seg.argtypes = [vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    lib.kiss_hip_debug_radix_sort_seg.restype = ctypes.c_int
    lib.kiss_hip_debug_scan_u32.argtypes = [vp, vp, ctypes.c_uint64]
    u64 = ctypes.c_uint64
    lib.kiss_hip_stage_classify.argtypes = [vp, vp, u64, ctypes.c_uint32, u64, u64, ctypes.POINTER(u64 * 13), vp]
    lib.kiss_hip_stage_local_lms.argtypes = [vp, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.kiss_hip_stage_key_hist.argtypes = [vp, vp, u64, ctypes.c_int, vp, vp]
    lib.kiss_hip_stage_partition.argtypes = [vp, vp, vp, u64, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp]
    lib.kiss_hip_stage_sort.argtypes = [vp, vp, vp, u64, u64, ctypes.c_uint32, vp, vp, vp]
    lib.kiss_hip_stage_induce.argtypes = [vp, u64, ctypes.c_uint32, vp, vp, u64, vp, u64, ctypes.POINTER(u64 * 12), vp, vp]
    lib.kiss_hip_stage_induce_exact.argtypes = [vp, u64, ctypes.c_uint32, vp, vp, u64, vp, u64, ctypes.POINTER(u64 * 12), vp, vp,
                                                ctypes.POINTER(ctypes.c_int)]
    lib.kiss_hip_stage_refine_exact.argtypes = [vp, u64, ctypes.c_uint32, vp, vp]
    lib.kiss_hip_stage_refine_exact.restype = ctypes.c_int
    lib.kiss_hip_fmi_query_batch_dev.argtypes = [
        vp, ctypes.POINTER(FmiView), vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp,
        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), vp, vp, ctypes.c_uint64, vp]
    lib.kiss_hip_fmi_build_dev.argtypes = [
        vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp,
        ctypes.POINTER(ctypes.c_uint32 * 4), ctypes.POINTER(ctypes.c_uint32), vp]
    u32 = ctypes.c_uint32
    lib.kiss_hip_fmi_sizes_ex_for.argtypes = [u64, u32, u32, ctypes.POINTER(FmiSizesEx)]
    lib.kiss_hip_fmi_build_ex_dev.argtypes = [
        vp, vp, u64, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(u32 * 4), ctypes.POINTER(u32), vp]
    lib.kiss_hip_fmi_query_ex_dev.argtypes = [
        vp, ctypes.POINTER(FmiViewEx), vp, u32, u64, u32, vp, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64), vp, vp,
        u64, vp]
    lib.kiss_hip_fmi_build_ex_host.argtypes = [vp, u64, vp, u32, u32] + [vp] * 9 + [ctypes.c_int]
    lib.kiss_hip_fmi_query_ex_host.argtypes = [ctypes.POINTER(FmiViewEx), vp, u32, u64, u32, vp, vp, vp,
                                               ctypes.POINTER(u64), ctypes.POINTER(u64), vp, vp, u64, ctypes.c_int]
    lib.kiss_hip_fmi_query_mm_dev.argtypes = [vp, ctypes.POINTER(FmiView), vp, u32, u64, u32, vp, vp, vp, vp, u64,
                                              ctypes.POINTER(FmiMmReport), vp]
    lib.kiss_hip_fmi_query_mm_host.argtypes = [ctypes.POINTER(FmiView), vp, u32, u64, u32, vp, vp, vp, vp, u64,
                                               ctypes.POINTER(FmiMmReport), ctypes.c_int]
    lib.kiss_hip_fmi_query_mm_dev.restype = lib.kiss_hip_fmi_query_mm_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_seeds_dev.argtypes = [vp, ctypes.POINTER(FmiViewEx), vp, vp, u64, u32, u32, u32, ctypes.c_int, vp, vp, vp, u64,
                                           vp, vp, u64, ctypes.POINTER(FmiSeedReport), vp]
    lib.kiss_hip_fmi_seeds_host.argtypes = [ctypes.POINTER(FmiViewEx), vp, vp, u64, u32, u32, u32, ctypes.c_int, vp, vp, vp, u64,
                                            vp, vp, u64, ctypes.POINTER(FmiSeedReport), ctypes.c_int]
    lib.kiss_hip_fmi_seeds_dev.restype = lib.kiss_hip_fmi_seeds_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_chain_dev.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.POINTER(ChainParams), vp, vp, u64, vp, vp, u64,
                                           ctypes.POINTER(ChainReport), vp]
    lib.kiss_hip_fmi_chain_host.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(ChainParams), vp, vp, u64, vp, vp, u64,
                                            ctypes.POINTER(ChainReport), ctypes.c_int]
    lib.kiss_hip_fmi_chain_dev.restype = lib.kiss_hip_fmi_chain_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_align_dev.argtypes = [vp, vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, ctypes.POINTER(AlignParams), vp, u64, vp,
                                           vp, u64, ctypes.POINTER(AlignReport), vp]
    lib.kiss_hip_fmi_align_host.argtypes = [vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, ctypes.POINTER(AlignParams), vp, u64, vp, vp,
                                            u64, ctypes.POINTER(AlignReport), ctypes.c_int]
    lib.kiss_hip_fmi_align_dev.restype = lib.kiss_hip_fmi_align_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_select_dev.argtypes = [vp, vp, vp, vp, u64, ctypes.c_int, vp, u64, ctypes.POINTER(SelectParams), vp, vp, u64,
                                            ctypes.POINTER(SelectReport), vp]
    lib.kiss_hip_fmi_select_host.argtypes = [vp, vp, vp, u64, ctypes.c_int, vp, u64, ctypes.POINTER(SelectParams), vp, vp, u64,
                                             ctypes.POINTER(SelectReport), ctypes.c_int]
    lib.kiss_hip_fmi_select_dev.restype = lib.kiss_hip_fmi_select_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_pair_dev.argtypes = [vp, vp, vp, u64, vp, u64, ctypes.POINTER(PairParams), vp, ctypes.POINTER(PairReport), vp]
    lib.kiss_hip_fmi_pair_host.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(PairParams), vp, ctypes.POINTER(PairReport),
                                           ctypes.c_int]
    lib.kiss_hip_fmi_pair_dev.restype = lib.kiss_hip_fmi_pair_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_rescue_dev.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(RescueParams), vp, vp, vp, u64,
                                            ctypes.POINTER(RescueReport), vp]
    lib.kiss_hip_fmi_rescue_host.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(RescueParams), vp, vp, vp, u64,
                                             ctypes.POINTER(RescueReport), ctypes.c_int]
    lib.kiss_hip_fmi_rescue_dev.restype = lib.kiss_hip_fmi_rescue_host.restype = ctypes.c_int
    lib.kiss_hip_fmi_aln_merge_dev.argtypes = [vp] * 9 + [u64, vp, u64, vp, vp, vp, vp, u64, ctypes.POINTER(MergeReport), vp]
    lib.kiss_hip_fmi_aln_merge_host.argtypes = [vp] * 8 + [u64, vp, u64, vp, vp, vp, vp, u64, ctypes.POINTER(MergeReport), ctypes.c_int]
    lib.kiss_hip_fmi_aln_merge_dev.restype = lib.kiss_hip_fmi_aln_merge_host.restype = ctypes.c_int
    lib.kiss_hip_reads_parse_dev.argtypes = [vp, vp, u64, ctypes.c_int, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(ReadsReport), vp]
    lib.kiss_hip_reads_parse_host.argtypes = [vp, u64, ctypes.c_int, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(ReadsReport), ctypes.c_int]
    lib.kiss_hip_reads_parse_part_dev.argtypes = [vp, vp, u64, ctypes.c_int, ctypes.c_int, u64, vp, vp, u64, vp, vp, vp, u64,
                                                  ctypes.POINTER(ReadsPartReport), vp]
    lib.kiss_hip_reads_parse_part_host.argtypes = [vp, u64, ctypes.c_int, ctypes.c_int, u64, vp, vp, u64, vp, vp, vp, u64,
                                                   ctypes.POINTER(ReadsPartReport), ctypes.c_int]
    lib.kiss_hip_reads_interleave_dev.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(u64), vp]
    lib.kiss_hip_reads_interleave_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, u64, ctypes.POINTER(u64), ctypes.c_int]
    for name in READS_EXPORTED_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    lib.kiss_hip_fmi_md_dev.argtypes = [vp, vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, vp, u64, vp, vp, vp, u64,
                                        ctypes.POINTER(MdReport), vp]
    lib.kiss_hip_fmi_md_host.argtypes = [vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, vp, u64, vp, vp, vp, u64,
                                         ctypes.POINTER(MdReport), ctypes.c_int]
    for name in MD_EXPORTED_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_fmi_pileup_dev"):  # (the parent commit's library under KISS_AMD_LIB_PATH, for an A-B of bench.py, has none)
        lib.kiss_hip_fmi_pileup_dev.argtypes = [vp, vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, vp, u64, vp, u64,
                                                ctypes.POINTER(PileupParams), u64, u64, vp, ctypes.c_int, ctypes.POINTER(PileupReport), vp]
        lib.kiss_hip_fmi_pileup_host.argtypes = [vp, u64, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, vp, u64, vp, u64,
                                                 ctypes.POINTER(PileupParams), u64, u64, vp, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(PileupReport), ctypes.c_int]
        for name in PILEUP_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    lib.kiss_hip_fmi_sam_dev.argtypes = [vp, ctypes.POINTER(SamInput), vp, u64, vp, u64, vp, ctypes.POINTER(SamReport), vp]
    lib.kiss_hip_fmi_sam_host.argtypes = [ctypes.POINTER(SamInput), vp, u64, vp, u64, vp, ctypes.POINTER(SamReport), ctypes.c_int]
    for name in SAM_EXPORTED_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_fmi_bam_dev"):  # (as the pileup call: an older library under KISS_AMD_LIB_PATH has none)
        lib.kiss_hip_fmi_bam_dev.argtypes = [vp, ctypes.POINTER(SamInput), vp, u64, vp, u64, vp, ctypes.POINTER(BamReport), vp]
        lib.kiss_hip_fmi_bam_host.argtypes = [ctypes.POINTER(SamInput), vp, u64, vp, u64, vp, ctypes.POINTER(BamReport), ctypes.c_int]
        lib.kiss_hip_bgzf_dev.argtypes = [vp, vp, u64, u32, ctypes.c_int, vp, u64, ctypes.POINTER(BgzfReport), vp]
        lib.kiss_hip_bgzf_host.argtypes = [vp, u64, u32, ctypes.c_int, vp, u64, ctypes.POINTER(BgzfReport), ctypes.c_int]
        for name in BAM_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_bgzf_deflate_dev"):  # (as the BAM calls)
        lib.kiss_hip_bgzf_deflate_dev.argtypes = [vp, vp, u64, u32, ctypes.c_int, vp, u64, vp, u64, ctypes.POINTER(BgzfDeflateReport), vp]
        lib.kiss_hip_bgzf_deflate_host.argtypes = [vp, u64, u32, ctypes.c_int, vp, u64, vp, u64, ctypes.POINTER(BgzfDeflateReport), ctypes.c_int]
        for name in DEFLATE_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_bam_sort_dev"):  # (as the BAM calls)
        lib.kiss_hip_bam_sort_dev.argtypes = [vp, vp, u64, vp, u64, u32, vp, u64, vp, vp, ctypes.POINTER(BamSortReport), vp]
        lib.kiss_hip_bam_sort_host.argtypes = [vp, u64, vp, u64, u32, vp, u64, vp, vp, ctypes.POINTER(BamSortReport), ctypes.c_int]
        for name in BAM_SORT_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_bai_dev"):  # (as the BAM calls)
        lib.kiss_hip_bai_dev.argtypes = [vp, vp, u64, vp, u64, u32, u32, vp, u64, vp, u64, ctypes.POINTER(BaiReport), vp]
        lib.kiss_hip_bai_host.argtypes = [vp, u64, vp, u64, u32, u32, vp, u64, vp, u64, ctypes.POINTER(BaiReport), ctypes.c_int]
        for name in BAI_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    if hasattr(lib, "kiss_hip_bam_markdup_dev"):  # (as the BAM calls)
        lib.kiss_hip_bam_markdup_dev.argtypes = [vp, vp, u64, vp, u64, u32, u32, vp, ctypes.POINTER(MarkdupReport), vp]
        lib.kiss_hip_bam_markdup_host.argtypes = [vp, u64, vp, u64, u32, u32, vp, ctypes.POINTER(MarkdupReport), ctypes.c_int]
        for name in MARKDUP_EXPORTED_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int
    lib.kiss_hip_fmi_insert_dev.argtypes = [vp, vp, vp, u64, vp, u64, ctypes.POINTER(InsertParams), vp, ctypes.POINTER(InsertReport), vp]
    lib.kiss_hip_fmi_insert_host.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(InsertParams), vp, ctypes.POINTER(InsertReport),
                                             ctypes.c_int]
    for name in INSERT_EXPORTED_SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    lib.kiss_hip_fmi8_sizes_for.argtypes = [u64, u32, u32, ctypes.POINTER(Fmi8Sizes)]
    lib.kiss_hip_fmi8_build_dev.argtypes = [vp, vp, u64, vp, u32, u32] + [vp] * 8 + [ctypes.POINTER(u32), ctypes.POINTER(u32), vp]
    lib.kiss_hip_fmi8_build_host.argtypes = [vp, u64, vp, u32, u32] + [vp] * 8 + [ctypes.POINTER(u32), ctypes.POINTER(u32),
                                                                                  ctypes.c_int]
    lib.kiss_hip_fmi8_query_dev.argtypes = [vp, ctypes.POINTER(Fmi8View), vp, vp, u64, vp, vp, ctypes.POINTER(u64),
                                            ctypes.POINTER(u64), vp, vp, u64, ctypes.POINTER(Fmi8Report), vp]
    lib.kiss_hip_fmi8_query_host.argtypes = [ctypes.POINTER(Fmi8View), vp, vp, u64, vp, vp, ctypes.POINTER(u64),
                                             ctypes.POINTER(u64), vp, vp, u64, ctypes.POINTER(Fmi8Report), ctypes.c_int]
    for name in ("kiss_hip_fmi8_sizes_for", "kiss_hip_fmi8_build_dev", "kiss_hip_fmi8_build_host", "kiss_hip_fmi8_query_dev",
                 "kiss_hip_fmi8_query_host"):
        getattr(lib, name).restype = ctypes.c_int
    lib.kiss_hip_file_size.argtypes = [ctypes.c_char_p, ctypes.POINTER(u64)]
    lib.kiss_hip_ctx_parse_text_dev.argtypes = [vp, vp, u64, vp, ctypes.POINTER(u64), vp]
    lib.kiss_hip_ctx_load_text_file.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(u64)]
    lib.kiss_hip_copy_to_host.argtypes = [vp, vp, u64]
    lib.kiss_hip_suffix_sort_u8.argtypes = [vp, u64, vp, ctypes.c_int]
    lib.kiss_hip_suffix_sort_u8.restype = ctypes.c_int
    lib.kiss_hip_ctx_suffix_sort_u8_dev.argtypes = [vp, vp, u64, vp, vp]
    lib.kiss_hip_ctx_suffix_sort_u8_dev.restype = ctypes.c_int
    lib.kiss_hip_free_dev.argtypes = [vp]
    lib.kiss_hip_alloc_dev.argtypes = [ctypes.POINTER(vp), u64]
    lib.kiss_hip_alloc_dev.restype = ctypes.c_int
    for name in ("kiss_hip_ctx_lcp_dna_u32_dev", "kiss_hip_ctx_lcp_u8_dev"):
        getattr(lib, name).argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(LcpReport), vp]
        getattr(lib, name).restype = ctypes.c_int
    for name in ("kiss_hip_lcp_dna_u32", "kiss_hip_lcp_u8"):
        getattr(lib, name).argtypes = [vp, u64, vp, vp, vp, ctypes.c_int]
        getattr(lib, name).restype = ctypes.c_int
    for name in ("kiss_hip_file_size", "kiss_hip_ctx_parse_text_dev", "kiss_hip_ctx_load_text_file",
                 "kiss_hip_copy_to_host", "kiss_hip_free_dev"):
        getattr(lib, name).restype = ctypes.c_int
    for name in ("kiss_hip_device_count", "kiss_hip_ctx_create", "kiss_hip_ctx_destroy", "kiss_hip_ctx_set_profiling", "kiss_hip_ctx_set_profiling_mask",
                 "kiss_hip_last_hip_error", "kiss_hip_get_stats", "kiss_hip_ctx_workspace_bytes",
                 "kiss_hip_suffix_sort_dna_u32", "kiss_hip_ctx_suffix_sort_dna_u32",
                 "kiss_hip_ctx_suffix_sort_dna_u32_dev", "kiss_hip_ctx_get_stage_outputs",
                 "kiss_hip_fmi_query_batch_dev", "kiss_hip_fmi_build_dev", "kiss_hip_debug_radix_sort",
                 "kiss_hip_debug_scan_u32", "kiss_hip_stage_classify", "kiss_hip_stage_local_lms",
                 "kiss_hip_stage_key_hist", "kiss_hip_stage_partition", "kiss_hip_stage_sort", "kiss_hip_stage_induce",
                 "kiss_hip_ctx_create_sized", "kiss_hip_ctx_release_io_buffers", "kiss_hip_multi_create",
                 "kiss_hip_multi_destroy", "kiss_hip_multi_suffix_sort_dna_u32", "kiss_hip_multi_suffix_sort_dna_u32_dev",
                 "kiss_hip_multi_get_stats", "kiss_hip_suffix_sort_dna_u32_multi", "kiss_hip_stage_view",
                 "kiss_hip_stage_reserve", "kiss_hip_fmi_sizes_ex_for", "kiss_hip_fmi_build_ex_dev",
                 "kiss_hip_fmi_query_ex_dev", "kiss_hip_fmi_build_ex_host", "kiss_hip_fmi_query_ex_host"):
        getattr(lib, name).restype = ctypes.c_int
    _libs[hooks] = lib
    return lib


def strerror(status):
    return load().kiss_hip_strerror(int(status)).decode()


# every symbol include/kiss_hip.h declares (checked by tests/test_abi.py without a GPU)
EXPORTED_SYMBOLS = [
    "kiss_hip_version", "kiss_hip_strerror", "kiss_hip_device_count", "kiss_hip_ctx_create", "kiss_hip_ctx_destroy",
    "kiss_hip_ctx_set_profiling", "kiss_hip_ctx_set_profiling_mask", "kiss_hip_last_hip_error", "kiss_hip_get_stats", "kiss_hip_ctx_workspace_bytes",
    "kiss_hip_suffix_sort_dna_u32", "kiss_hip_ctx_suffix_sort_dna_u32", "kiss_hip_ctx_suffix_sort_dna_u32_dev",
    "kiss_hip_ctx_get_stage_outputs", "kiss_hip_ctx_verify_sa_dev", "kiss_hip_sa_digest_host", "kiss_hip_fnv1a64_host",
    "kiss_hip_fmi_query_batch_dev", "kiss_hip_fmi_build_dev",
    "kiss_hip_debug_radix_sort", "kiss_hip_debug_radix_sort_seg", "kiss_hip_debug_scan_u32",
    "kiss_hip_stage_classify", "kiss_hip_stage_local_lms", "kiss_hip_stage_key_hist", "kiss_hip_stage_partition",
    "kiss_hip_stage_sort", "kiss_hip_stage_induce", "kiss_hip_stage_induce_exact", "kiss_hip_stage_refine_exact",
    "kiss_hip_fmi_sizes_for", "kiss_hip_fmi_build_host", "kiss_hip_fmi_query_batch_host",
    "kiss_hip_file_size", "kiss_hip_ctx_parse_text_dev", "kiss_hip_ctx_load_text_file", "kiss_hip_copy_to_host",
    "kiss_hip_free_dev", "kiss_hip_alloc_dev", "kiss_hip_suffix_sort_u8", "kiss_hip_ctx_suffix_sort_u8_dev",
    "kiss_hip_ctx_create_sized", "kiss_hip_ctx_release_io_buffers", "kiss_hip_stage_view", "kiss_hip_stage_reserve",
    "kiss_hip_multi_create", "kiss_hip_multi_destroy", "kiss_hip_multi_suffix_sort_dna_u32",
    "kiss_hip_multi_suffix_sort_dna_u32_dev", "kiss_hip_multi_get_stats", "kiss_hip_multi_ctx",
    "kiss_hip_suffix_sort_dna_u32_multi", "kiss_hip_debug_splitters", "kiss_hip_debug_fail_alloc_over",
    "kiss_hip_has_hooks", "kiss_hip_release_cached_contexts", "kiss_hip_get_stats_sized",
    "kiss_hip_fmi_sizes_ex_for", "kiss_hip_fmi_build_ex_dev", "kiss_hip_fmi_query_ex_dev", "kiss_hip_fmi_build_ex_host",
    "kiss_hip_fmi_query_ex_host", "kiss_hip_ctx_lcp_dna_u32_dev", "kiss_hip_ctx_lcp_u8_dev", "kiss_hip_lcp_dna_u32",
    "kiss_hip_lcp_u8", "kiss_hip_fmi_query_mm_dev", "kiss_hip_fmi_query_mm_host",
    "kiss_hip_fmi8_sizes_for", "kiss_hip_fmi8_build_dev", "kiss_hip_fmi8_build_host", "kiss_hip_fmi8_query_dev",
    "kiss_hip_fmi8_query_host", "kiss_hip_fmi_seeds_dev", "kiss_hip_fmi_seeds_host",
    "kiss_hip_fmi_chain_dev", "kiss_hip_fmi_chain_host", "kiss_hip_fmi_align_dev", "kiss_hip_fmi_align_host",
    "kiss_hip_fmi_select_dev", "kiss_hip_fmi_select_host", "kiss_hip_fmi_pair_dev", "kiss_hip_fmi_pair_host",
    "kiss_hip_fmi_rescue_dev", "kiss_hip_fmi_rescue_host", "kiss_hip_fmi_aln_merge_dev", "kiss_hip_fmi_aln_merge_host",
]

# every symbol include/kiss_hip_reads.h declares (tests/test_reads_model.py)
READS_EXPORTED_SYMBOLS = [
    "kiss_hip_reads_parse_dev", "kiss_hip_reads_parse_host", "kiss_hip_reads_interleave_dev", "kiss_hip_reads_interleave_host",
]
# every symbol include/kiss_hip_reads_part.h declares (tests/test_reads_part_model.py)
READS_PART_EXPORTED_SYMBOLS = ["kiss_hip_reads_parse_part_dev", "kiss_hip_reads_parse_part_host"]
# every symbol include/kiss_hip_md.h declares (tests/test_fm_md_abi.py)
MD_EXPORTED_SYMBOLS = ["kiss_hip_fmi_md_dev", "kiss_hip_fmi_md_host"]
# every symbol include/kiss_hip_pileup.h declares (tests/test_fm_pileup_abi.py)
PILEUP_EXPORTED_SYMBOLS = ["kiss_hip_fmi_pileup_dev", "kiss_hip_fmi_pileup_host"]
PILEUP_PLANES = 8
# every symbol include/kiss_hip_sam.h declares (tests/test_fm_sam_abi.py)
SAM_EXPORTED_SYMBOLS = ["kiss_hip_fmi_sam_dev", "kiss_hip_fmi_sam_host"]
# every symbol include/kiss_hip_bam.h declares (tests/test_fm_bam_abi.py)
BAM_EXPORTED_SYMBOLS = ["kiss_hip_fmi_bam_dev", "kiss_hip_fmi_bam_host", "kiss_hip_bgzf_dev", "kiss_hip_bgzf_host"]
BGZF_BLOCK_DEFAULT, BGZF_BLOCK_MAX, BGZF_OVERHEAD, BGZF_EOF_BYTES = 65280, 65505, 31, 28
# every symbol include/kiss_hip_deflate.h declares (tests/test_deflate_abi.py)
DEFLATE_EXPORTED_SYMBOLS = ["kiss_hip_bgzf_deflate_dev", "kiss_hip_bgzf_deflate_host"]
# every symbol include/kiss_hip_bam_sort.h declares (tests/test_bam_sort_abi.py)
BAM_SORT_EXPORTED_SYMBOLS = ["kiss_hip_bam_sort_dev", "kiss_hip_bam_sort_host"]
BAM_RECORD_MIN = 36
# every symbol include/kiss_hip_bai.h declares (tests/test_bai_abi.py)
BAI_EXPORTED_SYMBOLS = ["kiss_hip_bai_dev", "kiss_hip_bai_host"]
BAI_PSEUDO_BIN, BAI_MAX_END = 37450, 1 << 29
# every symbol include/kiss_hip_markdup.h declares (tests/test_markdup_abi.py)
MARKDUP_EXPORTED_SYMBOLS = ["kiss_hip_bam_markdup_dev", "kiss_hip_bam_markdup_host"]
MARKDUP_MIN_QUAL_DEFAULT, MARKDUP_MAX_N_REF, BAM_FLAG_DUP = 15, (1 << 30) - 1, 0x400
# every symbol include/kiss_hip_insert.h declares (tests/test_fm_insert_abi.py)
INSERT_EXPORTED_SYMBOLS = ["kiss_hip_fmi_insert_dev", "kiss_hip_fmi_insert_host"]
INSERT_MAX = 65535
INSERT_OK = 1
READS_AUTO, READS_LINES, READS_FASTQ = 0, 1, 2
READS_NONE = 0xFFFFFFFFFFFFFFFF
