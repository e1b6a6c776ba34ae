/*
 * kiss_hip.h -- C ABI of libkiss_hip.so: the MI355X (gfx950) implementation of the
 * jhhung/kISS hot path (k-ordered induced suffix sorting of DNA + FM-index queries).
 *
 * The reference has no FFI: its seam is the compile-time C++ facade
 *   biovoltron::KISS1Sorter<size_type>::get_suffix_array_dna(S, k, num_threads)
 *     (include/biovoltron/algo/sort/kiss1_sorter.hpp:20-26) ->
 *   kiss::kiss1_suffix_array_dna<uint8_t,uint32_t>(S, SA, k, num_threads)
 *     (include/biovoltron/algo/sort/kiss1_core.hpp:229-268)
 * and, for queries,
 *   FMIndex<4,uint32_t,KISS1Sorter<uint32_t>>::get_range / get_offsets
 *     (include/biovoltron/algo/align/exact_match/fm_index.hpp:453-501,553-584).
 * The entry points below are what a cgo/ctypes/C++ binding for that path binds
 * (see INTEGRATION.md).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions: every function returns 0 (KISS_HIP_OK) or a negative kiss_hip_status.
 * No exceptions cross the ABI.  Host buffers are owned by the caller.  Device
 * workspace is owned by a kiss_hip_ctx.  A ctx is bound to one HIP device and must
 * not be used from two threads at once; distinct ctxs are independent.  Inside one process the device phases of
 * sorts on ONE device -- kiss_hip_*suffix_sort*, every kiss_hip_stage_* call, every phase of kiss_hip_multi_* -- queue up
 * behind a per-device lock (a sort fills the GPU, two at once gain nothing); uploads, downloads, verification and queries
 * run side by side.  The lock is per PROCESS: two processes may sort on one GPU at the same time, and so may the caller's own
 * kernels on other streams; the results are the same (what round 3 saw go wrong there was a 16-byte load at
 * an 8-byte aligned address in one kernel, gone since round 4; the near-end tie runs are verified before they are used,
 * kiss_hip_stats.tie_run_retries).
 *
 * Device entries (*_dev), two promises that hold for every one of them (tests/test_dev_stream_gpu.py,
 * tests/test_dev_placement_gpu.py):
 *   stream   : `void *stream` is the caller's hipStream_t, NULL = the ctx's own stream.  All work of the call is queued on it, so
 *              it is ordered behind what the caller has queued there, and the call returns after that work has completed.  A ctx
 *              keeps no caller's stream past the call that brought it: the entries that take no stream (kiss_hip_get_stats,
 *              kiss_hip_ctx_get_stage_outputs, kiss_hip_stage_local_lms, kiss_hip_stage_view, kiss_hip_stage_reserve, the debug
 *              hooks) run on the ctx's own stream and wait for no other.
 *   alignment: a device array needs the NATURAL ALIGNMENT OF ITS ELEMENT and no more, unless its entry says otherwise: byte
 *              arrays (texts, reads, patterns, raw file bytes, mismatches, bwt and occ2 of the DNA index) any address, uint16_t
 *              2, uint32_t 4, uint64_t 8 bytes; arrays of records whose fields are uint32_t (kiss_hip_fmi_seed, kiss_hip_chain,
 *              kiss_hip_chain_anchor, kiss_hip_aln, kiss_hip_hit, kiss_hip_pair) 4 bytes: records are read and written field
 *              by field.  The one array that needs more is the bwt of the byte index (kiss_hip_fmi8_view: 16 bytes, anything
 *              else is KISS_HIP_E_INVALID).  No entry reads a byte in front of or behind an input whose value reaches a result,
 *              and none writes outside the capacity it is given.  Every entry below repeats what it needs.
 */
#ifndef KISS_HIP_H
#define KISS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_VERSION 103 /* 0.1.3: kiss_hip_get_stats_sized, kiss_hip_has_hooks, kiss_hip_release_cached_contexts; from here on
                              * kiss_hip_stats only ever grows at its END (0.1.2 put three fields in the middle: callers built
                              * against 0.1.0 must be rebuilt) */

typedef enum kiss_hip_status {
    KISS_HIP_OK = 0,
    KISS_HIP_E_INVALID = -1,     /* bad argument (null pointer, n too large, unknown algo) */
    KISS_HIP_E_NO_DEVICE = -2,   /* no HIP device / device index out of range */
    KISS_HIP_E_HIP = -3,         /* a HIP runtime call failed (see kiss_hip_last_hip_error) */
    KISS_HIP_E_NOMEM = -4,       /* device or host allocation failed */
    KISS_HIP_E_UNSUPPORTED = -5, /* valid request outside the implemented range (documented) */
    KISS_HIP_E_INTERNAL = -6,    /* an internal invariant failed (bug) */
    KISS_HIP_E_IO = -7,          /* a file could not be opened / read */
    KISS_HIP_E_DEEP = -8         /* stage_sort only: exact order (k >= n) asked of the 32-bases-per-round path on ties
                                    deeper than 32768 bases; sort with a bounded k (512) and finish with stage_refine_exact
                                    (the single-call entry points do this by themselves) */
} kiss_hip_status;

/* Sorting algorithm selector; mirrors kISS::SortingAlgorithm
 * (include/utils/constant.hpp, command/suffix_sort.hpp:38-48). */
#define KISS_HIP_ALGO_PARALLEL_SORTING 0 /* KISS1: k-ordered LMS sort (kiss1_core.hpp)   */
#define KISS_HIP_ALGO_PREFIX_DOUBLING 1  /* KISS2: k >= n -> exact SA by rank doubling; bounded k -> the (deterministic)
                                            k-ordered SA of PARALLEL_SORTING: the reference's own bounded-k KISS2 output
                                            depends on its thread count, only the k-order property is defined */

/* the reference's size_type is uint32_t and EMPTY = 0xFFFFFFFF, so n + 19 < 2^32
 * (algo/sort/structs.hpp:94, constant.hpp:19-20).  Here 4096 less: several kernels run one thread per suffix-array
 * entry, a HIP grid holds fewer than 2^32 threads per dimension, and n + 1 rounded up to a workgroup has to stay
 * below that (found by tools/stress_verify.py at n = 2^32 - 20: "invalid configuration argument") */
#define KISS_HIP_MAX_N 4294963200ull

typedef struct kiss_hip_ctx kiss_hip_ctx;

/* Per-call statistics (filled by kiss_hip_get_stats after a sort on that ctx). */
typedef struct kiss_hip_stats {
    uint64_t n;              /* text length */
    uint64_t m;              /* number of LMS suffixes (without the sentinel) */
    uint32_t k;              /* requested order */
    uint32_t depth;          /* effective comparison depth D (0 = unbounded) */
    uint32_t lms_rounds;     /* 32-base refinement rounds executed */
    uint32_t induce_passes;  /* stable-partition passes executed by the two sweeps */
    uint64_t near_end;       /* LMS suffixes ranked by the near-end rule */
    uint64_t sort_item_rounds; /* sum over rounds of active LMS items */
    uint64_t big_item_rounds;  /* of those, items that went through the radix path in rounds >= 1 */
    float ms_total;          /* device time of the whole call (HIP events) */
    float ms_pack;           /* 2-bit packing */
    float ms_classify;       /* get_lms: classification + LMS extraction */
    float ms_lms_sort;       /* k-ordered LMS sort (all rounds) */
    float ms_place;          /* near-end ranking + merge + context gather */
    float ms_induce;         /* L and S sweeps */
    /* live per-kernel-class timing, only when profiling is enabled on the ctx */
    float ms_kernel[16];
    uint64_t launches_kernel[16];
    uint64_t items_kernel[16]; /* units processed (items for radix/induce, bases for classify) */
    /* PREFIX_DOUBLING (exact order) only: */
    uint64_t refine_items;    /* suffixes still tied after the bounded-depth phase (depth = refine_depth) */
    uint32_t refine_depth;    /* bases the bounded phase ordered by (0: doubling phase not used) */
    uint32_t doubling_rounds; /* rank-doubling rounds executed */
    float ms_refine;          /* device time of the doubling phase (included in ms_total) */
    /* host-pointer entry points only: wall-clock time of the two PCIe legs (the reference's timed region,
     * command/suffix_sort.hpp:57-61, is host S -> host SA) */
    float ms_h2d;             /* host S -> device */
    float ms_d2h;             /* device SA -> host */
    uint32_t refine_form;     /* exact order, how it was reached: 0 = doubling phase not used, 1 = rank doubling over the LMS
                               * suffixes before the induction (KISS2's order of things, kiss2_core.hpp:835-886), 2 = rank doubling
                               * over the whole suffix array after it (the LMS form gave up or is switched off) */
    /* kiss_hip_fmi_query_batch_dev with KISS_HIP_K_FM_QUERY timed: the two halves of ms_kernel[KISS_HIP_K_FM_QUERY] */
    float ms_fm_range;        /* backward search (get_range) */
    float ms_fm_locate;       /* get_offsets */
    /* appended in 0.1.3 (fields are only ever appended from here on) */
    uint32_t tie_run_retries; /* near-end placement: searches of the tie runs that failed their verification and were
                               * repeated (0 on an undisturbed device; see DESIGN.md 4.2 when it is not) */
    uint32_t pair_records;    /* LMS sort: tied segments of two members that round 0 wrote as pair records and one lane each
                               * decided; their members count in sort_item_rounds like every other tied item.  (Takes the
                               * place of the reserved word at the tail: the struct keeps its size; always 0 before.) */
} kiss_hip_stats;

/* kernel classes for ms_kernel[] / launches_kernel[] */
enum {
    KISS_HIP_K_PACK = 0,
    KISS_HIP_K_CLASSIFY = 1,
    KISS_HIP_K_RADIX_HIST = 2,
    KISS_HIP_K_RADIX_SCATTER = 3,
    KISS_HIP_K_SCAN = 4,
    KISS_HIP_K_KEYGATHER = 5,
    KISS_HIP_K_FLAG_COMPACT = 6,
    KISS_HIP_K_PLACE = 7,
    KISS_HIP_K_INDUCE_COUNT = 8,
    KISS_HIP_K_INDUCE_SCATTER = 9,
    KISS_HIP_K_INDUCE_SMALL = 10,
    KISS_HIP_K_FM_QUERY = 11,
    KISS_HIP_K_FM_BUILD = 12,
    KISS_HIP_K_SEGRANK = 13,
    KISS_HIP_K_GROUP_HEADS = 14, /* PREFIX_DOUBLING: tie detection over the bounded-depth SA */
    KISS_HIP_K_ISA = 15,         /* PREFIX_DOUBLING: inverse suffix array init / rank updates */
    KISS_HIP_K_NCLASSES = 16
};

int kiss_hip_version(void);
/* 0 for the shipped library.  1 for the hooks build of the same sources (libkiss_hip_hooks.so, -DKISS_HIP_HOOKS): test
 * infrastructure in which KISS_HIP_* environment variables switch A-B forms, tuning values, fault injection and tracing,
 * re-read at the start of every call.  The shipped library looks at the environment once per context, in
 * kiss_hip_ctx_create, and only for KISS_HIP_DEBUG (progress lines on stderr), KISS_HIP_XFER_THREADS and
 * KISS_HIP_PREFAULT_THREADS (host-side copy / page-fault helper threads): no variable changes a result path. */
int kiss_hip_has_hooks(void);
const char *kiss_hip_strerror(int status);
/* number of visible HIP devices (does not initialise a context) */
int kiss_hip_device_count(int *count);

/* ---- context: device workspace sized for texts up to max_n bases ------------- */
int kiss_hip_ctx_create(kiss_hip_ctx **out, int device, uint64_t max_n);
/* the same with the capacity of the per-LMS-suffix work arrays chosen by the caller instead of 0.32 max_n: a rank of a
 * sharded sort (ranks > 0 hold about 1/G of the LMS suffixes; the arrays regrow on demand).  0 = the default. */
int kiss_hip_ctx_create_sized(kiss_hip_ctx **out, int device, uint64_t max_n, uint64_t lms_capacity);
int kiss_hip_ctx_destroy(kiss_hip_ctx *ctx);
/* enable/disable per-kernel HIP-event timing (adds event overhead; off by default) */
int kiss_hip_ctx_set_profiling(kiss_hip_ctx *ctx, int enabled);
/* the same for chosen kernel classes only: bit i of class_mask = class KISS_HIP_K_* number i.  A pair of events
 * per launch costs a few microseconds of stream time; timing one class leaves the others back to back. */
int kiss_hip_ctx_set_profiling_mask(kiss_hip_ctx *ctx, uint64_t class_mask);
/* last hipError_t seen by this ctx (0 = hipSuccess) and its string */
int kiss_hip_last_hip_error(const kiss_hip_ctx *ctx, const char **msg);
int kiss_hip_get_stats(const kiss_hip_ctx *ctx, kiss_hip_stats *out);
/* the same for a caller built against an older (shorter) or newer (longer) kiss_hip_stats: copies min(bytes, sizeof the
 * library's struct) bytes and zero-fills the rest of the caller's -- fields are only appended (see KISS_HIP_VERSION) */
int kiss_hip_get_stats_sized(const kiss_hip_ctx *ctx, void *out, uint64_t bytes);
/* bytes of device workspace the ctx holds */
int kiss_hip_ctx_workspace_bytes(const kiss_hip_ctx *ctx, uint64_t *bytes);
/* the host-pointer entry points keep device-side copies of the caller's buffers between calls (5 bytes per base of
 * max_n, counted in workspace_bytes); this releases them (the next such call allocates them again) */
int kiss_hip_ctx_release_io_buffers(kiss_hip_ctx *ctx);

/* ---- suffix sorting --------------------------------------------------------- */
/*
 * Replaces KISS1Sorter<uint32_t>::get_suffix_array_dna(S, k, num_threads)
 * (kiss1_sorter.hpp:20-26) / KISS2Sorter (kiss2_sorter.hpp:20-26).
 *   S  : n bytes, each in 0..3 (A C G T), host memory.  Only the low 2 bits are used.
 *   k  : order; 0xFFFFFFFF (the CLI's -k -1) or any k >= n means the exact suffix array.
 *   SA : caller-allocated, n+1 entries; SA[0] = n (sentinel), SA[1..n] a permutation.
 * One-shot: uploads, sorts and downloads on a context the library keeps for `device` between one-shot calls (created by
 * the first call, grown when a longer text arrives; a chm13-size context is 80 GB of work arrays and the reference's
 * facade allocates its 5 bytes per base per call too, kiss1_core.hpp:243-257 -- at 26 bytes per base that is not free).
 * One one-shot call at a time per device; kiss_hip_release_cached_contexts() gives the memory back.
 * n == 0 yields SA = {0} (kiss1_core.hpp:237-238).
 */
int kiss_hip_suffix_sort_dna_u32(const uint8_t *S, uint64_t n, uint32_t k, int algo, uint32_t *SA, int device);
/* frees the contexts the one-shot calls keep (all devices); the next one-shot call creates one again */
int kiss_hip_release_cached_contexts(void);

/* Same, on an existing ctx with host buffers (upload + sort + download).  The device-side copies of S and SA belong
 * to the ctx (allocated on the first call, kept for the next ones).  Page-locked host buffers (hipHostMalloc /
 * hipHostRegister) travel at the PCIe rate, and for a bounded k the download of SA starts while the induction sweeps are
 * still running (finished stretches leave on a copy stream); pageable ones are moved by 8 threads through page-locked
 * bounce buffers of the ctx.  kiss_hip_get_stats reports the wall time of both legs (ms_h2d, ms_d2h). */
int kiss_hip_ctx_suffix_sort_dna_u32(kiss_hip_ctx *ctx, const uint8_t *S, uint64_t n, uint32_t k, int algo,
                                     uint32_t *SA);

/* Device-resident form: d_S (n bytes) and d_SA (n+1 u32) are DEVICE pointers on the
 * ctx's device.  stream is a hipStream_t (NULL = the ctx's own stream).  The call
 * returns after the work on `stream` has completed.
 * Alignment: d_S any address (16-byte loads are taken only where the address allows them), d_SA 4 bytes. */
int kiss_hip_ctx_suffix_sort_dna_u32_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, uint32_t k, int algo,
                                         uint32_t *d_SA, void *stream);

/* ---- several GPUs of one node driven by ONE process (`kiss_hip_opts{ngpus, device ids}`) ----
 * What a `suffix_sort_main`-shaped caller (reference include/command/suffix_sort.hpp:37-61) binds to use more than one
 * device: same arguments as kiss_hip_suffix_sort_dna_u32 plus the device list.  The LMS sort is sharded by key range
 * over the devices: devices[0] packs the text and the others pull it, every device classifies
 * a slice of the text, the LMS list is exchanged by direct peer copies over xGMI (every pair of devices its own link,
 * receiver keeps source order = text order), every device sorts its key range, devices[0] pulls the sorted pieces and
 * runs the induction (one dependency chain: it does not shard).  Host threads inside the call, one per device; no
 * fork, no exec.  A device may be listed more than once (two shares on one GPU: how the path is tested on a one-GPU
 * box).  ndev = 1 runs the same staged pipeline on one device and moves nothing. */
typedef struct kiss_hip_multi kiss_hip_multi;
typedef struct kiss_hip_multi_stats {
    uint64_t n, m;          /* text length, LMS suffixes */
    uint32_t ndev;
    uint32_t refine_depth;  /* != 0: exact order finished by rank doubling from this order on devices[0] */
    uint64_t piece[8];      /* far LMS suffixes sorted by each of the first 8 devices */
    /* wall-clock phases of the last call (barrier to barrier, i.e. the slowest device of each phase) */
    float ms_total, ms_pack, ms_classify, ms_partition, ms_exchange, ms_sort, ms_gather, ms_induce;
} kiss_hip_multi_stats;
int kiss_hip_multi_create(kiss_hip_multi **out, const int *devices, int ndev, uint64_t max_n);
int kiss_hip_multi_destroy(kiss_hip_multi *mc);
/* host S -> host SA (the reference's timed region); the SA is downloaded from devices[0] */
int kiss_hip_multi_suffix_sort_dna_u32(kiss_hip_multi *mc, const uint8_t *S, uint64_t n, uint32_t k, int algo, uint32_t *SA);
/* d_S (n bytes) and d_SA (n + 1 u32) are device pointers on devices[0] */
int kiss_hip_multi_suffix_sort_dna_u32_dev(kiss_hip_multi *mc, const uint8_t *d_S, uint64_t n, uint32_t k, int algo,
                                           uint32_t *d_SA);
int kiss_hip_multi_get_stats(const kiss_hip_multi *mc, kiss_hip_multi_stats *out);
/* the per-device context of share `rank` (statistics, profiling switches); owned by mc */
kiss_hip_ctx *kiss_hip_multi_ctx(kiss_hip_multi *mc, int rank);
/* one-shot: create, upload, sort, download, free */
int kiss_hip_suffix_sort_dna_u32_multi(const uint8_t *S, uint64_t n, uint32_t k, int algo, uint32_t *SA, const int *devices,
                                       int ndev);

/* ---- verification (device side; independent of the sort kernels: reads only the caller's text and SA) --------
 * Checks that d_SA (n+1 entries) is what the reference's own tests require of a k-ordered suffix array
 * (tests/kiss.cpp:26-28): SA[0] = n, a permutation of [0, n], and for every i >= 1
 *   S.substr(SA[i-1], k) <= S.substr(SA[i], k).
 * For k >= n the stronger linear-time proof of exactness is used instead (inverse SA; first character, then the rank
 * of the following suffix), which holds iff d_SA is THE suffix array.  Text bytes compare as unsigned values, so the
 * call serves both the DNA codes 0..3 and byte texts (kiss_hip_suffix_sort_u8).  `digest` is an order-sensitive
 * 64-bit sum that any host can recompute (kiss_hip_sa_digest_host).  order_violations is meaningful only when SA is a
 * permutation of [0, n] (the k >= n proof reads ranks that a non-permutation never wrote; ok = 0 either way, and
 * out_of_range, duplicates and sa0_ok are exact for every input).  Allocates its own scratch (n/8 bytes, plus
 * 4(n+1) bytes for k >= n) and frees it before returning; the ctx is only used for the device and the stream.
 * Alignment: d_S any address (the aligned 8-byte words around a text position are read and the bytes outside the text shifted
 * out: nothing outside [d_S, d_S + n) reaches the result), d_SA 4 bytes. */
typedef struct kiss_hip_verify_report {
    uint64_t n;
    uint32_t k;
    uint32_t exact;            /* 1: the k >= n proof was used */
    uint32_t ok;               /* 1: every check passed */
    uint32_t sa0_ok;           /* SA[0] == n */
    uint64_t out_of_range;     /* entries > n */
    uint64_t duplicates;       /* entries whose value occurred before */
    uint64_t order_violations; /* adjacent pairs in the wrong order */
    uint64_t first_violation;  /* smallest such index i (pair SA[i-1], SA[i]); meaningful if order_violations > 0 */
    uint64_t tied_pairs;       /* bounded k: adjacent pairs equal through k bases (their order is not constrained) */
    uint64_t digest;
    float ms;                  /* device time of the checks */
    uint32_t reserved_;
} kiss_hip_verify_report;
int kiss_hip_ctx_verify_sa_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, uint32_t k, const uint32_t *d_SA,
                               kiss_hip_verify_report *out, void *stream);
/* host helpers (no device): the digest above, and FNV-1a-64 over raw bytes (seed 0xcbf29ce484222325 to start, or the
 * previous return value to continue over the next chunk) */
uint64_t kiss_hip_sa_digest_host(const uint32_t *SA, uint64_t count);
uint64_t kiss_hip_fnv1a64_host(const void *data, uint64_t bytes, uint64_t seed);

/* Stage outputs of the LAST sort on this ctx, for stage-level parity tests
 * (get_lms: kiss_common.hpp:543-579; lms_suffix_direct_sort_dna: kiss1_core.hpp:24-145).
 *   lms_ascending : m entries (text order), may be NULL
 *   lms_sorted    : m entries (k-order, sentinel excluded), may be NULL
 *   counts        : 12 entries {count[c], s_type_count[c], lms_count[c]} c = A,C,G,T, may be NULL
 * Host pointers. */
int kiss_hip_ctx_get_stage_outputs(kiss_hip_ctx *ctx, uint32_t *lms_ascending, uint32_t *lms_sorted,
                                   uint64_t *counts);

/* ---- stage-level entry points for the sharded (one process per GPU) suffix sort: SURVEY.md section 8(e) --------
 * The exchange between ranks (histogram all-reduce, all-to-all of the LMS list, gather of the sorted pieces) is done
 * by the host with RCCL (torch.distributed); these calls do the arithmetic.  All data pointers are DEVICE pointers.
 *   stage_classify  : pack the whole text, emit the LMS suffixes of text positions [lo, hi) (ascending) with their
 *                     first 32-base key; counts13 = {count[c], s_count[c], lms_count[c] (c = A,C,G,T), far LMS count}
 *                     restricted to the window (sum over ranks = global)       (get_lms, kiss_common.hpp:543-579)
 *   stage_local_lms : sizes of that list (m_local, of which the first m_far_local are far) and a copy of it
 *   stage_key_hist  : histogram (u64[2^bits]) of the first `bits` key bits of count items
 *   stage_partition : stable partition by destination group g = #{splitters <= first `bits` key bits}
 *   stage_sort      : k-ordered sort of `count` far LMS suffixes (ascending position order inside equal keys on input)
 *                                                                        (lms_suffix_direct_sort_dna, kiss1_core.hpp:24-145)
 *   stage_induce    : near-end rule + placement + L/S induction from the concatenated sorted far list, the near-end
 *                     suffixes (ascending positions) and the global counts -> SA     (kiss1_core.hpp:259-267)
 * Alignment: natural alignment of the element for every array (d_S any address, uint32_t arrays 4, uint64_t arrays 8 bytes).  */
int kiss_hip_stage_classify(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, uint32_t k, uint64_t lo, uint64_t hi,
                            uint64_t counts13[13], void *stream);
int kiss_hip_stage_local_lms(kiss_hip_ctx *ctx, uint64_t *d_keys_out /* may be NULL: sizes only */,
                             uint32_t *d_pos_out, uint64_t *m_local, uint64_t *m_far_local);
/* Zero-copy hand-over between the stages: device pointers of the ctx's own work arrays (capacity = entries each holds).
 * A caller that passes these very pointers to the stage calls gets no copy in and no copy out:
 *   LOCAL_KEYS / LOCAL_POS  : what stage_classify emitted (u64 / u32), input of stage_partition, destination of the
 *                             exchange (the receiver's list) and input of stage_sort
 *   PART_KEYS / PART_POS    : output of stage_partition = source of the exchange
 *   SORTED / SORTED_CTX     : output of stage_sort (u32 / u32) = source of the gather; on the rank that runs the
 *                             induction also its destination and the input of stage_induce
 * kiss_hip_stage_reserve: makes the arrays hold lms_capacity entries; their CONTENTS ARE LOST when it has to regrow
 * (call it before stage_classify, or classify again).  The pointers change then: ask for the views afterwards.  It waits for
 * no stream but the ctx's own: the arrays a regrowth replaces are freed by the next call on the ctx that takes a stream (old
 * and new arrays exist side by side until then, both counted by kiss_hip_ctx_workspace_bytes; where they do not fit, the old
 * ones are freed first). */
enum {
    KISS_HIP_VIEW_LOCAL_KEYS = 0,
    KISS_HIP_VIEW_LOCAL_POS = 1,
    KISS_HIP_VIEW_PART_KEYS = 2,
    KISS_HIP_VIEW_PART_POS = 3,
    KISS_HIP_VIEW_SORTED = 4,
    KISS_HIP_VIEW_SORTED_CTX = 5
};
int kiss_hip_stage_view(kiss_hip_ctx *ctx, int which, void **d_ptr, uint64_t *capacity);
int kiss_hip_stage_reserve(kiss_hip_ctx *ctx, uint64_t lms_capacity);
int kiss_hip_stage_key_hist(kiss_hip_ctx *ctx, const uint64_t *d_keys, uint64_t count, int bits, uint64_t *d_hist,
                            void *stream);
int kiss_hip_stage_partition(kiss_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_pos, uint64_t count, int bits,
                             const uint32_t *splitters, int groups, uint64_t *d_keys_out, uint32_t *d_pos_out,
                             void *stream);
/* d_ctx_out / d_far_ctx (both optional): the context words the sort derives from the key payload, parallel to the
 * sorted positions (0 = not available, the induction gathers it from the text); shipping them with the pieces
 * spares rank 0 a random text gather per LMS suffix. */
int kiss_hip_stage_sort(kiss_hip_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_pos, uint64_t count, uint64_t n,
                        uint32_t k, uint32_t *d_sorted_out, uint32_t *d_ctx_out, void *stream);
int kiss_hip_stage_induce(kiss_hip_ctx *ctx, uint64_t n, uint32_t k, const uint32_t *d_far_sorted,
                          const uint32_t *d_far_ctx, uint64_t m_far, const uint32_t *d_near_pos, uint64_t near_count,
                          const uint64_t counts12[12], uint32_t *d_SA, void *stream);
/* stage_induce_exact: stage_induce for a list the stages have ordered by h0 bases (k = h0), with the exact-order finish of
 * kiss2_suffix_array_dna in front of the induction: rank doubling over the LMS suffixes, then ONE induction
 * (kiss2_core.hpp:835-886).  *exact_out = 1: d_SA is the exact suffix array; 0: it is h0-ordered and stage_refine_exact
 * has to finish the job (texts whose LMS suffixes are further apart than any window: DESIGN.md 2.3). */
int kiss_hip_stage_induce_exact(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, const uint32_t *d_far_sorted,
                                const uint32_t *d_far_ctx, uint64_t m_far, const uint32_t *d_near_pos, uint64_t near_count,
                                const uint64_t counts12[12], uint32_t *d_SA, void *stream, int *exact_out);
/* stage_refine_exact: turns the h0-ordered suffix array of the text packed by stage_classify (h0 = 512, say: the output of the
 * stages run with k = h0) into the exact suffix array by rank doubling over the tied suffixes -- what
 * kiss2_suffix_array_dna's prefix doubling yields for k = -1 (kiss2_core.hpp:728-797, 835-886).  Needs n >= 4 h0 + 1024. */
int kiss_hip_stage_refine_exact(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, uint32_t *d_SA, void *stream);

/* Test hooks (used by tests/ only): the library's stable LSD radix sort on bits [key_lo_bit, 64) of keys with a
 * 32-bit payload, and its exclusive u32 scan, run on caller data in host memory (count <= ctx LMS capacity). */
int kiss_hip_debug_radix_sort(kiss_hip_ctx *ctx, uint64_t *keys, uint32_t *pos, uint64_t count, int key_lo_bit);
/* The same sort in the form the tied-segment rounds and the stage partition call it: tuples (key, seg, pos), ordered by
 * seg first, then by bits [key_lo_bit & ~7, 64) of key; key_lo_bit = 64 sorts by seg alone.  key_lo_bit 0..64, seg_bits
 * 0..32, at most 12 passes of 8 bits in all (KISS_HIP_E_INVALID otherwise, and for count > ctx LMS capacity).
 * Contract of the callers, not checked: every seg value is below 2^seg_bits (bits above the sorted ones of the last
 * segment digit would take part in the order).  With seg_bits == 0 the sort never touches the segment column: `seg` may
 * be NULL, and otherwise comes back as the column of buffer 0, i.e. as it went in, which is where the callers read it.
 * flags bit 0: the positions go in through a buffer of their own that only the first pass reads (the sort's `first_pos`
 * form) while the first position buffer holds a poison value; not with key_lo_bit = 64 and seg_bits = 0, where no pass
 * runs that could read them (KISS_HIP_E_INVALID).  All three columns come back sorted, in host memory. */
int kiss_hip_debug_radix_sort_seg(kiss_hip_ctx *ctx, uint64_t *keys, uint32_t *seg, uint32_t *pos, uint64_t count,
                                  int key_lo_bit, int seg_bits, unsigned flags);
int kiss_hip_debug_scan_u32(kiss_hip_ctx *ctx, uint32_t *data, uint64_t count);
/* fault injection: from now on work-array allocations of this ctx above `bytes` fail with KISS_HIP_E_NOMEM (0 = off) */
int kiss_hip_debug_fail_alloc_over(kiss_hip_ctx *ctx, uint64_t bytes);
/* host only: the key-range rule of the multi-device sort (kiss_hip_multi_*) on a caller's histogram of `bins` entries:
 * groups - 1 splitters (group of a bin = number of splitters <= bin) and the resulting items per group */
int kiss_hip_debug_splitters(const uint64_t *hist, uint64_t bins, int groups, uint32_t *splitters_out,
                             uint64_t *group_counts_out);

/* ---- FM-index (biovoltron FMIndex<4,uint32_t,...>{LOOKUP_LEN=0}) --------------- */
/* Raw views of the arrays of the .fmi layout (fm_index.hpp:591-615).
 * For the *_dev call every pointer is a device pointer. */
typedef struct kiss_hip_fmi_view {
    uint64_t n_sa;        /* N = n + 1 */
    uint32_t cnt[4];      /* fm_index.hpp:296-307 */
    uint32_t pri;         /* SA index i with SA[i] == 0 (:324-325) */
    uint32_t sa_intv;     /* SA sampling interval (4) */
    const uint8_t *bwt;   /* ceil(N/4) bytes, dibit i at bits 2(i%4) of byte i/4 (:317-328) */
    const uint32_t *occ1; /* (N/256+1) x 4 (:280,283-301) */
    const uint8_t *occ2;  /* (N/16+1) x 4 (:281,286-287) */
    const uint32_t *sa;   /* sampled SA values, ceil(N/4) (:358-369) */
    const uint64_t *b;    /* bit i = (SA[i] % sa_intv == 0), ceil(N/64) words (:338-350) */
    const uint32_t *b_occ;/* N/64+1 (:339,352-356) */
} kiss_hip_fmi_view;

/*
 * Batched backward search + locate; replaces the per-pattern loop of
 * fmindex_query_main (include/command/fmindex_query.hpp:79-95):
 *   get_range(pattern) (fm_index.hpp:553-584) then get_offsets(beg,end) (:453-501).
 *   patterns : Q x L bytes in 0..3, row-major (device)
 *   beg,end  : Q entries each (device), the SA range per pattern
 *   hit_count_total, checksum : host pointers; sum of (end-beg) and sum of all hit positions
 *   offsets / offsets_index : optional device buffers; offsets_index has Q+1 entries
 *       (exclusive prefix of hit counts), offsets receives the hit positions of pattern q
 *       at [offsets_index[q], offsets_index[q+1]) in get_offsets order; pass NULL to skip.
 *   offsets_capacity : entries available in `offsets`
 * Alignment: natural alignment of the element -- patterns and the view's bwt (a pointer into a loaded .fmi will do) and occ2
 * any address; beg, end, offsets and the view's occ1, sa, b_occ 4 bytes; offsets_index and the view's b 8 bytes.
 */
int kiss_hip_fmi_query_batch_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L,
                                 uint64_t Q, uint32_t *beg, uint32_t *end, uint64_t *hit_count_total,
                                 uint64_t *checksum, uint32_t *offsets, uint64_t *offsets_index,
                                 uint64_t offsets_capacity, void *stream);

/*
 * FM-index construction from a text and its suffix array, both device resident
 * (FMIndex::build(ref, ori_sa), fm_index.hpp:390-451).  Output arrays are device
 * buffers sized as in kiss_hip_fmi_view; cnt/pri are written to the host struct.
 * Alignment: natural alignment of the element -- d_S, d_bwt, d_occ2 any address; d_SA, d_occ1, d_sa_sampled, d_b_occ 4 bytes;
 * d_b 8 bytes.  Exactly the sizes of kiss_hip_fmi_sizes_for are written, nothing behind them.
 */
int kiss_hip_fmi_build_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t sa_intv,
                           uint8_t *d_bwt, uint32_t *d_occ1, uint8_t *d_occ2, uint32_t *d_sa_sampled, uint64_t *d_b,
                           uint32_t *d_b_occ, uint32_t cnt_out[4], uint32_t *pri_out, void *stream);

/* Host-pointer forms of the two FM-index calls (create a ctx on `device`, upload, run, download, free): what a host
 * that does not link HIP binds -- the `kiss` CLI (kiss_amd/csrc/host/kiss_cli.cpp), cgo / ctypes callers.
 * kiss_hip_fmi_build_host: SA_or_null == NULL sorts with k = 32 first, like FMIndex::build(ref) (fm_index.hpp:379-387).
 * Array sizes for a text of n bases: kiss_hip_fmi_sizes_for (the .fmi layout of fm_index.hpp:591-615). */
typedef struct kiss_hip_fmi_sizes {
    uint64_t n_sa, bwt_bytes, occ1_entries, occ2_bytes, sa_entries, b_words, b_occ_entries;
} kiss_hip_fmi_sizes;
int kiss_hip_fmi_sizes_for(uint64_t n, kiss_hip_fmi_sizes *out);
int kiss_hip_fmi_build_host(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint8_t *bwt, uint32_t *occ1,
                            uint8_t *occ2, uint32_t *sa, uint64_t *b, uint32_t *b_occ, uint32_t cnt_out[4],
                            uint32_t *pri_out, int device);
int kiss_hip_fmi_query_batch_host(const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                                  uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum,
                                  uint32_t *offsets, uint64_t *offsets_index, uint64_t offsets_capacity, int device);

/* ---- FM-index, any instantiation: FMIndex<SA_INTV, uint32_t, ...>{.LOOKUP_LEN} ---------------------------------
 * SA_INTV in 1..KISS_HIP_FMI_MAX_SA_INTV, LOOKUP_LEN in 0..KISS_HIP_FMI_MAX_LOOKUP_LEN; anything else is
 * KISS_HIP_E_UNSUPPORTED.  (SA_INTV, LOOKUP_LEN) = (4, 0) is the index of the calls above, byte for byte.
 * .fmi layout (fm_index.hpp:591-646): cnt, pri, bwt, occ1, occ2, sa_, lookup_, then b_ and b_occ_ only if SA_INTV != 1.
 *   sa_     : SA_INTV == 1: the whole SA (N entries); else the values SA[i] with SA[i] % SA_INTV == 0 in row order.
 *   lookup_ : 4^LOOKUP_LEN + 1 entries; lookup_[K] = beg of the backward search of the K-th LOOKUP_LEN-mer (Codec::hash:
 *             last character in the low bits) from (0, N), lookup_[4^LOOKUP_LEN] = N (build_lookup, :238-270). */
#define KISS_HIP_FMI_MAX_SA_INTV 32u
#define KISS_HIP_FMI_MAX_LOOKUP_LEN 14u
typedef struct kiss_hip_fmi_view_ex {
    kiss_hip_fmi_view base;  /* base.sa_intv = SA_INTV; base.b / base.b_occ NULL when SA_INTV == 1 */
    uint32_t lookup_len;     /* LOOKUP_LEN */
    const uint32_t *lookup;  /* 4^lookup_len + 1 entries */
} kiss_hip_fmi_view_ex;
typedef struct kiss_hip_fmi_sizes_ex {
    kiss_hip_fmi_sizes base; /* sa_entries = ceil(N / SA_INTV); b_words = b_occ_entries = 0 when SA_INTV == 1 */
    uint64_t lookup_entries; /* 4^LOOKUP_LEN + 1 */
} kiss_hip_fmi_sizes_ex;
int kiss_hip_fmi_sizes_ex_for(uint64_t n, uint32_t sa_intv, uint32_t lookup_len, kiss_hip_fmi_sizes_ex *out);
/* build from a device text and its SA: the arrays of kiss_hip_fmi_build_dev plus lookup_ (d_lookup, lookup_entries);
 * d_b / d_b_occ may be NULL when sa_intv == 1.  Device times under KISS_HIP_K_FM_BUILD.
 * Alignment: as kiss_hip_fmi_build_dev; d_lookup 4 bytes. */
int kiss_hip_fmi_build_ex_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t sa_intv,
                              uint32_t lookup_len, uint8_t *d_bwt, uint32_t *d_occ1, uint8_t *d_occ2, uint32_t *d_sa,
                              uint64_t *d_b, uint32_t *d_b_occ, uint32_t *d_lookup, uint32_t cnt_out[4], uint32_t *pri_out,
                              void *stream);
/* get_range(pattern, stop_cnt) (fm_index.hpp:553-584) then get_offsets(beg, end) (:453-501) for every pattern; the
 * arguments of kiss_hip_fmi_query_batch_dev plus stop_cnt (0: no early stop; 0xFFFFFFFF: stop_cnt + 1 wraps to 0, never
 * stops) and offs (device, Q entries, may be NULL): get_range's third value, the characters left unmatched.
 * Alignment: as kiss_hip_fmi_query_batch_dev; offs and the view's lookup 4 bytes. */
int kiss_hip_fmi_query_ex_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view_ex *fmi, const uint8_t *patterns, uint32_t L,
                              uint64_t Q, uint32_t stop_cnt, uint32_t *beg, uint32_t *end, uint32_t *offs,
                              uint64_t *hit_count_total, uint64_t *checksum, uint32_t *offsets, uint64_t *offsets_index,
                              uint64_t offsets_capacity, void *stream);
/* host-pointer forms, as kiss_hip_fmi_build_host / kiss_hip_fmi_query_batch_host */
int kiss_hip_fmi_build_ex_host(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t sa_intv,
                               uint32_t lookup_len, uint8_t *bwt, uint32_t *occ1, uint8_t *occ2, uint32_t *sa, uint64_t *b,
                               uint32_t *b_occ, uint32_t *lookup, uint32_t cnt_out[4], uint32_t *pri_out, int device);
int kiss_hip_fmi_query_ex_host(const kiss_hip_fmi_view_ex *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                               uint32_t stop_cnt, uint32_t *beg, uint32_t *end, uint32_t *offs, uint64_t *hit_count_total,
                               uint64_t *checksum, uint32_t *offsets, uint64_t *offsets_index, uint64_t offsets_capacity,
                               int device);

/* ---- FM-index: batched search with up to KISS_HIP_FMI_MAX_MISMATCHES substitutions (no reference counterpart) --------
 * For a batch of Q patterns of one length L and a bound e = max_mismatches, a hit of pattern P is a text position p in
 * [0, n - L] whose Hamming distance to P, d = #{j : S[p + j] != P[j]}, is at most e (substitutions only; pattern bytes are
 * used & 3).  Backward search that branches, then locate, then a sort into the one canonical order.
 *   counts     : Q x (e + 1) u32: counts[q * (e + 1) + j] = hits of pattern q with exactly j mismatches.
 *   positions / mismatches / index : optional (all three or none; none: capacity = 0).  index has Q + 1 entries; the hits of
 *                pattern q are (positions[i], mismatches[i]) for i in [index[q], index[q + 1]) in ASCENDING position.
 *   capacity   : entries available in positions / mismatches.  Smaller than the total: KISS_HIP_E_INVALID with the totals
 *                in report->hits (call again with room, as with kiss_hip_fmi_query_batch_dev).
 * Domain.  COUNTS are defined for L <= the order of the suffix array the index was built from: 32 for the default build
 * (kiss_hip_fmi_build_host with SA_or_null == NULL), any L for an index built from the exact suffix array -- the domain of
 * get_range.  POSITIONS are defined only for an index built from the EXACT suffix array (k = 0xFFFFFFFF): on a k-ordered
 * one the LF walk of a tied row lands on another suffix's row.  The walk is bounded (at most SA_INTV - 1 steps, never from the
 * primary row), so the call returns whatever arrays it is handed; a row that reaches no sampled row inside the bound is
 * counted in walk_failures and the call returns KISS_HIP_E_INVALID, promising nothing about positions.  THE BOUND DOES NOT
 * CATCH EVERY NON-EXACT INDEX: a tied row can reach a sampled row of the wrong suffix in time; walk_failures == 0 proves
 * nothing.  Build with the exact order when positions are wanted.
 * Limits: max_mismatches > KISS_HIP_FMI_MAX_MISMATCHES or sa_intv outside 1..32: KISS_HIP_E_UNSUPPORTED.  L == 0 or a
 * required pointer NULL: KISS_HIP_E_INVALID.  L > n or Q == 0: KISS_HIP_OK, no hits.  The hits of a call are sorted in the
 * ctx's LMS work arrays (their contents are lost; about 0.32 x the ctx's max_n entries): more hits than those hold is
 * KISS_HIP_E_UNSUPPORTED with the totals in the report -- split the batch.
 * Device times: report->ms_* always; the kernels also count under KISS_HIP_K_FM_QUERY when that class is profiled. */
#define KISS_HIP_FMI_MAX_MISMATCHES 3u
typedef struct kiss_hip_fmi_mm_report {
    uint64_t Q;
    uint32_t L, max_mismatches;
    uint64_t hits[4];        /* by number of mismatches */
    uint64_t ranges;         /* SA ranges (leaves) the search emitted */
    uint64_t lf_pairs;       /* fm_lf2-equivalents ((range, base) pairs) evaluated by the search: the denominator of its rate */
    uint64_t walk_failures;  /* rows that reached no sampled row within SA_INTV - 1 steps (index not from an exact SA) */
    uint64_t checksum;       /* sum of all hit positions (0 without positions) */
    float ms_total, ms_search, ms_locate, ms_sort;
} kiss_hip_fmi_mm_report;
/* every pointer except report is a device pointer; report may be NULL.  Alignment: natural alignment of the element -- patterns,
 * mismatches and the view's bwt and occ2 any address; counts, positions and the view's occ1, sa, b_occ 4 bytes; index and the
 * view's b 8 bytes. */
int kiss_hip_fmi_query_mm_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                              uint32_t max_mismatches, uint32_t *counts, uint32_t *positions, uint8_t *mismatches,
                              uint64_t *index, uint64_t capacity, kiss_hip_fmi_mm_report *report, void *stream);
/* the same with host pointers, as kiss_hip_fmi_query_ex_host (creates a ctx on `device`, uploads, runs, downloads) */
int kiss_hip_fmi_query_mm_host(const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                               uint32_t max_mismatches, uint32_t *counts, uint32_t *positions, uint8_t *mismatches,
                               uint64_t *index, uint64_t capacity, kiss_hip_fmi_mm_report *report, int device);

/* ---- General alphabet (bytes): exact suffix array ---------------------------------
 * Replaces KISS1Sorter::get_suffix_array -> kiss1_suffix_array (kiss1_core.hpp:270-311), reachable only from the
 * reference's tests / experiments.  For that entry only the k-order property is defined (its comparator has no
 * index tie-break); the exact suffix array (shorter suffix first on a tie, SA[0] = n, n + 1 entries) satisfies it for
 * every k.  7-character keys + rank doubling over all suffixes; no induction.  n <= ctx max_n.
 * Alignment (_dev): d_S any address, d_SA 4 bytes. */
int kiss_hip_suffix_sort_u8(const uint8_t *S, uint64_t n, uint32_t *SA, int device);
int kiss_hip_ctx_suffix_sort_u8_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, uint32_t *d_SA, void *stream);

/* ---- LCP array of an exact suffix array (DNA and bytes) -------------------------------------------------------
 * Input: a text S of n symbols and its EXACT suffix array SA (n + 1 entries, SA[0] = n: the convention of
 * kiss_hip_suffix_sort_dna_u32 / kiss_hip_suffix_sort_u8).  Output: LCP, n + 1 u32, LCP[0] = 0 and for i >= 1 the length
 * of the longest common prefix of suffixes SA[i-1] and SA[i] (so LCP[1] = 0: suffix SA[0] is the empty one).
 *   _dna_u32: symbols 0..3, only the low 2 bits are used (as the sort);  _u8: the full byte range.
 * SA[0] != n or an entry > n: KISS_HIP_E_INVALID (checked on the device, nothing is written to LCP).  An SA that is a
 * permutation but not the exact order -- e.g. the k-ordered SA of PARALLEL_SORTING -- gives UNSPECIFIED values (the
 * permuted-LCP relation the computation rests on holds for the exact order only); the call still stays inside its arrays
 * and returns KISS_HIP_OK.  n = 0 gives LCP = {0}.
 * Device time goes into the report below, never into kiss_hip_stats.  The calls take the per-device lock of the sorts.
 * Work arrays: the ctx's own (the packed text, the context words, the LMS work arrays): after an exact sort of the same n
 * on the ctx an LCP call allocates nothing; on a fresh ctx it allocates what that sort would have. */
typedef struct kiss_hip_lcp_report {
    uint64_t n;
    uint64_t irreducible;     /* positions whose lcp was computed directly (the rest follow from their left neighbour) */
    uint64_t long_pairs;      /* of those, pairs sent on from the one-lane compare to the cooperative one */
    uint64_t lcp_sum;         /* sum of LCP[1..n] */
    uint32_t max_lcp;
    uint32_t reserved_;
    float ms_total;           /* device time of the call (HIP events) */
    float ms_phi;             /* text packing / padded copy + Phi scatter with the SA checks */
    float ms_short;           /* irreducible test + one-lane compares */
    float ms_long;            /* cooperative compares (one wave per pair, then the whole grid per pair) */
    float ms_scan_gather;     /* max-scan to PLCP + LCP[i] = PLCP[SA[i]] */
    uint32_t reserved2_;
} kiss_hip_lcp_report;
/* device-resident: d_S (n symbols), d_SA (n + 1), d_LCP (n + 1) on the ctx's device; d_LCP may be d_SA (the LCP then
 * replaces the SA); report may be NULL.  stream: as kiss_hip_ctx_suffix_sort_dna_u32_dev; returns after the work is done.
 * Alignment: d_S any address (no byte behind d_S + n reaches a result), d_SA and d_LCP 4 bytes. */
int kiss_hip_ctx_lcp_dna_u32_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP,
                                 kiss_hip_lcp_report *report, void *stream);
int kiss_hip_ctx_lcp_u8_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP,
                            kiss_hip_lcp_report *report, void *stream);
/* host-pointer one-shots on the cached per-device context (as kiss_hip_suffix_sort_dna_u32): SA_or_null == NULL sorts in
 * exact order first and writes that SA to SA_out (n + 1 entries; SA_out may be NULL as well).  With an SA given, SA_out
 * (if not NULL) receives a copy of it. */
int kiss_hip_lcp_dna_u32(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t *SA_out, uint32_t *LCP,
                         int device);
int kiss_hip_lcp_u8(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t *SA_out, uint32_t *LCP, int device);

/* ---- FASTA / plain-text input parsed on the device (replaces read_sequence, include/utils/io.hpp:6-18, and the
 * `c % 4` of command/suffix_sort.hpp:33; record rules of biovoltron/file_io/fasta.hpp:117-151) ------------------
 * The file is FASTA iff its first byte is '>'.  Header lines are dropped, every other byte except '\n' is a base:
 * A/a 0, C/c 1, G/g 2, T/t 3, anything else 0 (the reference maps it to 4 and reduces % 4; that includes '\r').
 * kiss_hip_ctx_parse_text_dev: raw file bytes already in device memory -> codes in d_S (capacity >= bytes), *n_out
 *   = number of bases.  The ctx must have been created with max_n >= bytes / 1000.
 * kiss_hip_ctx_load_text_file: streams the file through pinned buffers into device memory and parses it there;
 *   *d_S_out is a device buffer owned by the caller (kiss_hip_free_dev).  No base is touched on the host.
 * kiss_hip_alloc_dev / kiss_hip_copy_to_host / kiss_hip_free_dev: for hosts that do not link HIP (the CLI, ctypes);
 *   they act on the current device of the calling thread (the one the last ctx call selected).
 * Alignment (kiss_hip_ctx_parse_text_dev): d_raw and d_S any address.  Only the first *n_out bytes of d_S are defined; nothing is
 * written behind d_S + bytes. */
int kiss_hip_file_size(const char *path, uint64_t *bytes);
int kiss_hip_ctx_parse_text_dev(kiss_hip_ctx *ctx, const uint8_t *d_raw, uint64_t bytes, uint8_t *d_S, uint64_t *n_out,
                                void *stream);
int kiss_hip_ctx_load_text_file(kiss_hip_ctx *ctx, const char *path, uint8_t **d_S_out, uint64_t *n_out);
int kiss_hip_alloc_dev(void **d_out, uint64_t bytes);
int kiss_hip_copy_to_host(void *dst, const void *d_src, uint64_t bytes);
int kiss_hip_free_dev(void *p);

/* ---- FM-index over a byte text (values 0..255; no reference counterpart: its -g commands are a TODO) ---------------------
 * Built from a text S of n bytes and its EXACT suffix array (kiss_hip_suffix_sort_u8: N = n + 1 entries, SA[0] = n).  A hit of
 * a pattern P of length L >= 1 is a position p in [0, n - L] with S[p .. p + L) == P; bytes compare as unsigned values and
 * overlapping hits all count.  Every result is a function of (S, patterns) alone, whatever sa_intv.
 * Arrays, with nblk = N / 256 + 1 and nsb = N / 65536 + 1:
 *   C     : 257 u32, C[c] = 1 + #{bytes of S smaller than c}
 *   map   : 256 bytes, the dense code (0 .. sigma - 1, in value order) of a byte value that occurs in S, 0xFF otherwise
 *           (a value v is absent iff C[v + 1] == C[v]: at sigma = 256 the code 255 is a code like the others)
 *   bwt   : nblk * 256 bytes, 16-byte aligned; row i holds S[SA[i] - 1], the primary row (SA[i] == 0) and the rows >= N hold 0
 *   occ1  : sigma x nsb u32, symbol-major: occurrences of code c in bwt[0, 65536 j), the primary row left out
 *   occ2  : sigma x nblk u16, symbol-major: occurrences of code c in bwt[65536 (j / 256), 256 j)
 *   sa / b / b_occ : as in kiss_hip_fmi_view_ex (sa_intv == 1: the whole SA, b = b_occ = NULL)
 * For the *_dev calls every pointer of the view is a device pointer, for the *_host calls a host pointer. */
typedef struct kiss_hip_fmi8_view {
    uint64_t n_sa;        /* N = n + 1 */
    uint32_t pri;         /* row i with SA[i] == 0 */
    uint32_t sa_intv;     /* 1..KISS_HIP_FMI_MAX_SA_INTV */
    uint32_t sigma;       /* distinct byte values of S (0 for n = 0) */
    uint32_t reserved_;
    const uint32_t *C;
    const uint8_t *map;
    const uint8_t *bwt;
    const uint32_t *occ1;
    const uint16_t *occ2;
    const uint32_t *sa;
    const uint64_t *b;
    const uint32_t *b_occ;
} kiss_hip_fmi8_view;
typedef struct kiss_hip_fmi8_sizes {
    uint64_t n_sa, bwt_bytes, occ1_entries, occ2_entries, sa_entries, b_words, b_occ_entries;
} kiss_hip_fmi8_sizes;
/* host-only arithmetic.  sa_intv outside 1..32: KISS_HIP_E_UNSUPPORTED; sigma > 256 or n > KISS_HIP_MAX_N: KISS_HIP_E_INVALID */
int kiss_hip_fmi8_sizes_for(uint64_t n, uint32_t sa_intv, uint32_t sigma, kiss_hip_fmi8_sizes *out);
typedef struct kiss_hip_fmi8_report {
    uint64_t Q;
    uint64_t hits;           /* sum of end - beg */
    uint64_t lf_pairs;       /* (range, byte) pairs the search evaluated: the denominator of its rate */
    uint64_t walk_failures;  /* rows that reached no sampled row within sa_intv - 1 steps (index not from an exact SA) */
    uint64_t checksum;       /* sum of all hit positions (0 without positions) */
    float ms_total, ms_search, ms_locate, ms_sort;
} kiss_hip_fmi8_report;
/* Build from a device text and its exact suffix array.  The arrays depend on sigma, which only the text knows, so the call has
 * two forms: d_bwt == NULL is the census -- it writes *sigma_out (and d_C / d_map when given) and nothing else; otherwise the
 * arrays are sized by kiss_hip_fmi8_sizes_for(n, sa_intv, sigma_capacity), sigma_capacity >= the text's sigma (smaller:
 * KISS_HIP_E_INVALID with *sigma_out set), and occ1 / occ2 are laid out for *sigma_out rows.  d_b / d_b_occ may be NULL when
 * sa_intv == 1.  n = 0 builds the index of one row.  Device times under KISS_HIP_K_FM_BUILD.
 * Alignment: d_bwt 16 bytes (anything else: KISS_HIP_E_INVALID before anything is launched, nothing written); every other array
 * the natural alignment of its element -- d_S, d_map any address; d_occ2 2 bytes; d_SA, d_C, d_occ1, d_sa, d_b_occ 4 bytes; d_b 8
 * bytes. */
int kiss_hip_fmi8_build_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t sa_intv,
                            uint32_t sigma_capacity, uint32_t *d_C, uint8_t *d_map, uint8_t *d_bwt, uint32_t *d_occ1,
                            uint16_t *d_occ2, uint32_t *d_sa, uint64_t *d_b, uint32_t *d_b_occ, uint32_t *sigma_out,
                            uint32_t *pri_out, void *stream);
/* host pointers (creates a ctx on `device`, uploads, runs, downloads); SA_or_null == NULL sorts with kiss_hip_suffix_sort_u8's
 * kernels first; bwt == NULL: the census, as above */
int kiss_hip_fmi8_build_host(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t sa_intv, uint32_t sigma_capacity,
                             uint32_t *C, uint8_t *map, uint8_t *bwt, uint32_t *occ1, uint16_t *occ2, uint32_t *sa, uint64_t *b,
                             uint32_t *b_occ, uint32_t *sigma_out, uint32_t *pri_out, int device);
/* Batched backward search + locate over a RAGGED batch: Q patterns concatenated in `patterns`, pattern q =
 * patterns[pat_index[q], pat_index[q + 1]) (pat_index: Q + 1 u64, strictly increasing: every pattern has L >= 1).
 *   beg, end   : Q u32 each, the SA range; count = end - beg; no hits: beg == end
 *   hit_count_total, checksum : host pointers (may be NULL): sum of the counts, sum of all positions (0 without positions)
 *   positions / index : optional (both or none; none: capacity = 0).  index has Q + 1 u64 (exclusive prefix of the counts);
 *                the hits of pattern q are positions[index[q] .. index[q + 1]) in ASCENDING position.
 *   capacity   : entries available in positions.  Smaller than the total: KISS_HIP_E_INVALID with the total in
 *                *hit_count_total and report->hits (call again with room).
 * A zero-length pattern, a pat_index that decreases, a required pointer NULL or a bwt that is not 16-byte aligned:
 * KISS_HIP_E_INVALID.  L > n or Q == 0: KISS_HIP_OK, no hits.  sa_intv outside 1..32: KISS_HIP_E_UNSUPPORTED.  The hits of a
 * call are sorted in the ctx's LMS work arrays (their contents are lost): more hits than those hold is
 * KISS_HIP_E_UNSUPPORTED with the totals reported -- split the batch.  A row that reaches no sampled row (an index that was not
 * built from an exact suffix array) is counted in walk_failures and the call returns KISS_HIP_E_INVALID.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY when that class is profiled.
 * Alignment: the view's bwt 16 bytes (see above: KISS_HIP_E_INVALID otherwise, decided from the address, no output touched);
 * every other array the natural alignment of its element -- patterns and the view's map any address; occ2 2 bytes; beg, end,
 * positions and the view's C, occ1, sa, b_occ 4 bytes; pat_index, index and the view's b 8 bytes. */
int kiss_hip_fmi8_query_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi8_view *fmi, const uint8_t *patterns, const uint64_t *pat_index,
                            uint64_t Q, uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum,
                            uint32_t *positions, uint64_t *index, uint64_t capacity, kiss_hip_fmi8_report *report, void *stream);
int kiss_hip_fmi8_query_host(const kiss_hip_fmi8_view *fmi, const uint8_t *patterns, const uint64_t *pat_index, uint64_t Q,
                             uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum, uint32_t *positions,
                             uint64_t *index, uint64_t capacity, kiss_hip_fmi8_report *report, int device);

/* ---- FM-index: maximal exact match seeds of a batch of reads (no reference counterpart) -------------------------------
 * Every other query of this header takes whole patterns.  This one takes reads that need not occur in the text anywhere in
 * full and reports which stretches of them do, and where: what a read mapper chains and extends.
 * Text S: n bases as indexed.  A read R has L >= 1 bytes; the values 0..3 are bases, ANY OTHER VALUE IS "NO BASE": no match
 * contains it (this is how N is carried -- on purpose NOT the `& 3` of the pattern calls above).  The complement of a
 * no-base is itself.  The batch is ragged, as with kiss_hip_fmi8_query_dev: read q = reads[read_index[q], read_index[q + 1]).
 * Virtual reads: without both_strands V = Q and virtual read v is read v; with it V = 2 Q, virtual read 2 q is read q and
 * 2 q + 1 its reverse complement R'[j] = 3 - R[L - 1 - j].  All coordinates of a virtual read are in that virtual read.
 * Matching statistics: for an end e in 1..L, ms[e] is the largest l <= min(e, max_len or e) such that R[e - l, e) occurs in
 * S (0 if R[e - 1] does not occur); start[e] = e - ms[e], non-decreasing in e.
 * Seeds: e ends a seed iff ms[e] >= min_len and (e == L or start[e + 1] > start[e]); the seed is (start[e], ms[e]).  These
 * are the substrings of R of at most max_len bases that occur in S and are contained in no other such substring, of length
 * >= min_len; with max_len == 0 (no cap) the super-maximal exact matches.  The seeds of a virtual read come out in ascending
 * e, which is strictly ascending start.
 *   min_len >= 1; max_len: 0 = no cap; max_occ: 0 = no limit.
 *   ms         : optional, `bases` u32 (bases = sum of the virtual read lengths): ms of end e of virtual read v at
 *                vbase[v] + e - 1, vbase = the exclusive prefix sum of the virtual read lengths.
 *   seeds / seed_index : seed_index has V + 1 u64; the seeds of virtual read v are seeds[seed_index[v] .. seed_index[v + 1]).
 *                sa_beg / sa_end: the backward-search range of the seed string, count = sa_end - sa_beg.
 *   seed_capacity : entries available in seeds; `bases` always suffices.
 *   positions / pos_index : optional (both or none; none: pos_capacity = 0).  pos_index has seeds + 1 u64; the occurrences of
 *                seed s -- every p with S[p, p + len) == the seed -- are positions[pos_index[s] .. pos_index[s + 1]) in
 *                ASCENDING order.  Only seeds with count <= max_occ are located (all when max_occ == 0); a seed over the
 *                limit has an empty segment and still reports its range.
 * A capacity smaller than the total: KISS_HIP_E_INVALID with the totals in the report (seeds, positions; call again with
 * room).  Other KISS_HIP_E_INVALID: a required pointer NULL, min_len == 0, a zero-length read or a read_index that
 * decreases.  Q == 0: KISS_HIP_OK, seed_index[0] = 0.
 * Domain (that of kiss_hip_fmi_query_mm_dev).  RANGES and ms are defined when max_len is at most the order of the suffix
 * array the index was built from: max_len in 1..32 on the default build, any max_len including 0 on an index built from the
 * exact suffix array.  POSITIONS are defined only on an index built from the EXACT suffix array; the locate walk is bounded
 * as there, walk_failures > 0 gives KISS_HIP_E_INVALID, and walk_failures == 0 proves nothing.
 * Limits (KISS_HIP_E_UNSUPPORTED): sa_intv outside 1..32; a read of 2^31 bytes or more; more ends in one call than the ctx
 * scans -- bases must be below 2^31 and below about 0.32 x the ctx's max_n; more located positions than the ctx's LMS work
 * arrays hold (about 0.32 x max_n entries; their contents are lost), with the totals in the report -- split the batch.
 * A kiss_hip_fmi_view_ex is taken so that any SA_INTV works; lookup may be NULL (the search does not use it: the ends have
 * no common length).  Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
typedef struct kiss_hip_fmi_seed { uint32_t start, len, sa_beg, sa_end; } kiss_hip_fmi_seed;
typedef struct kiss_hip_fmi_seed_report {
    uint64_t Q, V, bases;      /* bases = ends searched (sum of virtual read lengths) */
    uint64_t seeds, located_seeds, positions, lf_pairs, walk_failures, checksum;
    uint32_t max_ms, reserved_;
    float ms_total, ms_search, ms_compact, ms_locate, ms_sort;
} kiss_hip_fmi_seed_report;
/* every pointer except fmi and report is a device pointer (the arrays of the view too).  Alignment: natural alignment of the
 * element -- reads and the view's bwt and occ2 any address; ms, positions, seeds (records of uint32_t) and the view's occ1, sa,
 * b_occ 4 bytes; read_index, seed_index, pos_index and the view's b 8 bytes. */
int kiss_hip_fmi_seeds_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view_ex *fmi, const uint8_t *reads, const uint64_t *read_index,
                           uint64_t Q, uint32_t min_len, uint32_t max_len, uint32_t max_occ, int both_strands, uint32_t *ms,
                           kiss_hip_fmi_seed *seeds, uint64_t *seed_index, uint64_t seed_capacity, uint32_t *positions,
                           uint64_t *pos_index, uint64_t pos_capacity, kiss_hip_fmi_seed_report *report, void *stream);
/* the same with host pointers, as kiss_hip_fmi_query_mm_host (creates a ctx on `device`, uploads, runs, downloads) */
int kiss_hip_fmi_seeds_host(const kiss_hip_fmi_view_ex *fmi, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            uint32_t min_len, uint32_t max_len, uint32_t max_occ, int both_strands, uint32_t *ms,
                            kiss_hip_fmi_seed *seeds, uint64_t *seed_index, uint64_t seed_capacity, uint32_t *positions,
                            uint64_t *pos_index, uint64_t pos_capacity, kiss_hip_fmi_seed_report *report, int device);

/* ---- FM-index: the seeds of a read chained into candidate loci (no reference counterpart) -----------------------------
 * The seeds call ends where a mapper begins: it says where every seed occurs, not which occurrences belong together.  This
 * call groups them.  The result is a function of the input arrays and the parameters alone; it needs no index and no text.
 * Input: the output of kiss_hip_fmi_seeds_dev -- seeds with seed_index (V + 1 u64), positions with pos_index (seeds + 1
 * u64).  The ANCHORS of virtual read v are the triples (r, t, l) = (start, position, len), one for every position of every
 * seed of v; a seed with an empty position segment (over max_occ) contributes none.  An anchor's SLOT is its index in
 * `positions`; the anchors of one v are contiguous in slots.
 * Order: the anchors of v are numbered 0 .. A - 1 in ascending (t, slot).
 * Parameters (kiss_hip_chain_params, all u32; in parentheses the defaults of Python and the command line): max_gap (5000),
 * band (500), gap_cost (2), max_lookback (64; 0 = no bound), min_score (40).  max_gap and band are at most 2^31 - 1,
 * gap_cost at most 65535; anything else is KISS_HIP_E_INVALID.
 * Predecessors: anchor j may precede anchor i when all of these hold: j < i; if max_lookback != 0, i - j <= max_lookback;
 * with dt = t_i - t_j and dr = r_i - r_j (signed), dt > 0 and dr > 0; dt <= max_gap and dr <= max_gap;
 * g = |dt - dr| <= band.  The score through j is f(j) + min(l_i, dr, dt) - floor(g * gap_cost / 8), in signed 64-bit
 * arithmetic that cannot wrap.
 * Score: take the maximum, in lexicographic order, of the pair (l_i, 0) and the pairs (score through j, j + 1) over all
 * allowed j.  f(i) is its first component; pred(i) its second minus 1, none if that is 0.  So on equal scores the nearest
 * predecessor in the order wins, and a predecessor that only ties with starting afresh still wins.  root(i) = i if pred(i)
 * is none, else root(pred(i)); depth(i) = 0 if pred(i) is none, else depth(pred(i)) + 1.
 * Chains: the pred pointers form a forest, and every tree yields at most one chain.  Its end is the anchor of the tree with
 * the largest f, the smallest i on ties; the chain is the path from the root to that end; it is reported iff
 * f(end) >= min_score.  The chains of v come in ascending root number, that is ascending (tbeg, slot).  The record has
 * score = f(end), anchors = depth(end) + 1, (rbeg, tbeg) from the root, rend = r_end + l_end, tend = t_end + l_end.
 * KNOWN PROPERTY: one chain per tree means that two loci closer together than max_gap, and inside the band, come out as ONE
 * chain; there are no secondary chains inside a tree.
 * Outputs: chains with chain_index (V + 1 u64: the chains of v are chains[chain_index[v] .. chain_index[v + 1])); optionally
 * (both or neither) chain_anchors with anchor_index (chains + 1 u64): the anchors of each chain from root to end.
 * A capacity smaller than the total: KISS_HIP_E_INVALID with the totals in the report (chains, chain_anchors; call again
 * with room) -- the seeds call's convention.  Other KISS_HIP_E_INVALID: a required pointer NULL, a seed_index or pos_index
 * that decreases, a located seed with len == 0 (checked on the device while the anchors are expanded).  V == 0: KISS_HIP_OK,
 * chain_index[0] = 0.
 * The u32 fields of a record hold the low 32 bits of their values.  Nothing is lost on the output of the seeds call, where
 * r + l is at most a read length (below 2^31), so every score is below 2^32; t + l must not pass 2^32 - 1.
 * Limits (KISS_HIP_E_UNSUPPORTED): V of 2^31 or more; more anchors in one call than the ctx's LMS work arrays hold (about
 * 0.32 x max_n entries; their contents are lost) or than it scans, with the total in the report -- split the batch.
 * seed_index[0] and pos_index[seed_index[0]] need not be 0: seeds and positions are indexed as the indexes say.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
typedef struct kiss_hip_chain_params { uint32_t max_gap, band, gap_cost, max_lookback, min_score; } kiss_hip_chain_params;
typedef struct kiss_hip_chain { uint32_t score, anchors, rbeg, rend, tbeg, tend; } kiss_hip_chain;
typedef struct kiss_hip_chain_anchor { uint32_t rstart, tpos, len; } kiss_hip_chain_anchor;
typedef struct kiss_hip_chain_report {
    uint64_t V, anchors, chains, chain_anchors;
    uint64_t dp_pairs;         /* the (i, j) candidates with j inside the lookback: sum over i of min(i, max_lookback) */
    uint32_t max_anchors, best_score; /* the largest A of a virtual read; the largest score of a reported chain */
    float ms_total, ms_sort, ms_dp, ms_emit; /* sort: expand, order, gather; emit: tree ends, scan, totals, records */
} kiss_hip_chain_report;
/* every pointer except params and report is a device pointer.  Alignment: natural alignment of the element -- seeds, chains
 * and chain_anchors (records of uint32_t, read and written field by field) and positions 4 bytes; seed_index, pos_index,
 * chain_index and anchor_index 8 bytes. */
int kiss_hip_fmi_chain_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, uint64_t V,
                           const uint32_t *positions, const uint64_t *pos_index, const kiss_hip_chain_params *params,
                           kiss_hip_chain *chains, uint64_t *chain_index, uint64_t chain_capacity, kiss_hip_chain_anchor *chain_anchors,
                           uint64_t *anchor_index, uint64_t anchor_capacity, kiss_hip_chain_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_lcp_dna_u32: uploads, runs, downloads) */
int kiss_hip_fmi_chain_host(const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, uint64_t V, const uint32_t *positions,
                            const uint64_t *pos_index, const kiss_hip_chain_params *params, kiss_hip_chain *chains,
                            uint64_t *chain_index, uint64_t chain_capacity, kiss_hip_chain_anchor *chain_anchors, uint64_t *anchor_index,
                            uint64_t anchor_capacity, kiss_hip_chain_report *report, int device);

/* ---- FM-index: the chains of a read aligned to the text, banded (no reference counterpart) ---------------------------
 * A chain is a guess: "read bases [rbeg, rend) lie near text bases [tbeg, tend)".  This call turns every chain into a
 * base-level, banded, affine-gap LOCAL alignment: score, ends, counts and optionally the operations.  One definition in
 * integers; tests/fm_align_model.py restates it.
 * Input: the text S -- n bytes of 0..3, the array the index was built from (the index does not keep it); reads /
 * read_index / Q / both_strands exactly as in kiss_hip_fmi_seeds_dev (virtual read 2 q + 1 is the reverse complement, read
 * in place; a no-base is its own complement); chains with chain_index (V + 1 u64) as kiss_hip_fmi_chain_dev wrote them.
 * C = chain_index[V] - chain_index[0]; alignment a (0 <= a < C) belongs to chains[chain_index[0] + a], whose virtual read
 * is the v with chain_index[v] <= chain_index[0] + a < chain_index[v + 1] (chain_index[0] need not be 0).
 * Parameters (kiss_hip_align_params, all u32; in parentheses the defaults of Python and the command line): match (1),
 * mismatch (4), gap_open (6), gap_extend (1), band (32).  A gap of g bases costs gap_open + g * gap_extend.  match >= 1, the
 * four scores <= 65535, band <= 2^31 - 1; anything else is KISS_HIP_E_INVALID.
 * Band: for a chain of virtual read v (read R of L bases), in signed 64-bit: d0 = tbeg - rbeg, d1 = tend - rend,
 * dlo = min(d0, d1) - band, dhi = max(d0, d1) + band, B = dhi - dlo + 1.  Only these four fields of the chain record are
 * used; no other field is validated and any values are defined.  Cell (i, j), 1 <= i <= L, 1 <= j <= n, compares R[i - 1]
 * with S[j - 1]; it EXISTS iff dlo <= j - i <= dhi.  B > KISS_HIP_ALIGN_MAX_BAND: the chain is not aligned, flags =
 * KISS_HIP_ALN_BAND_TOO_WIDE, every other field 0 except band.
 * Recurrence (o = gap_open, e = gap_extend): s(x, y) = match if x == y <= 3; -1 if x is a no-base (it never matches);
 * -mismatch otherwise.
 *   E(i, j) = max(H(i, j - 1) - o - e, E(i, j - 1) - e) if cell (i, j - 1) exists, else -inf   (consumes text: a deletion)
 *   F(i, j) = max(H(i - 1, j) - o - e, F(i - 1, j) - e) if cell (i - 1, j) exists, else -inf   (consumes read: an insertion)
 *   H(i, j) = max(0, Hd + s(R[i - 1], S[j - 1]), E(i, j), F(i, j)), Hd = H(i - 1, j - 1) if that cell exists, else 0 (it is
 *   on the same diagonal, so it is missing only at i = 1 or j = 1).
 * Equivalently: the best H is the largest score over all lattice paths of M / I / D steps all of whose points lie on the
 * diagonals dlo..dhi inside [0, L] x [0, n].
 * Best cell: the largest H; ties: the smallest i, then the smallest j.  Largest H = 0: not aligned, all fields 0 except
 * band, flags = 0.
 * Traceback, a function of the final H / E / F values only.  In state H at (i, j): stop if i = 0, j = 0 or H = 0; otherwise
 * take the diagonal if H = Hd + s, else go to state E if H = E, else to state F.  In state E: emit D; go back to state H if
 * E(i, j) = H(i, j - 1) - o - e (opening is preferred over extending), else stay in E; then j -= 1.  State F mirrors E with I
 * and i -= 1.
 * Record (kiss_hip_aln, 12 u32): score, flags, rbeg, rend, tbeg, tend (half-open, 0-based, in the virtual read and the
 * text), matches, mismatches (no-base columns count here), ins, del (bases), gaps (maximal runs of I or D), band (= B,
 * saturated to u32).  So rend - rbeg = matches + mismatches + ins and tend - tbeg = matches + mismatches + del.
 * CIGAR, optional (cigar with cigar_index, both or neither): u32 ops len << 4 | op, op 0 = M (match or mismatch), 1 = I,
 * 2 = D; maximal runs in read order, CSR over the alignments (cigar_index has C + 1 u64).  No clip ops: the clips are rbeg
 * and L - rend.
 * KNOWN PROPERTY: the alignment is local within the band; it is NOT forced through the chain's anchors.  A chain that wanders
 * outside [min(d0, d1) - band, max(d0, d1) + band] between its ends is aligned inside the band only.
 * aln_capacity < C or cigar_capacity < the total of ops: KISS_HIP_E_INVALID with the totals in the report (chains,
 * cigar_ops), nothing written; call again with room.  Other KISS_HIP_E_INVALID: a required pointer NULL, a chain_index or
 * read_index that decreases, a zero-length read.  V == 0 or C == 0: KISS_HIP_OK, cigar_index[0] = 0.
 * Limits (KISS_HIP_E_UNSUPPORTED): n above KISS_HIP_MAX_N; V of 2^31 or more; a read of the batch with L * match >= 2^30;
 * more DP cells -- `cells`, the sum of L * B over the chains that are not too wide -- than the traceback store of the call
 * holds.  That store, one byte per cell, comes out of the ctx's pooled scratch, and its limit is
 * KISS_HIP_ALIGN_CELLS_PER_N x the ctx's max_n cells; the total is in the report -- split the batch.
 * All score arithmetic is signed 32-bit and cannot wrap under these limits.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
#define KISS_HIP_ALIGN_MAX_BAND 1024u
#define KISS_HIP_ALIGN_CELLS_PER_N 16u
#define KISS_HIP_ALN_BAND_TOO_WIDE 1u
typedef struct kiss_hip_align_params { uint32_t match, mismatch, gap_open, gap_extend, band; } kiss_hip_align_params;
typedef struct kiss_hip_aln {
    uint32_t score, flags, rbeg, rend, tbeg, tend, matches, mismatches, ins, del, gaps, band;
} kiss_hip_aln;
typedef struct kiss_hip_align_report {
    uint64_t V, chains, aligned, too_wide; /* aligned = chains - too_wide: the chains whose band was filled */
    uint64_t cells, cigar_ops;
    uint32_t best_score, max_band;         /* the largest score; the largest B of a chain that was not too wide */
    float ms_total, ms_dp, ms_trace, ms_emit; /* trace: the walk back and the op counts; emit: scan, totals, records, ops */
} kiss_hip_align_report;
/* every pointer except params and report is a device pointer.  Alignment: natural alignment of the element -- text and reads
 * any address; chains and alns (records of uint32_t, read and written field by field) and cigar 4 bytes; read_index,
 * chain_index and cigar_index 8 bytes. */
int kiss_hip_fmi_align_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index,
                           uint64_t Q, int both_strands, const kiss_hip_chain *chains, const uint64_t *chain_index,
                           const kiss_hip_align_params *params, kiss_hip_aln *alns, uint64_t aln_capacity, uint32_t *cigar,
                           uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_align_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host) */
int kiss_hip_fmi_align_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            int both_strands, const kiss_hip_chain *chains, const uint64_t *chain_index,
                            const kiss_hip_align_params *params, kiss_hip_aln *alns, uint64_t aln_capacity, uint32_t *cigar,
                            uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_align_report *report, int device);

/* ---- FM-index: the alignments of a read turned into its mappings: primary, secondary, MAPQ (no reference counterpart) ---
 * The align call writes one record per CHAIN.  Two neighbouring chains routinely give the same alignment (see the two KNOWN
 * PROPERTY notes above), both strands may reach one locus, a repeat gives many.  This call says which alignment is the
 * mapping, which are the same locus twice, which are repeats and how far the best can be trusted, and which reads did not
 * map.  One definition in integers; tests/fm_select_model.py restates it.  The result is a function of the input arrays and
 * the parameters alone; it needs no index, no text and no reads.
 * Input: alns with chain_index (V + 1 u64) exactly as kiss_hip_fmi_align_dev wrote and read them: C = chain_index[V] -
 * chain_index[0], and alignment a (0 <= a < C, alns[a]) belongs to the virtual read v that contains chain_index[0] + a.
 * read_index (Q + 1 u64): only the lengths L_q = read_index[q + 1] - read_index[q] are used.  Q and both_strands: V = 2 Q or
 * Q; read q owns the virtual reads 2 q and 2 q + 1, or just q, so its alignments are one contiguous stretch of alns.
 * bounds, optional: R + 1 u64, bounds[0] = 0, strictly ascending -- the starts of the R records of the text, bounds[R] = n.
 * NULL (R is then ignored): one record and no boundary rule.
 * Parameters (kiss_hip_select_params, all u32; in parentheses the defaults of Python and the command line): min_score (30),
 * overlap (128, in 256ths; at most 256), mapq_coef (120; at most 65535), mapq_max (60; at most 255), max_hits (0 = all).
 * Strand and frames: alignment a of virtual read v is on the reverse strand iff both_strands and v is odd.  Its text interval
 * is [tbeg, tend).  Its read interval in the frame of the ORIGINAL read is [rbeg, rend) on the forward strand and
 * [L - rend, L - rbeg) on the reverse strand.  All interval arithmetic is signed 64-bit; the length |X| of an interval is
 * max(0, x1 - x0), so a record with tend < tbeg overlaps nothing.
 * Candidates: alignment a of read q is a candidate iff flags == 0, score >= max(min_score, 1) and, if bounds is given, its
 * record rho (the largest rho with bounds[rho] <= tbeg) has rho < R and tend <= bounds[rho + 1].  An alignment that fails only
 * the third condition is SPANNING: counted in the report, not a candidate (a tbeg at or past bounds[R] too).
 * Order: the candidates of a read in descending score, then ascending a.
 * Overlap: ov(X, Y) = max(0, min(x1, y1) - max(x0, y0)); X and Y "overlap by more than the share" iff
 * ov * 256 > overlap * min(|X|, |Y|), in u64.  So overlap = 256 never holds and overlap = 0 holds for any common base.
 * Walk -- greedy, and the order is part of the definition.  Go through the candidates in order, K = the kept ones so far:
 *   1. candidate c is REDUNDANT iff some k in K has c's strand and their text intervals overlap by more than the share: c is
 *      dropped and counted.  Only KEPT alignments make others redundant.
 *   2. otherwise c is kept as hit number h = |K| of its read.  Let g be the HEAD in K with the smallest hit number whose read
 *      interval overlaps c's by more than the share.  If g exists, c is SECONDARY, head(c) = g, g.n_sec += 1, g.sub =
 *      max(g.sub, score(c)).  Otherwise c is a HEAD, head(c) = h; the first head of a read is its PRIMARY, every later head
 *      is SUPPLEMENTARY.
 * MAPQ: a secondary has 0.  A head with s = score and s2 = sub (0 when n_sec = 0) has min(mapq_max, floor(mapq_coef *
 * (s - s2) / s)), in u64: a head whose best secondary ties it has 0, a head with no secondary min(mapq_max, mapq_coef).
 * Cap: with max_hits != 0 only the hits with number < max_hits are written; sub, n_sec and mapq are computed before the cap;
 * head points at an earlier hit or at the hit itself, so it stays valid.
 * Output: hits with hit_index (Q + 1 u64, CSR over the READS, not the virtual reads), in hit-number order.  Record
 * kiss_hip_hit, 8 u32: aln (a), flags, mapq, score, sub, n_sec, head, ref (rho; 0 without bounds); sub and n_sec of a secondary
 * are 0.  A read with no candidate has an empty segment.
 * Report: Q, V, alignments (C), candidates, spanning, redundant, hits (written, that is after the cap), heads (among the
 * written hits), mapped (reads with at least one hit), max_candidates (the largest candidate count of a read), times.
 * hit_capacity below the total: KISS_HIP_E_INVALID with the totals in the report, nothing written; call again with room.
 * A read keeps no more hits than it has alignments, so hit_capacity = C always suffices and no sizing call is needed.
 * hits and alns need no more than the 4-byte alignment of their fields: records are read and written field by field.
 * Other KISS_HIP_E_INVALID: a required pointer NULL, a chain_index or read_index that decreases, a zero-length read, bounds
 * with bounds[0] != 0 or not strictly ascending (or R == 0), a parameter over its limit.  Q == 0 or C == 0: KISS_HIP_OK,
 * hit_index all zero.
 * Limits (KISS_HIP_E_UNSUPPORTED): V of 2^31 or more, C of 2^32 or more; more alignments in one call than the ctx's LMS work
 * arrays hold (about 0.32 x max_n entries; their contents are lost: the alignments are sorted there) -- split the batch.
 * KNOWN PROPERTY: the walk of a read is sequential in its candidates and parallel over the kept hits, 64 per step: a read with
 * c candidates of which k are kept costs about c * ceil(k / 64) steps of one wave.  A read with thousands of candidates is
 * slow, and finite.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
#define KISS_HIP_HIT_REVERSE 1u
#define KISS_HIP_HIT_SECONDARY 2u
#define KISS_HIP_HIT_SUPPLEMENTARY 4u
typedef struct kiss_hip_select_params { uint32_t min_score, overlap, mapq_coef, mapq_max, max_hits; } kiss_hip_select_params;
typedef struct kiss_hip_hit { uint32_t aln, flags, mapq, score, sub, n_sec, head, ref; } kiss_hip_hit;
typedef struct kiss_hip_select_report {
    uint64_t Q, V, alignments, candidates, spanning, redundant, hits, heads, mapped;
    uint32_t max_candidates, reserved_;
    float ms_total, ms_sort, ms_walk, ms_emit; /* sort: checks, keys, the radix sort; emit: scan, totals, records */
} kiss_hip_select_report;
/* every pointer except params and report is a device pointer.  Alignment: alns and hits 4 bytes (above); chain_index,
 * read_index, bounds and hit_index 8 bytes. */
int kiss_hip_fmi_select_dev(kiss_hip_ctx *ctx, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index,
                            uint64_t Q, int both_strands, const uint64_t *bounds, uint64_t R, const kiss_hip_select_params *params,
                            kiss_hip_hit *hits, uint64_t *hit_index, uint64_t hit_capacity, kiss_hip_select_report *report,
                            void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host) */
int kiss_hip_fmi_select_host(const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index, uint64_t Q,
                             int both_strands, const uint64_t *bounds, uint64_t R, const kiss_hip_select_params *params,
                             kiss_hip_hit *hits, uint64_t *hit_index, uint64_t hit_capacity, kiss_hip_select_report *report,
                             int device);

/* ---- FM-index: the mappings of two mates paired: proper pairs, pair MAPQ, TLEN (no reference counterpart) ---------------
 * The select call treats every read on its own.  This call takes what it wrote for a batch in which reads 2 p and 2 p + 1
 * are mate 1 and mate 2 of pair p (so Q is even, P = Q / 2) and says which combination of their hits is the pair.  One
 * definition in integers; tests/fm_pair_model.py restates it.  The result is a function of the input arrays and the
 * parameters alone: no index, no text, no reads, no bounds (a hit carries ref) and no both_strands (a hit carries
 * KISS_HIP_HIT_REVERSE).  ONLY forward-then-reverse libraries (FR: the mates face each other) are supported.
 * Input: hits with hit_index (Q + 1 u64 over the READS) as kiss_hip_fmi_select_dev wrote them: the hits of read q are
 * hits[hit_index[q] .. hit_index[q + 1]), and a hit's number is its place in that segment.  alns with aln_count: hit.aln
 * indexes alns; only tbeg and tend are read.
 * Parameters (kiss_hip_pair_params, all u32; in parentheses the defaults of Python and the command line, which are part of the
 * definition and not measurements): ins_min (0), ins_max (1000), ins_mean (400), pen_coef (8, in 256ths of a score point per
 * base of deviation; at most 65535), pen_max (20; at most 65535), mapq_coef (120; at most 65535), mapq_max (60; at most 255).
 * All interval arithmetic is signed 64-bit, as in select.
 * Eligible: the hits of a read with head == 0 (the primary and its secondaries) and tbeg < tend.  Supplementary heads and
 * their secondaries never pair.  x and y are hit numbers of mate 1 and mate 2.
 * Concordant: a combination (x, y) of eligible hits is concordant iff their ref fields are equal, their strands differ, and
 * with f the forward hit and r the reverse one f.tbeg <= r.tbeg, f.tend <= r.tend and T = r.tend - f.tbeg has
 * ins_min <= T <= ins_max.
 * Pair score: S(x, y) = max(1, score(x) + score(y) - min(pen_max, floor(|T - ins_mean| * pen_coef / 256))).
 * Best: the largest S; ties go to the smallest x, then the smallest y.  sub1 = the largest S over the concordant (x', y')
 * with x' != x, 0 if there is none; sub2 the same with y' != y.  (Select has dropped the duplicates of a locus, so another
 * x' is another locus of mate 1.)
 * MAPQ of mate m in a proper pair: max(mapq of its chosen hit, min(mapq_max, floor(mapq_coef * (S - sub_m) / S))), in u64.
 * So a mate in a repeat whose other copies have no concordant partner gets the full value, and a chosen hit that select
 * called secondary (mapq 0) is lifted by the pair.  tlen = T.
 * No concordant combination: each mate keeps its hit number 0, or KISS_HIP_PAIR_NONE when its segment is empty; score = the sum
 * of the scores of the mates that mapped; sub1 = sub2 = 0; the MAPQs are those of the hits (0 for an unmapped mate); tlen =
 * max(tend) - min(tbeg) of the two hits (0 if that is negative) when both mapped with equal ref, else 0.
 * Record kiss_hip_pair, 10 u32: hit1, hit2 (indices into hits: hit_index[q] + hit number, or KISS_HIP_PAIR_NONE), flags, tlen,
 * score, sub1, sub2, mapq1, mapq2, n_conc (the concordant combinations, saturated at 2^32 - 1).  Flags: PROPER, MATE1_MAPPED,
 * MATE2_MAPPED (the segment is not empty), SAME_REF (both mapped and the chosen hits have equal ref), PROMOTED1, PROMOTED2 (the
 * chosen hit is not hit number 0).  Exactly P records are written, in pair order: no capacity, no sizing call.  pairs, hits
 * and alns need no more than the 4-byte alignment of their fields: records are read and written field by field.
 * BAD INPUT: a pair one of whose hits -- any hit of the two segments -- has aln outside [0, aln_count) or a score of 2^30 or
 * more (select writes neither) gets a record that is all zero but for flags = KISS_HIP_PAIR_BAD_INPUT, and counts nowhere in
 * the report but in bad_input.  So nothing is read outside alns whatever the arrays hold, and S fits u32.
 * Report: P, eligible (hits), combinations (the sum of |E1| * |E2|), concordant, proper (pairs), promoted (mates), lifted
 * (mates whose MAPQ is above their hit's), bad_input (pairs), max_combinations (the largest |E1| * |E2|), times.
 * KISS_HIP_E_INVALID: a required pointer NULL, Q odd, a hit_index that decreases, ins_min > ins_max, a parameter over its
 * limit; pairs is untouched then.  Q == 0: KISS_HIP_OK.  KISS_HIP_E_UNSUPPORTED: Q of 2^32 or more, hit_index[Q] of
 * 2^32 - 1 or more.
 * KNOWN PROPERTY: one wave per pair; the hits of mate 2 live in the lanes, 64 at a time, and the eligible hits of mate 1 are
 * handed to them one by one, twice (the best, then sub1 / sub2 / n_conc).  A pair with |E1| eligible hits of mate 1 and n2
 * hits of mate 2 costs about 2 * |E1| * ceil(n2 / 64) steps of one wave: cap it with select's max_hits.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
#define KISS_HIP_PAIR_NONE 0xFFFFFFFFu
#define KISS_HIP_PAIR_PROPER 1u
#define KISS_HIP_PAIR_MATE1_MAPPED 2u
#define KISS_HIP_PAIR_MATE2_MAPPED 4u
#define KISS_HIP_PAIR_SAME_REF 8u
#define KISS_HIP_PAIR_PROMOTED1 16u
#define KISS_HIP_PAIR_PROMOTED2 32u
#define KISS_HIP_PAIR_BAD_INPUT 64u
typedef struct kiss_hip_pair_params { uint32_t ins_min, ins_max, ins_mean, pen_coef, pen_max, mapq_coef, mapq_max; } kiss_hip_pair_params;
typedef struct kiss_hip_pair { uint32_t hit1, hit2, flags, tlen, score, sub1, sub2, mapq1, mapq2, n_conc; } kiss_hip_pair;
typedef struct kiss_hip_pair_report {
    uint64_t P, eligible, combinations, concordant, proper, promoted, lifted, bad_input, max_combinations;
    float ms_total, ms_check, ms_pair; /* check: hit_index looked at once by the host; pair: the one kernel */
    uint32_t reserved_;
} kiss_hip_pair_report;
/* every pointer except params and report is a device pointer.  Alignment: hits, alns and pairs 4 bytes (above); hit_index 8
 * bytes. */
int kiss_hip_fmi_pair_dev(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q,
                          const kiss_hip_aln *alns, uint64_t aln_count, const kiss_hip_pair_params *params, kiss_hip_pair *pairs,
                          kiss_hip_pair_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host); hits holds hit_index[Q]
 * records */
int kiss_hip_fmi_pair_host(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                           uint64_t aln_count, const kiss_hip_pair_params *params, kiss_hip_pair *pairs,
                           kiss_hip_pair_report *report, int device);

/* ---- FM-index: the missing mate looked for near its partner: the rescue plan (no reference counterpart) -----------------
 * Every stage before the pair call treats a read on its own, so a mate without a seed has no alignment although its partner
 * says within a few hundred bases where it must lie.  This call turns the pairs that are not proper into WINDOWS next to the
 * hits of either mate, written as chain records that kiss_hip_fmi_align_dev takes as they are; kiss_hip_fmi_aln_merge_dev
 * (below) then puts the alignments of those chains behind the reads' own, and the select and pair calls run once more:
 *   pass 1: seeds -> chain -> align -> select -> pair;  rescue: plan -> align (the rescue chains) -> merge;
 *   pass 2: select -> pair on the merged alignments.
 * One definition in integers; tests/fm_rescue_model.py restates it.  The result is a function of the input arrays and the
 * parameters alone: no index, no text and no read is looked at.  FR libraries only, as the pair call.
 * Input: pairs (P = Q / 2 records as kiss_hip_fmi_pair_dev wrote them; only flags is read); hits with hit_index (Q + 1 u64 over
 * the READS) and alns with aln_count exactly as the pair call reads them; read_index (Q + 1 u64; only the lengths are used); n,
 * the length of the text; bounds with R, optional, as in kiss_hip_fmi_select_dev, with bounds[R] <= n (NULL: one record
 * [0, n), a hit's ref is ignored).
 * Parameters (kiss_hip_rescue_params, all u32; in parentheses the defaults of Python and the command line): ins_min (0),
 * ins_max (1000) -- the pair call's --, max_anchors (4; at least 1), min_anchor_score (0), max_width (960; at least 1 and at
 * most KISS_HIP_ALIGN_MAX_BAND).  All interval arithmetic is signed 64-bit, as in select and pair.
 * Which pairs: pair p is rescued iff its flags has neither KISS_HIP_PAIR_PROPER nor KISS_HIP_PAIR_BAD_INPUT.
 * Anchors: for mate m of such a pair (read q = 2 p + m of L bases; the other read is o = 2 p + 1 - m) a hit of read o QUALIFIES
 * iff head == 0, score >= min_anchor_score and either aln >= aln_count (its interval cannot be read: see bad anchors) or
 * tbeg < tend of alns[aln].  The anchors of mate m are the first max_anchors qualifying hits of o, in hit order.  Both mates
 * of a pair are rescued, each from the other's hits.
 * Bad anchors: an anchor with aln >= aln_count, or, with bounds, ref >= R, gives no window and is counted in bad_input (it
 * still is one of the max_anchors).  So nothing is read outside alns or bounds whatever the arrays hold.
 * Window of an anchor A (tbeg, tend of its alignment, record rho = ref): the diagonals d at which the whole mate, laid end to
 * end as [d, d + L), would be concordant with A under the pair call's rule.
 *   A forward (the mate is virtual read 2 q + 1): dmin = max(A.tbeg + ins_min, A.tend, A.tbeg + L) - L,
 *                                                 dmax = A.tbeg + ins_max - L.
 *   A reverse (the mate is virtual read 2 q):     dmin = A.tend - ins_max, dmax = min(A.tend - ins_min, A.tbeg, A.tend - L).
 *   Clip to the record: dmin = max(dmin, lo), dmax = min(dmax, hi - L), [lo, hi) = [bounds[rho], bounds[rho + 1]) or [0, n).
 *   dmin > dmax: no window, counted in `empty` (a read longer than its record always ends here).
 * Split: a window of W = dmax - dmin + 1 diagonals is cut into k = ceil(W / max_width) pieces; piece j (0 <= j < k) covers
 * the diagonals dmin + floor(j W / k) .. dmin + floor((j + 1) W / k) - 1.  Windows with k > 1 are counted in `split`.  The
 * align call's own band widens every piece on both sides, so neighbouring pieces overlap and select drops the duplicate; with
 * max_width = 960 and band = 32 a piece is exactly KISS_HIP_ALIGN_MAX_BAND diagonals wide.
 * Chain record of a piece [a, b] (kiss_hip_chain): score = the anchor's score, anchors = 0 (no real chain has none), rbeg = 0,
 * rend = L, tbeg = a, tend = b + L: the align call sees d0 = a and d1 = b.
 * Output: chains with chain_index (2 Q + 1 u64 over the VIRTUAL reads of both strands, chain_index[0] = 0); inside a virtual
 * read the anchors in hit order, the pieces of an anchor ascending.  origin, optional: one u32 per chain, the anchor's index
 * into hits.
 * chain_capacity below the total: KISS_HIP_E_INVALID with the totals in the report, nothing written; call again with room.
 * Q * max_anchors * ceil((ins_max - ins_min + 1) / max_width) always suffices.
 * Report: P, pairs_planned (pairs with at least one chain), anchors (bad and empty ones included), chains, split, empty,
 * bad_input (anchors), max_chains (of a pair), times.
 * Other KISS_HIP_E_INVALID: a required pointer NULL, Q odd, a hit_index that decreases, a read_index that does not ascend (a
 * zero-length read), ins_min > ins_max, max_anchors or max_width out of range, bounds with bounds[0] != 0, not strictly
 * ascending, bounds[R] > n or R == 0.  Q == 0: KISS_HIP_OK, chain_index[0] = 0.  KISS_HIP_E_UNSUPPORTED: Q of 2^31 or more, n
 * above KISS_HIP_MAX_N, hit_index[Q] of 2^32 - 1 or more, more reads than the ctx's scratch scans.
 * pairs, hits, alns and chains need no more than the 4-byte alignment of their fields.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
typedef struct kiss_hip_rescue_params { uint32_t ins_min, ins_max, max_anchors, min_anchor_score, max_width; } kiss_hip_rescue_params;
typedef struct kiss_hip_rescue_report {
    uint64_t P, pairs_planned, anchors, chains, split, empty, bad_input, max_chains;
    float ms_total, ms_check, ms_count, ms_emit; /* count: the counting walk and the scan; emit: the writing walk */
} kiss_hip_rescue_report;
/* every pointer except params and report is a device pointer.  Alignment: pairs, hits, alns, chains (above) and origin 4
 * bytes; hit_index, read_index, bounds and chain_index 8 bytes. */
int kiss_hip_fmi_rescue_dev(kiss_hip_ctx *ctx, const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index,
                            uint64_t Q, const kiss_hip_aln *alns, uint64_t aln_count, const uint64_t *read_index, uint64_t n,
                            const uint64_t *bounds, uint64_t R, const kiss_hip_rescue_params *params, kiss_hip_chain *chains,
                            uint64_t *chain_index, uint32_t *origin, uint64_t chain_capacity, kiss_hip_rescue_report *report,
                            void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host); hits holds hit_index[Q]
 * records */
int kiss_hip_fmi_rescue_host(const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q,
                             const kiss_hip_aln *alns, uint64_t aln_count, const uint64_t *read_index, uint64_t n,
                             const uint64_t *bounds, uint64_t R, const kiss_hip_rescue_params *params, kiss_hip_chain *chains,
                             uint64_t *chain_index, uint32_t *origin, uint64_t chain_capacity, kiss_hip_rescue_report *report,
                             int device);

/* ---- FM-index: two alignment sets of one batch made one (no reference counterpart) --------------------------------------
 * Set A (alns_a, chain_index_a, optionally cigar_a with cigar_index_a) and set B (the same) are over the same V virtual reads,
 * each as kiss_hip_fmi_align_dev wrote it: C_A = chain_index_a[V] - chain_index_a[0], alns_a[i] (0 <= i < C_A) belongs to the
 * virtual read that contains chain_index_a[0] + i (either chain_index[0] may be non-zero), its ops are cigar_a[cigar_index_a[i]
 * .. cigar_index_a[i + 1]).  Output: the merged alns with chain_index (V + 1 u64, from 0), in which every virtual read has all
 * of A's alignments in their order and then all of B's; source, optional: one u32 per merged alignment, i for alns_a[i] and
 * C_A + j for alns_b[j]; cigar with cigar_index (C_A + C_B + 1 u64, from 0) when the ops are asked for.  The ops of both sets
 * and room for the merged ones are given together or not at all (anything else is KISS_HIP_E_INVALID).
 * aln_capacity < C_A + C_B or cigar_capacity < the total of ops: KISS_HIP_E_INVALID with the totals in the report, nothing
 * written; call again with room.  Other KISS_HIP_E_INVALID: a required pointer NULL, a chain index or cigar index that
 * decreases.  KISS_HIP_E_UNSUPPORTED: C_A + C_B of 2^32 or more, V of 2^31 or more, more alignments than the ctx's scratch
 * scans.  Records are read and written field by field: 4-byte alignment suffices.
 * Device times: report->ms_* (report may be NULL); the kernels also count under KISS_HIP_K_FM_QUERY. */
typedef struct kiss_hip_merge_report {
    uint64_t V, alignments_a, alignments_b, alignments, cigar_ops;
    float ms_total, ms_place, ms_copy; /* place: checks, sources, the scan of the op counts; copy: records, indices, ops */
    uint32_t reserved_;
} kiss_hip_merge_report;
/* every pointer except report is a device pointer.  Alignment: the alignment records (above), the cigar arrays and source 4
 * bytes; the chain and cigar indexes 8 bytes. */
int kiss_hip_fmi_aln_merge_dev(kiss_hip_ctx *ctx, const kiss_hip_aln *alns_a, const uint64_t *chain_index_a, const uint32_t *cigar_a,
                               const uint64_t *cigar_index_a, const kiss_hip_aln *alns_b, const uint64_t *chain_index_b,
                               const uint32_t *cigar_b, const uint64_t *cigar_index_b, uint64_t V, kiss_hip_aln *alns,
                               uint64_t aln_capacity, uint64_t *chain_index, uint32_t *source, uint32_t *cigar,
                               uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_merge_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host) */
int kiss_hip_fmi_aln_merge_host(const kiss_hip_aln *alns_a, const uint64_t *chain_index_a, const uint32_t *cigar_a,
                                const uint64_t *cigar_index_a, const kiss_hip_aln *alns_b, const uint64_t *chain_index_b,
                                const uint32_t *cigar_b, const uint64_t *cigar_index_b, uint64_t V, kiss_hip_aln *alns,
                                uint64_t aln_capacity, uint64_t *chain_index, uint32_t *source, uint32_t *cigar,
                                uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_merge_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif /* KISS_HIP_H */
