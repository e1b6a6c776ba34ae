// fm_pileup.hip -- FM-index: per-position pileup counts of the mappings, accumulated on the GPU (kiss_hip_fmi_pileup_*).
//
// The reference has no such function; the definition is in include/kiss_hip_pileup.h and restated in
// tests/fm_pileup_model.py.  The call reads what the align (or merge), select and pair calls wrote, and the text and the reads
// they were made from, and adds into 8 planes of W u32 that the caller keeps from call to call.
//
//   head  : one kernel checks chain_index and read_index and fetches the ends of chain_index (C); the host looks once.  A second
//           one, once C is known, checks cigar_index; its verdict is read ON THE DEVICE by the two kernels behind it, which do
//           nothing when it is set: counts stays untouched on an E_INVALID return without another round trip.
//   zero  : accumulate == 0: a grid-stride store kernel over the 8 W words.
//   walk  : ONE WAVE PER ITEM (a wave takes items g, g + waves, ...).  The wave opens the item -- in pair mode from the pair
//           record, else from the hit or the alignment number --, applies the filter (wave-uniform), holds the record against
//           the read and the text and the op list against the record exactly as fm_md.hip's md_open<true> does (a second copy of
//           that code: fm_md.hip is left as it is), then goes through the ops in order with the lanes over the
//           columns of the current op, 64 per step.  Every add is a no-return atomic add of 1 on a u32 at device scope.  The
//           planes are plane-major so that the add every column makes (COV) is 64 consecutive words per wave instruction; ALT adds
//           come only from the lanes whose base differs; DEL is contiguous; INS is one lane per op.
// The report's counts are wave-uniform registers (ballots and interval arithmetic, no cross-lane sums), one atomic per wave and
// field at the end.  No LDS, no scratch.  Every address is a kernel-argument pointer plus a 64-bit offset; the only value that
// crosses lanes is the 32-bit op word.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_pileup.h"

#include <vector>

namespace {

constexpr int PILE_THREADS = 256;
constexpr int PILE_WAVES = PILE_THREADS / 64;
constexpr unsigned PILE_MAX_BLOCKS = 8192;
constexpr uint32_t PILE_HIT_FLAGS = KISS_HIP_HIT_REVERSE | KISS_HIP_HIT_SECONDARY | KISS_HIP_HIT_SUPPLEMENTARY;

// control block of a call (u64 words)
enum {
    PILE_BADIN = 0, PILE_C0, PILE_C1, PILE_BAD, PILE_FILTERED, PILE_UNMAPPED, PILE_COUNTED, PILE_COLUMNS, PILE_ALT, PILE_DEL, PILE_INS,
    PILE_CLIPPED, PILE_CTL_WORDS
};

// Every load of a field or an index entry starts at a multiple of its own size, as in fm_md.hip: relaxed
// loads of wavefront scope, which the compiler does not merge into wider ones.
__device__ __forceinline__ uint32_t pile_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t pile_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t pile_wave_sum64(uint64_t v)
{
    // (two unsigned halves per step, joined without a sign)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t l = __shfl_xor((uint32_t)v, d, 64), h = __shfl_xor((uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)h << 32) | (uint64_t)l;
    }
    return v;
}

// a chain_index that decreases, a read_index that does not ascend (a zero-length read too); the ends of chain_index
__global__ __launch_bounds__(PILE_THREADS) void k_pile_head(const uint64_t *__restrict__ chain_index, uint64_t V, const uint64_t *__restrict__ read_index,
                                                           uint64_t Q, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * PILE_THREADS + threadIdx.x;
    if (g == 0) {
        ctl[PILE_C0] = pile_ld64(chain_index);
        ctl[PILE_C1] = pile_ld64(chain_index + V);
    }
    bool bad = g < V && pile_ld64(chain_index + g + 1) < pile_ld64(chain_index + g);
    if (g < Q && pile_ld64(read_index + g + 1) <= pile_ld64(read_index + g)) bad = true;
    if (__ballot(bad) && lane_id() == 0) ctl[PILE_BADIN] = 1;
}
// a cigar_index that decreases
__global__ __launch_bounds__(PILE_THREADS) void k_pile_check_ops(const uint64_t *__restrict__ cigar_index, uint64_t C, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * PILE_THREADS + threadIdx.x;
    const bool bad = g < C && pile_ld64(cigar_index + g + 1) < pile_ld64(cigar_index + g);
    if (__ballot(bad) && lane_id() == 0) ctl[PILE_BADIN] = 1;
}
// counts[0, words) = 0, unless the checks in front refused the input
__global__ __launch_bounds__(PILE_THREADS) void k_pile_zero(uint32_t *__restrict__ counts, uint64_t words, const unsigned long long *__restrict__ ctl)
{
    if (ctl[PILE_BADIN]) return;
    for (uint64_t g = (uint64_t)blockIdx.x * PILE_THREADS + threadIdx.x; g < words; g += (uint64_t)gridDim.x * PILE_THREADS) counts[g] = 0u;
}

struct PileIn {
    const uint8_t *text;
    uint64_t n;
    const uint8_t *reads;
    const uint64_t *read_index;
    int both;
    const kiss_hip_aln *alns;
    const uint64_t *chain_index;
    uint64_t V, c0, C;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const kiss_hip_hit *hits;
    uint64_t H;
    const kiss_hip_pair *pairs;
    uint64_t items;
    uint32_t min_mapq, skip_flags, proper_only;
    uint64_t lo, hi, W;
    uint32_t *counts;
};

// what a wave knows of its item once it is opened; every field is the same in all lanes
struct PileItem {
    uint64_t rb, L; // where the read starts in reads, its length
    uint64_t o0, nops;
    uint32_t rbeg, tbeg;
    bool rev;
};
enum { PILE_WALK = 0, PILE_EMPTY = 1, PILE_ISBAD = 2, PILE_ISFILTERED = 3, PILE_ISUNMAPPED = 4 };

// which alignment item g is, after the filter
__device__ __forceinline__ int pile_select(const PileIn &in, uint64_t g, uint64_t &a)
{
    if (!in.hits) {
        a = g;
        return PILE_WALK;
    }
    uint64_t h = g;
    uint32_t mapq = 0, keep = ~0u;
    if (in.pairs) {
        const uint32_t *rec = &in.pairs[g >> 1].hit1;
        const uint32_t m = (uint32_t)(g & 1ull);
        const uint32_t pflags = pile_ld32(rec + 2);
        if (pflags & KISS_HIP_PAIR_BAD_INPUT) return PILE_ISBAD;
        h = pile_ld32(rec + m);
        if (h == (uint64_t)KISS_HIP_PAIR_NONE) return PILE_ISUNMAPPED;
        if (h >= in.H) return PILE_ISBAD;
        if (in.proper_only && !(pflags & KISS_HIP_PAIR_PROPER)) return PILE_ISFILTERED;
        mapq = pile_ld32(rec + 7 + m);
        keep = ~KISS_HIP_HIT_SECONDARY;
    } else {
        mapq = pile_ld32(&in.hits[h].mapq);
    }
    const uint32_t flags = pile_ld32(&in.hits[h].flags) & keep;
    if (mapq < in.min_mapq || (flags & in.skip_flags)) return PILE_ISFILTERED;
    a = pile_ld32(&in.hits[h].aln);
    return PILE_WALK;
}

// Alignment a held against the definition: the checks of md_open<true> (fm_md.hip), in its order.
__device__ __forceinline__ int pile_open(const PileIn &in, uint64_t a, PileItem &it)
{
    const uint32_t lane = lane_id();
    if (a >= in.C) return PILE_ISBAD;
    const uint64_t x = pile_ld64(in.cigar_index + a), y = pile_ld64(in.cigar_index + a + 1);
    it.o0 = x;
    it.nops = y > x ? y - x : 0; // (an index that decreases fails the call: k_pile_check_ops)
    if (it.nops == 0) return PILE_EMPTY;
    // the largest v with chain_index[v] <= c0 + a (chain_index[V] > c0 + a: a < C)
    const uint64_t at = in.c0 + a;
    uint64_t lo = 0, hi = in.V;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pile_ld64(in.chain_index + mid) <= at) lo = mid;
        else hi = mid;
    }
    const uint64_t q = in.both ? lo >> 1 : lo;
    it.rev = in.both && (lo & 1ull);
    it.rb = pile_ld64(in.read_index + q);
    it.L = pile_ld64(in.read_index + q + 1) - it.rb;
    const uint32_t *rec = &in.alns[a].score;
    const uint32_t rbeg = pile_ld32(rec + 2), rend = pile_ld32(rec + 3), tbeg = pile_ld32(rec + 4), tend = pile_ld32(rec + 5);
    it.rbeg = rbeg;
    it.tbeg = tbeg;
    if ((uint64_t)rend > it.L || (uint64_t)tend > in.n || rbeg > rend || tbeg > tend) return PILE_ISBAD;
    uint64_t sum_r = 0, sum_t = 0;
    bool bad_op = false;
    for (uint64_t kb = 0; kb < it.nops; kb += 64) {
        if (kb + lane < it.nops) {
            const uint32_t w = pile_ld32(in.cigar + it.o0 + kb + lane);
            const uint32_t op = w & 15u;
            const uint64_t len = w >> 4;
            bad_op = bad_op || op > 2u || len == 0;
            if (op == 0 || op == 1) sum_r += len;
            if (op == 0 || op == 2) sum_t += len;
        }
    }
    if (__ballot(bad_op)) return PILE_ISBAD;
    if (pile_wave_sum64(sum_r) != (uint64_t)(rend - rbeg) || pile_wave_sum64(sum_t) != (uint64_t)(tend - tbeg)) return PILE_ISBAD;
    return PILE_WALK;
}

// how many of the positions [j, j + len) lie inside [lo, hi)
__device__ __forceinline__ uint64_t pile_inside(uint64_t j, uint64_t len, uint64_t lo, uint64_t hi)
{
    const uint64_t b = j > lo ? j : lo, e = j + len < hi ? j + len : hi;
    return e > b ? e - b : 0;
}
// (pos inside the window: the caller has looked)
__device__ __forceinline__ void pile_add(const PileIn &in, uint32_t plane, uint64_t pos)
{
    (void)__hip_atomic_fetch_add(in.counts + (uint64_t)plane * in.W + (pos - in.lo), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct PileSums {
    unsigned long long columns = 0, alt = 0, del = 0, ins = 0, clipped = 0;
};

// The walk of an item that pile_open let through: i stays inside [rbeg, rend) of a read of L bases, j inside [tbeg, tend) of the
// text (j - 1 of an I op: tbeg <= j <= tend <= n, and j == 0 adds nothing), and every add is held against the window.
__device__ __forceinline__ void pile_walk(const PileIn &in, const PileItem &it, PileSums &s)
{
    const uint32_t lane = lane_id();
    const uint8_t *const rd = in.reads + it.rb;
    uint64_t i = it.rbeg, j = it.tbeg;
    for (uint64_t kb = 0; kb < it.nops; kb += 64) {
        const uint32_t mine = kb + lane < it.nops ? pile_ld32(in.cigar + it.o0 + kb + lane) : 0u;
        const uint32_t here = it.nops - kb < 64 ? (uint32_t)(it.nops - kb) : 64u;
        for (uint32_t kk = 0; kk < here; kk++) {
            const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl(mine, (int)kk, 64));
            const uint32_t op = w & 15u, len = w >> 4;
            if (op == 1u) { // once per op, in front of the inserted bases
                s.ins++;
                if (j > 0) {
                    const uint64_t pos = j - 1;
                    if (pos >= in.lo && pos < in.hi) {
                        if (lane == 0) pile_add(in, KISS_HIP_PILEUP_INS, pos);
                    } else {
                        s.clipped++;
                    }
                }
                i += len;
                continue;
            }
            const uint64_t inside = pile_inside(j, len, in.lo, in.hi);
            s.clipped += len - inside;
            if (op == 2u) {
                s.del += len;
                if (inside)
                    for (uint32_t c = lane; c < len; c += 64) {
                        const uint64_t pos = j + c;
                        if (pos >= in.lo && pos < in.hi) pile_add(in, KISS_HIP_PILEUP_DEL, pos);
                    }
                j += len;
                continue;
            }
            s.columns += len;
            for (uint32_t c0 = 0; c0 < len; c0 += 64) {
                const uint32_t cnt = len - c0 < 64 ? len - c0 : 64u;
                const uint64_t pos = j + c0 + lane;
                const bool inw = lane < cnt && pos >= in.lo && pos < in.hi;
                uint32_t alt = 0; // the ALT plane of this column, 0: none
                if (lane < cnt) {
                    const uint64_t ri = i + c0 + lane;
                    uint32_t r = it.rev ? rd[it.L - 1 - ri] : rd[ri];
                    if (it.rev && r <= 3u) r = 3u - r;
                    const uint32_t tj = in.text[pos];
                    alt = r > 3u ? KISS_HIP_PILEUP_ALT_N : (r != tj ? KISS_HIP_PILEUP_ALT_A + r : 0u);
                }
                if (inw) {
                    pile_add(in, KISS_HIP_PILEUP_COV, pos);
                    if (alt) pile_add(in, alt, pos);
                }
                s.alt += (unsigned long long)__popcll(__ballot(alt != 0u));
                s.clipped += (unsigned long long)__popcll(__ballot(alt != 0u && !inw));
            }
            i += len;
            j += len;
        }
    }
}

__global__ __launch_bounds__(PILE_THREADS) void k_pile_walk(PileIn in, unsigned long long *__restrict__ ctl)
{
    if (ctl[PILE_BADIN]) return; // (k_pile_check_ops, in front on the stream)
    const uint64_t waves = (uint64_t)gridDim.x * PILE_WAVES;
    unsigned long long a_bad = 0, a_filtered = 0, a_unmapped = 0, a_counted = 0;
    PileSums s;
    for (uint64_t g = (uint64_t)blockIdx.x * PILE_WAVES + (threadIdx.x >> 6); g < in.items; g += waves) {
        uint64_t a = 0;
        int what = pile_select(in, g, a);
        PileItem it;
        if (what == PILE_WALK) what = pile_open(in, a, it);
        if (what == PILE_WALK) pile_walk(in, it, s);
        a_counted += what == PILE_WALK || what == PILE_EMPTY;
        a_bad += what == PILE_ISBAD;
        a_filtered += what == PILE_ISFILTERED;
        a_unmapped += what == PILE_ISUNMAPPED;
    }
    if (lane_id() == 0) {
        if (a_bad) atomicAdd(&ctl[PILE_BAD], a_bad);
        if (a_filtered) atomicAdd(&ctl[PILE_FILTERED], a_filtered);
        if (a_unmapped) atomicAdd(&ctl[PILE_UNMAPPED], a_unmapped);
        if (a_counted) atomicAdd(&ctl[PILE_COUNTED], a_counted);
        if (s.columns) atomicAdd(&ctl[PILE_COLUMNS], s.columns);
        if (s.alt) atomicAdd(&ctl[PILE_ALT], s.alt);
        if (s.del) atomicAdd(&ctl[PILE_DEL], s.del);
        if (s.ins) atomicAdd(&ctl[PILE_INS], s.ins);
        if (s.clipped) atomicAdd(&ctl[PILE_CLIPPED], s.clipped);
    }
}

struct PileArgs {
    const uint8_t *text;
    uint64_t n;
    const uint8_t *reads;
    const uint64_t *read_index;
    uint64_t Q;
    int both;
    const kiss_hip_aln *alns;
    const uint64_t *chain_index;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const kiss_hip_hit *hits;
    uint64_t H;
    const kiss_hip_pair *pairs;
    uint64_t P;
    const kiss_hip_pileup_params *params;
    uint64_t lo, hi;
    uint32_t *counts;
};

int pile_args_check(const PileArgs &a)
{
    if (!a.text || !a.reads || !a.read_index || !a.alns || !a.chain_index || !a.cigar || !a.cigar_index || !a.params) return KISS_HIP_E_INVALID;
    if (a.pairs && !a.hits) return KISS_HIP_E_INVALID;
    if (a.lo > a.hi || a.hi > a.n || (a.hi > a.lo && !a.counts)) return KISS_HIP_E_INVALID;
    if (a.params->reserved_ || a.params->min_mapq > 255u || (a.params->skip_flags & ~PILE_HIT_FLAGS)) return KISS_HIP_E_INVALID;
    if (a.n > KISS_HIP_MAX_N || a.Q >= (1ull << 31) || (a.both && 2 * a.Q >= (1ull << 31))) return KISS_HIP_E_UNSUPPORTED;
    if (a.hits && a.H > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (a.pairs && a.P > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int pile_steps(kiss_hip_ctx *ctx, const PileArgs &a, int accumulate, kiss_hip_pileup_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t V = a.both ? 2 * a.Q : a.Q;
    FmCtl<PILE_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_PILEUP_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    const dim3 threads(PILE_THREADS);
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_pile_head, dim3(fm_grid((V > a.Q ? V : a.Q) + 1, PILE_THREADS)), threads, 0, ctx->stream, a.chain_index, V, a.read_index,
                       a.Q, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[PILE_BADIN]) return KISS_HIP_E_INVALID; // an index out of order, a read of length 0
    const uint64_t C = h[PILE_C1] - h[PILE_C0];
    const uint64_t items = a.pairs ? 2 * a.P : (a.hits ? a.H : C);
    rep.items = items;
    if (items > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    ev.mark(1);
    const uint64_t W = a.hi - a.lo;
    const PileIn in{a.text, a.n, a.reads, a.read_index, a.both, a.alns, a.chain_index, V, h[PILE_C0], C, a.cigar, a.cigar_index, a.hits, a.H, a.pairs,
                    items, a.params->min_mapq, a.params->skip_flags, a.params->proper_only, a.lo, a.hi, W, a.counts};
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, items);
        if (C) hipLaunchKernelGGL(k_pile_check_ops, dim3(fm_grid(C, PILE_THREADS)), threads, 0, ctx->stream, a.cigar_index, C, d_ctl);
        if (!accumulate && W) {
            const uint64_t blocks = div_up(8 * W, (uint64_t)PILE_THREADS * 4);
            hipLaunchKernelGGL(k_pile_zero, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), threads, 0, ctx->stream, a.counts, 8 * W,
                               (const unsigned long long *)d_ctl);
        }
        if (items) {
            const uint64_t blocks = div_up(items, PILE_WAVES);
            hipLaunchKernelGGL(k_pile_walk, dim3((unsigned)(blocks < PILE_MAX_BLOCKS ? blocks : PILE_MAX_BLOCKS)), threads, 0, ctx->stream, in, d_ctl);
        }
        KCHECK(hipGetLastError());
    }
    KTRY(ctl.fetch());
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_check = ev.ms(0, 1);
    rep.ms_walk = ev.ms(1, 2);
    if (h[PILE_BADIN]) return KISS_HIP_E_INVALID; // a cigar index decreases: nothing was zeroed, nothing added
    rep.bad = h[PILE_BAD];
    rep.filtered = h[PILE_FILTERED];
    rep.unmapped = h[PILE_UNMAPPED];
    rep.counted = h[PILE_COUNTED];
    rep.columns = h[PILE_COLUMNS];
    rep.alt_columns = h[PILE_ALT];
    rep.deleted_bases = h[PILE_DEL];
    rep.insertions = h[PILE_INS];
    rep.clipped = h[PILE_CLIPPED];
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_pileup_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            int both_strands, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar,
                            const uint64_t *cigar_index, const kiss_hip_hit *hits, uint64_t H, const kiss_hip_pair *pairs, uint64_t P,
                            const kiss_hip_pileup_params *params, uint64_t lo, uint64_t hi, uint32_t *counts, int accumulate,
                            kiss_hip_pileup_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_pileup_report rep{};
    if (report) *report = rep;
    const PileArgs a{text, n, reads, read_index, Q, both_strands ? 1 : 0, alns, chain_index, cigar, cigar_index, hits, hits ? H : 0, pairs,
                     pairs ? P : 0, params, lo, hi, counts};
    KTRY(pile_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    int rc = pile_steps(ctx, a, accumulate, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_fmi_pileup_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q, int both_strands,
                             const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar, const uint64_t *cigar_index,
                             const kiss_hip_hit *hits, uint64_t H, const kiss_hip_pair *pairs, uint64_t P,
                             const kiss_hip_pileup_params *params, uint64_t lo, uint64_t hi, uint32_t *counts, int counts_on_device,
                             int accumulate, kiss_hip_pileup_report *report, int device)
{
    if (report) *report = kiss_hip_pileup_report{};
    const PileArgs a{text, n, reads, read_index, Q, both_strands ? 1 : 0, alns, chain_index, cigar, cigar_index, hits, hits ? H : 0, pairs,
                     pairs ? P : 0, params, lo, hi, counts};
    KTRY(pile_args_check(a));
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (!fm_index_ascending(read_index, Q, true) || !fm_index_ascending(chain_index, V, false)) return KISS_HIP_E_INVALID;
    const uint64_t C = chain_index[V] - chain_index[0];
    if (!fm_index_ascending(cigar_index, C, false)) return KISS_HIP_E_INVALID;
    const uint64_t items = a.pairs ? 2 * a.P : (a.hits ? a.H : C);
    if (report) report->items = items;
    if (items > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    // (the ops are uploaded from the first one the alignments use, their index from 0)
    std::vector<uint64_t> oi(C + 1);
    for (uint64_t i = 0; i <= C; i++) oi[i] = cigar_index[i] - cigar_index[0];
    const uint64_t bytes = 32 * (hi - lo);
    return kiss_one_shot_cached(device, fm_host_max_n(0, 0), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *dtext = st.up(text, n), *dreads = st.up(reads, read_index[Q]);
        const uint64_t *dridx = st.up(read_index, (Q + 1) * 8), *dcidx = st.up(chain_index, (V + 1) * 8);
        const kiss_hip_aln *dalns = st.up(alns, C * sizeof(kiss_hip_aln));
        const uint32_t *dcig = st.up(cigar + cigar_index[0], oi[C] * 4);
        const uint64_t *doidx = st.up(oi.data(), (C + 1) * 8);
        const kiss_hip_hit *dhits = st.up(hits, a.H * sizeof(kiss_hip_hit));
        const kiss_hip_pair *dpairs = st.up(pairs, a.P * sizeof(kiss_hip_pair));
        uint32_t *dcounts = counts;
        if (!counts_on_device && bytes) dcounts = accumulate ? const_cast<uint32_t *>(st.up(counts, bytes)) : st.room<uint32_t>(true, bytes);
        if (st.rc) return st.rc;
        const int rc = kiss_hip_fmi_pileup_dev(ctx, dtext, n, dreads, dridx, Q, both_strands, dalns, dcidx, dcig, doidx, dhits, a.H, dpairs, a.P,
                                               params, lo, hi, dcounts, accumulate, report, nullptr);
        if (rc) return rc;
        if (!counts_on_device && bytes) st.down(counts, dcounts, bytes);
        return st.rc;
    });
}

} // extern "C"
