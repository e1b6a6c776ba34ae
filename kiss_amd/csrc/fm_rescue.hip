// fm_rescue.hip -- FM-index: the missing mate looked for near its partner (kiss_hip_fmi_rescue_*), and two alignment sets of
// one batch made one (kiss_hip_fmi_aln_merge_*).
//
// The reference has no such functions; the definitions are in include/kiss_hip.h and restated in tests/fm_rescue_model.py.
// The plan call reads what the select and pair calls wrote and writes chain records for kiss_hip_fmi_align_dev as it is; the
// merge call puts the alignments of those chains behind a read's own, so that select and pair run once more on the whole.
//
//   plan  head  : one kernel checks hit_index, read_index and bounds and fetches hit_index[Q].
//         count : ONE WAVE PER PAIR (a wave takes pairs p, p + waves, ...).  For either mate the hits of the OTHER mate go
//                 through the lanes 64 at a time; the first max_anchors qualifying ones are found by ballot and prefix
//                 popcount, every such lane works out its window and the number of its pieces.  The four virtual reads of
//                 the pair get their chain counts, the report's counts reach the control block once per wave.
//         scan  : the library's u64 scan over the 2 Q + 1 counts; the host looks at the total once (capacity).
//         emit  : the same walk again, now writing: a lane's pieces go behind those of the lanes before it (a prefix sum
//                 over the wave), so the CSR is the model's whatever the schedule.
//   merge head  : the chain indices checked, their ends fetched.
//         place : one lane per merged alignment finds its virtual read by search, then its source record and op count.
//         emit  : after the scan of the op counts and one look at the totals: records, source, both indices.
//         ops   : one lane per op finds its alignment by search in the scanned counts; writes are coalesced.
#include "fm_internal.hpp"

#include <vector>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr unsigned RS_MAX_BLOCKS = 4096;

// control block of a plan call (u64 words)
enum { RS_BAD = 0, RS_TOTAL = 1, RS_PLANNED = 2, RS_ANCHORS = 3, RS_SPLIT = 4, RS_EMPTY = 5, RS_BADIN = 6, RS_MAXCH = 7, RS_CTL_WORDS = 8 };
// ... of a merge call (the two calls share the slot: one call at a time per ctx)
enum { MG_BAD = 0, MG_A0 = 1, MG_A1 = 2, MG_B0 = 3, MG_B1 = 4, MG_CTL_WORDS = 8 };
static_assert(MG_CTL_WORDS == RS_CTL_WORDS, "one slot for both control blocks");

struct RescueP {
    uint32_t ins_min, ins_max, max_anchors, min_score, max_width;
};

// Every load of this file starts at a multiple of its own size, as in fm_pair.hip: fields and index entries
// go through relaxed loads and stores of wavefront scope, which the compiler does not merge into wider ones.
__device__ __forceinline__ uint32_t rs_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t rs_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void rs_st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void rs_st64(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// the sum of v over the lanes below this one; total: over the wave
__device__ __forceinline__ uint64_t rs_wave_excl64(uint64_t v, uint64_t &total)
{
    const uint32_t lane = lane_id();
    uint64_t s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(s, o, 64);
        if (lane >= (uint32_t)o) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

// the last v with index[v] <= x (index[0] <= x)
__device__ __forceinline__ uint64_t rs_last_le(const uint64_t *__restrict__ index, uint64_t count, uint64_t x)
{
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rs_ld64(index + mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- plan ---------------------------------------------------------------------------------------------------------------

// a hit_index that decreases, a read_index that does not ascend, bounds that do not start at 0, do not ascend or end past n;
// hit_index[Q]
__global__ __launch_bounds__(RS_THREADS) void k_rescue_head(const uint64_t *__restrict__ hit_index, const uint64_t *__restrict__ read_index,
                                                           uint64_t Q, const uint64_t *__restrict__ bounds, uint64_t R, uint64_t n,
                                                           unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (g == 0) ctl[RS_TOTAL] = rs_ld64(hit_index + Q);
    bool bad = g < Q && rs_ld64(hit_index + g + 1) < rs_ld64(hit_index + g);
    if (g < Q && rs_ld64(read_index + g + 1) <= rs_ld64(read_index + g)) bad = true; // (a zero-length read too)
    if (bounds) {
        if (g == 0 && (rs_ld64(bounds) != 0 || rs_ld64(bounds + R) > n)) bad = true;
        if (g < R && rs_ld64(bounds + g + 1) <= rs_ld64(bounds + g)) bad = true;
    }
    if (__ballot(bad) && lane_id() == 0) ctl[RS_BAD] = 1;
}

// The walk of both passes.  EMIT false: counts[4 p .. 4 p + 3] = the chains of the four virtual reads of pair p, and the
// report's counts.  EMIT true: offs (the scanned counts) says where they go.  hit_index never decreases and no read is empty
// (k_rescue_head).
template <bool EMIT>
__device__ __forceinline__ void rs_walk(const kiss_hip_pair *__restrict__ pairs, const kiss_hip_hit *__restrict__ hits,
                                        const uint64_t *__restrict__ hit_index, uint64_t NP, const kiss_hip_aln *__restrict__ alns,
                                        uint64_t aln_count, const uint64_t *__restrict__ read_index, uint64_t n,
                                        const uint64_t *__restrict__ bounds, uint64_t R, const RescueP &P, uint64_t *__restrict__ counts,
                                        const uint64_t *__restrict__ offs, kiss_hip_chain *__restrict__ chains,
                                        uint32_t *__restrict__ origin, unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = lane_id();
    const uint64_t waves = (uint64_t)gridDim.x * RS_WAVES;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long a_planned = 0, a_anchors = 0, a_split = 0, a_empty = 0, a_bad = 0, a_maxch = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * RS_WAVES + (threadIdx.x >> 6); p < NP; p += waves) {
        const uint32_t pf = rs_ld32(&pairs[p].flags);
        const bool rescued = !(pf & (KISS_HIP_PAIR_PROPER | KISS_HIP_PAIR_BAD_INPUT));
        uint64_t of_pair = 0;
        for (uint32_t m = 0; m < 2; m++) {
            const uint64_t q = 2 * p + m, o = 2 * p + 1 - m;
            uint64_t base_r = 0, base_f = 0; // the chains of virtual reads 2 q (reverse anchors) and 2 q + 1 (forward anchors) so far
            if (rescued) {
                uint64_t Lu = rs_ld64(read_index + q + 1) - rs_ld64(read_index + q);
                // (a read longer than the text fits no record: any such length gives empty windows, and this one cannot wrap)
                const long long L = (long long)(Lu < (1ull << 33) ? Lu : (1ull << 33));
                const uint64_t so = rs_ld64(hit_index + o), no = rs_ld64(hit_index + o + 1) - so;
                const uint64_t off_r = EMIT ? rs_ld64(offs + 2 * q) : 0, off_f = EMIT ? rs_ld64(offs + 2 * q + 1) : 0;
                uint64_t taken = 0;
                for (uint64_t b = 0; b < no && taken < (uint64_t)P.max_anchors; b += 64) {
                    bool qual = false, badaln = false;
                    uint32_t tb = 0, te = 0, ref = 0, rev = 0, score = 0;
                    if (b + lane < no) {
                        const kiss_hip_hit *h = hits + so + b + lane;
                        const uint32_t aln = rs_ld32(&h->aln), head = rs_ld32(&h->head);
                        score = rs_ld32(&h->score);
                        rev = rs_ld32(&h->flags) & KISS_HIP_HIT_REVERSE;
                        ref = rs_ld32(&h->ref);
                        qual = head == 0 && score >= P.min_score;
                        badaln = aln >= aln_count;
                        if (qual && !badaln) {
                            tb = rs_ld32(&alns[aln].tbeg);
                            te = rs_ld32(&alns[aln].tend);
                            qual = tb < te;
                        }
                    }
                    const unsigned long long qm = __ballot(qual);
                    const bool sel = qual && taken + (uint64_t)__popcll(qm & below) < (uint64_t)P.max_anchors;
                    const unsigned long long sm = __ballot(sel);
                    taken += (uint64_t)__popcll(sm);
                    const bool bad = sel && (badaln || (bounds && (uint64_t)ref >= R));
                    bool empty = false;
                    long long dmin = 0, W = 0;
                    uint64_t k = 0;
                    if (sel && !bad) {
                        const long long lo = bounds ? (long long)rs_ld64(bounds + ref) : 0ll;
                        const long long hi = bounds ? (long long)rs_ld64(bounds + ref + 1) : (long long)n;
                        long long dmax;
                        if (!rev) {
                            long long t = (long long)tb + (long long)P.ins_min;
                            t = t > (long long)te ? t : (long long)te;
                            t = t > (long long)tb + L ? t : (long long)tb + L;
                            dmin = t - L;
                            dmax = (long long)tb + (long long)P.ins_max - L;
                        } else {
                            dmin = (long long)te - (long long)P.ins_max;
                            long long t = (long long)te - (long long)P.ins_min;
                            t = t < (long long)tb ? t : (long long)tb;
                            t = t < (long long)te - L ? t : (long long)te - L;
                            dmax = t;
                        }
                        dmin = dmin > lo ? dmin : lo;
                        dmax = dmax < hi - L ? dmax : hi - L;
                        empty = dmin > dmax;
                        if (!empty) {
                            W = dmax - dmin + 1; // (at most ins_max - ins_min + 1)
                            k = ((uint64_t)W + P.max_width - 1) / P.max_width;
                        }
                    }
                    uint64_t tot_r, tot_f;
                    const uint64_t ex_r = rs_wave_excl64(rev ? k : 0, tot_r), ex_f = rs_wave_excl64(rev ? 0 : k, tot_f);
                    if (EMIT) {
                        const uint64_t at = rev ? off_r + base_r + ex_r : off_f + base_f + ex_f;
                        for (uint64_t j = 0; j < k; j++) { // (in [lo, hi - L] of a record inside [0, n]: every field fits u32)
                            const long long a0 = dmin + (long long)(j * (uint64_t)W / k), b0 = dmin + (long long)((j + 1) * (uint64_t)W / k) - 1;
                            uint32_t *c = &chains[at + j].score;
                            rs_st32(c + 0, score);
                            rs_st32(c + 1, 0u);
                            rs_st32(c + 2, 0u);
                            rs_st32(c + 3, (uint32_t)L);
                            rs_st32(c + 4, (uint32_t)a0);
                            rs_st32(c + 5, (uint32_t)(b0 + L));
                            if (origin) origin[at + j] = (uint32_t)(so + b + lane); // (hit_index[Q] < 2^32 - 1)
                        }
                    } else {
                        a_anchors += (unsigned long long)__popcll(sm);
                        a_bad += (unsigned long long)__popcll(__ballot(bad));
                        a_empty += (unsigned long long)__popcll(__ballot(empty));
                        a_split += (unsigned long long)__popcll(__ballot(k > 1));
                    }
                    base_r += tot_r;
                    base_f += tot_f;
                }
            }
            if (!EMIT && lane == 0) {
                rs_st64(counts + 2 * q, base_r);
                rs_st64(counts + 2 * q + 1, base_f);
            }
            of_pair += base_r + base_f;
        }
        if (of_pair) a_planned++;
        a_maxch = a_maxch > of_pair ? a_maxch : of_pair;
    }
    if (!EMIT && lane == 0) {
        if (a_planned) atomicAdd(&ctl[RS_PLANNED], a_planned);
        if (a_anchors) atomicAdd(&ctl[RS_ANCHORS], a_anchors);
        if (a_split) atomicAdd(&ctl[RS_SPLIT], a_split);
        if (a_empty) atomicAdd(&ctl[RS_EMPTY], a_empty);
        if (a_bad) atomicAdd(&ctl[RS_BADIN], a_bad);
        if (a_maxch) atomicMax(&ctl[RS_MAXCH], a_maxch);
    }
}

__global__ __launch_bounds__(RS_THREADS) void k_rescue_count(const kiss_hip_pair *__restrict__ pairs, const kiss_hip_hit *__restrict__ hits,
                                                            const uint64_t *__restrict__ hit_index, uint64_t NP,
                                                            const kiss_hip_aln *__restrict__ alns, uint64_t aln_count,
                                                            const uint64_t *__restrict__ read_index, uint64_t n,
                                                            const uint64_t *__restrict__ bounds, uint64_t R, RescueP P,
                                                            uint64_t *__restrict__ counts, unsigned long long *__restrict__ ctl)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[4 * NP] = 0; // closes the array for the scan
    rs_walk<false>(pairs, hits, hit_index, NP, alns, aln_count, read_index, n, bounds, R, P, counts, nullptr, nullptr, nullptr, ctl);
}

__global__ __launch_bounds__(RS_THREADS) void k_rescue_emit(const kiss_hip_pair *__restrict__ pairs, const kiss_hip_hit *__restrict__ hits,
                                                           const uint64_t *__restrict__ hit_index, uint64_t NP,
                                                           const kiss_hip_aln *__restrict__ alns, uint64_t aln_count,
                                                           const uint64_t *__restrict__ read_index, uint64_t n,
                                                           const uint64_t *__restrict__ bounds, uint64_t R, RescueP P,
                                                           const uint64_t *__restrict__ offs, kiss_hip_chain *__restrict__ chains,
                                                           uint64_t *__restrict__ chain_index, uint32_t *__restrict__ origin)
{
    for (uint64_t g = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x; g <= 4 * NP; g += (uint64_t)gridDim.x * RS_THREADS)
        chain_index[g] = rs_ld64(offs + g);
    rs_walk<true>(pairs, hits, hit_index, NP, alns, aln_count, read_index, n, bounds, R, P, nullptr, offs, chains, origin, nullptr);
}

int rescue_steps(kiss_hip_ctx *ctx, const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q,
                 const kiss_hip_aln *alns, uint64_t aln_count, const uint64_t *read_index, uint64_t n, const uint64_t *bounds, uint64_t R,
                 const RescueP &P, kiss_hip_chain *chains, uint64_t *chain_index, uint32_t *origin, uint64_t chain_capacity,
                 kiss_hip_rescue_report *rep, FmEvents &ev)
{
    const uint64_t NP = Q / 2, V = 2 * Q;
    if ((V + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    DevBuf slab;
    FmCtl<RS_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_RESCUE_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    {
        const uint64_t items = bounds && R + 1 > Q + 1 ? R + 1 : Q + 1;
        hipLaunchKernelGGL(k_rescue_head, dim3(fm_grid(items, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, hit_index, read_index, Q, bounds, R, n,
                           d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(ctl.fetch_sync());
    if (h[RS_BAD]) return KISS_HIP_E_INVALID;                         // an index out of order, a read of length 0, bad bounds
    if (h[RS_TOTAL] >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED; // origin is u32, as hit1 / hit2 of a pair
    KTRY(slab.take(ctx, FM_SLOT_RESCUE_SLAB, (V + 1) * 8));
    uint64_t *const counts = (uint64_t *)slab.p;
    const uint64_t blocks = div_up(NP, RS_WAVES);
    const dim3 grid((unsigned)(blocks < RS_MAX_BLOCKS ? blocks : RS_MAX_BLOCKS));
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, NP);
        hipLaunchKernelGGL(k_rescue_count, grid, dim3(RS_THREADS), 0, ctx->stream, pairs, hits, hit_index, NP, alns, aln_count, read_index, n,
                           bounds, R, P, counts, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, counts, counts, V + 1));
    uint64_t total = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total, counts + V, 8, hipMemcpyDeviceToHost, ctx->stream));
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) {
        rep->pairs_planned = h[RS_PLANNED];
        rep->anchors = h[RS_ANCHORS];
        rep->chains = total;
        rep->split = h[RS_SPLIT];
        rep->empty = h[RS_EMPTY];
        rep->bad_input = h[RS_BADIN];
        rep->max_chains = h[RS_MAXCH];
        rep->ms_check = ev.ms(0, 1);
        rep->ms_count = ev.ms(1, 2);
    }
    // (the totals are in the report: the caller's second call)
    if (chain_capacity < total) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, NP);
        hipLaunchKernelGGL(k_rescue_emit, grid, dim3(RS_THREADS), 0, ctx->stream, pairs, hits, hit_index, NP, alns, aln_count, read_index, n,
                           bounds, R, P, (const uint64_t *)counts, chains, chain_index, origin);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) rep->ms_emit = ev.ms(2, 3);
    return KISS_HIP_OK;
}

int rescue_args_check(const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                      const uint64_t *read_index, uint64_t n, const uint64_t *bounds, uint64_t R, const kiss_hip_rescue_params *params,
                      const kiss_hip_chain *chains, const uint64_t *chain_index)
{
    if (!pairs || !hits || !hit_index || !alns || !read_index || !params || !chains || !chain_index) return KISS_HIP_E_INVALID;
    if (Q & 1ull) return KISS_HIP_E_INVALID;
    if (bounds && (R == 0 || R > 0xFFFFFFFFull)) return KISS_HIP_E_INVALID;
    if (params->ins_min > params->ins_max || params->max_anchors < 1 || params->max_width < 1 || params->max_width > KISS_HIP_ALIGN_MAX_BAND)
        return KISS_HIP_E_INVALID;
    if (Q > 0x7FFFFFFFull || n > KISS_HIP_MAX_N) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

// ---- merge --------------------------------------------------------------------------------------------------------------

// chain indices that decrease; their ends
__global__ __launch_bounds__(RS_THREADS) void k_rescue_merge_head(const uint64_t *__restrict__ cia, const uint64_t *__restrict__ cib, uint64_t V,
                                                                 unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (g == 0) {
        ctl[MG_A0] = rs_ld64(cia);
        ctl[MG_A1] = rs_ld64(cia + V);
        ctl[MG_B0] = rs_ld64(cib);
        ctl[MG_B1] = rs_ld64(cib + V);
    }
    const bool bad = g < V && (rs_ld64(cia + g + 1) < rs_ld64(cia + g) || rs_ld64(cib + g + 1) < rs_ld64(cib + g));
    if (__ballot(bad) && lane_id() == 0) ctl[MG_BAD] = 1;
}

// one lane per merged alignment m: its virtual read (the last v whose merged segment starts at or before m), its source
// (i < CA: alns_a[i]; else alns_b[i - CA]) and its ops; lane C closes nops for the scan.  A cigar index that decreases is
// bad input.
__global__ __launch_bounds__(RS_THREADS) void k_rescue_merge_place(const uint64_t *__restrict__ cia, const uint64_t *__restrict__ cib, uint64_t V,
                                                                  uint64_t a0, uint64_t b0, uint64_t CA, uint64_t C,
                                                                  const uint64_t *__restrict__ oia, const uint64_t *__restrict__ oib,
                                                                  uint32_t *__restrict__ src, uint64_t *__restrict__ nops,
                                                                  unsigned long long *__restrict__ ctl)
{
    const uint64_t m = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    bool bad = false;
    if (m < C) {
        uint64_t lo = 0, hi = V;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((rs_ld64(cia + mid) - a0) + (rs_ld64(cib + mid) - b0) <= m) lo = mid;
            else hi = mid;
        }
        const uint64_t fa = rs_ld64(cia + lo) - a0, fb = rs_ld64(cib + lo) - b0, na = rs_ld64(cia + lo + 1) - a0 - fa;
        const uint64_t r = m - fa - fb;
        const bool from_a = r < na;
        const uint64_t i = from_a ? fa + r : fb + (r - na);
        src[m] = (uint32_t)(from_a ? i : CA + i);
        if (oia) {
            const uint64_t *oi = from_a ? oia : oib;
            const uint64_t x = rs_ld64(oi + i), y = rs_ld64(oi + i + 1);
            bad = y < x;
            nops[m] = bad ? 0ull : y - x;
        }
    } else if (m == C && oia) {
        nops[m] = 0;
    }
    if (__ballot(bad) && lane_id() == 0) ctl[MG_BAD] = 1;
}

// one lane per merged alignment: the record, its source, cigar_index; lanes 0 .. V write chain_index
__global__ __launch_bounds__(RS_THREADS) void k_rescue_merge_emit(const kiss_hip_aln *__restrict__ alns_a, const kiss_hip_aln *__restrict__ alns_b,
                                                                 const uint64_t *__restrict__ cia, const uint64_t *__restrict__ cib, uint64_t V,
                                                                 uint64_t a0, uint64_t b0, uint64_t CA, uint64_t C,
                                                                 const uint32_t *__restrict__ src, const uint64_t *__restrict__ op_off,
                                                                 kiss_hip_aln *__restrict__ alns, uint64_t *__restrict__ chain_index,
                                                                 uint32_t *__restrict__ source, uint64_t *__restrict__ cigar_index)
{
    const uint64_t m = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (m <= V) chain_index[m] = (rs_ld64(cia + m) - a0) + (rs_ld64(cib + m) - b0);
    if (m <= C && cigar_index) cigar_index[m] = rs_ld64(op_off + m);
    if (m >= C) return;
    const uint32_t s = src[m];
    const uint32_t *from = (uint64_t)s < CA ? &alns_a[s].score : &alns_b[(uint64_t)s - CA].score;
    uint32_t *to = &alns[m].score; // (twelve dword copies: no array need be 16-byte aligned)
#pragma unroll
    for (int f = 0; f < 12; f++) rs_st32(to + f, rs_ld32(from + f));
    if (source) source[m] = s;
}

// one lane per op of the merged cigar
__global__ __launch_bounds__(RS_THREADS) void k_rescue_merge_ops(const uint32_t *__restrict__ cigar_a, const uint64_t *__restrict__ oia,
                                                                const uint32_t *__restrict__ cigar_b, const uint64_t *__restrict__ oib, uint64_t CA,
                                                                uint64_t C, const uint32_t *__restrict__ src, const uint64_t *__restrict__ op_off,
                                                                uint64_t total, uint32_t *__restrict__ cigar)
{
    const uint64_t t = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (t >= total) return;
    const uint64_t m = rs_last_le(op_off, C, t); // (alignments without ops own empty segments: the last one that starts at or before t)
    const uint32_t s = src[m];
    const uint64_t k = t - rs_ld64(op_off + m);
    cigar[t] = (uint64_t)s < CA ? cigar_a[rs_ld64(oia + s) + k] : cigar_b[rs_ld64(oib + ((uint64_t)s - CA)) + k];
}

struct MergeIn {
    const kiss_hip_aln *alns;
    const uint64_t *chain_index;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
};

int merge_steps(kiss_hip_ctx *ctx, const MergeIn &A, const MergeIn &B, uint64_t V, kiss_hip_aln *alns, uint64_t aln_capacity,
                uint64_t *chain_index, uint32_t *source, uint32_t *cigar, uint64_t *cigar_index, uint64_t cigar_capacity,
                kiss_hip_merge_report *rep, FmEvents &ev)
{
    if (V > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    DevBuf slab;
    FmCtl<MG_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_RESCUE_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_rescue_merge_head, dim3(fm_grid(V + 1, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, A.chain_index, B.chain_index, V,
                       d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[MG_BAD]) return KISS_HIP_E_INVALID; // a chain index decreases
    const uint64_t a0 = h[MG_A0], CA = h[MG_A1] - a0, b0 = h[MG_B0], CB = h[MG_B1] - b0;
    if (rep) {
        rep->alignments_a = CA;
        rep->alignments_b = CB;
    }
    if (CA > 0xFFFFFFFFull || CB > 0xFFFFFFFFull || CA + CB > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    const uint64_t C = CA + CB;
    if (rep) rep->alignments = C;
    const bool ops = cigar != nullptr;
    if (ops && (C + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    FmSlab lay;
    const uint64_t o_nops = lay.carve((C + 1) * 8), o_src = lay.carve((C ? C : 1) * 4);
    KTRY(slab.take(ctx, FM_SLOT_RESCUE_SLAB, lay.size));
    uint64_t *const nops = (uint64_t *)((char *)slab.p + o_nops);
    uint32_t *const src = (uint32_t *)((char *)slab.p + o_src);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_rescue_merge_place, dim3(fm_grid(C + 1, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, A.chain_index, B.chain_index, V,
                           a0, b0, CA, C, A.cigar_index, B.cigar_index, src, nops, d_ctl);
        KCHECK(hipGetLastError());
    }
    uint64_t total = 0;
    if (ops) {
        KTRY(kiss_scan_u64(ctx, nops, nops, C + 1));
        KCHECK(hipMemcpyAsync(&total, nops + C, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    KTRY(ctl.fetch());
    ev.mark(1);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (h[MG_BAD]) return KISS_HIP_E_INVALID; // a cigar index decreases
    if (rep) {
        rep->cigar_ops = total;
        rep->ms_place = ev.ms(0, 1);
    }
    // (the totals are in the report: the caller's second call)
    if (aln_capacity < C || (ops && cigar_capacity < total)) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        const uint64_t items = (C > V ? C : V) + 1;
        hipLaunchKernelGGL(k_rescue_merge_emit, dim3(fm_grid(items, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, A.alns, B.alns, A.chain_index,
                           B.chain_index, V, a0, b0, CA, C, (const uint32_t *)src, (const uint64_t *)nops, alns, chain_index, source,
                           ops ? cigar_index : nullptr);
        KCHECK(hipGetLastError());
        if (ops && total) {
            hipLaunchKernelGGL(k_rescue_merge_ops, dim3(fm_grid(total, RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, A.cigar, A.cigar_index, B.cigar,
                               B.cigar_index, CA, C, (const uint32_t *)src, (const uint64_t *)nops, total, cigar);
            KCHECK(hipGetLastError());
        }
    }
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) rep->ms_copy = ev.ms(1, 2);
    return KISS_HIP_OK;
}

int merge_args_check(const MergeIn &A, const MergeIn &B, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar,
                     const uint64_t *cigar_index, uint64_t cigar_capacity)
{
    if (!A.alns || !A.chain_index || !B.alns || !B.chain_index || !alns || !chain_index) return KISS_HIP_E_INVALID;
    const bool ca = A.cigar || A.cigar_index, cb = B.cigar || B.cigar_index, co = cigar || cigar_index;
    if ((ca && !(A.cigar && A.cigar_index)) || (cb && !(B.cigar && B.cigar_index)) || (co && !(cigar && cigar_index))) return KISS_HIP_E_INVALID;
    if (ca != cb || ca != co || (!co && cigar_capacity)) return KISS_HIP_E_INVALID; // the ops of both sets and room for them, or none
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_rescue_dev(kiss_hip_ctx *ctx, const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q,
                            const kiss_hip_aln *alns, uint64_t aln_count, const uint64_t *read_index, uint64_t n, const uint64_t *bounds,
                            uint64_t R, const kiss_hip_rescue_params *params, kiss_hip_chain *chains, uint64_t *chain_index,
                            uint32_t *origin, uint64_t chain_capacity, kiss_hip_rescue_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_rescue_report{};
        report->P = Q / 2;
    }
    KTRY(rescue_args_check(pairs, hits, hit_index, Q, alns, read_index, n, bounds, R, params, chains, chain_index));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) { // chain_index[0] = 0
        KTRY(kiss_zero_u32(ctx, chain_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    RescueP P;
    P.ins_min = params->ins_min;
    P.ins_max = params->ins_max;
    P.max_anchors = params->max_anchors;
    P.min_score = params->min_anchor_score;
    P.max_width = params->max_width;
    FmEvents ev(ctx, report != nullptr);
    const int rc = rescue_steps(ctx, pairs, hits, hit_index, Q, alns, aln_count, read_index, n, bounds, R, P, chains, chain_index, origin,
                                chain_capacity, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_rescue_host(const kiss_hip_pair *pairs, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q,
                             const kiss_hip_aln *alns, uint64_t aln_count, const uint64_t *read_index, uint64_t n, const uint64_t *bounds,
                             uint64_t R, const kiss_hip_rescue_params *params, kiss_hip_chain *chains, uint64_t *chain_index,
                             uint32_t *origin, uint64_t chain_capacity, kiss_hip_rescue_report *report, int device)
{
    if (report) {
        *report = kiss_hip_rescue_report{};
        report->P = Q / 2;
    }
    KTRY(rescue_args_check(pairs, hits, hit_index, Q, alns, read_index, n, bounds, R, params, chains, chain_index));
    if (Q == 0) {
        chain_index[0] = 0;
        return KISS_HIP_OK;
    }
    if (!fm_index_ascending(hit_index, Q, false) || !fm_index_ascending(read_index, Q, true)) return KISS_HIP_E_INVALID;
    const uint64_t H = hit_index[Q];
    if (H >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    // Q * max_anchors * ceil((ins_max - ins_min + 1) / max_width) chains always suffice, and no anchor is used twice
    const uint64_t per = ((uint64_t)(params->ins_max - params->ins_min) + params->max_width) / params->max_width; // (at most 2^32)
    uint64_t anchors = Q * (uint64_t)params->max_anchors;                                                         // (below 2^63)
    if (anchors > H) anchors = H;
    const uint64_t bound = anchors * per; // (H is below 2^32)
    return kiss_one_shot_cached(device, fm_host_max_n(0, 2 * Q + 1), [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t P = Q / 2, V = 2 * Q;
        const uint64_t cap = chain_capacity < bound ? chain_capacity : bound; // (no more chains than the header's bound)
        FmStage st(ctx);
        const kiss_hip_pair *dpairs = st.up(pairs, P * sizeof(kiss_hip_pair));
        const kiss_hip_hit *dhits = st.up(hits, H * sizeof(kiss_hip_hit));
        const uint64_t *dhidx = st.up(hit_index, (Q + 1) * 8);
        const kiss_hip_aln *dalns = st.up(alns, aln_count * sizeof(kiss_hip_aln));
        const uint64_t *dridx = st.up(read_index, (Q + 1) * 8);
        const uint64_t *dbounds = st.up(bounds, (R + 1) * 8);
        kiss_hip_chain *dchains = st.room<kiss_hip_chain>(true, cap * sizeof(kiss_hip_chain));
        uint64_t *dcidx = st.room<uint64_t>(true, (V + 1) * 8);
        uint32_t *dorigin = st.room<uint32_t>(origin != nullptr, cap * 4);
        if (st.rc) return st.rc;
        kiss_hip_rescue_report r{};
        const int rc = kiss_hip_fmi_rescue_dev(ctx, dpairs, dhits, dhidx, Q, dalns, aln_count, dridx, n, dbounds, R, params, dchains, dcidx,
                                               dorigin, cap, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(chain_index, dcidx, (V + 1) * 8);
        st.down(chains, dchains, r.chains * sizeof(kiss_hip_chain));
        if (origin) st.down(origin, dorigin, r.chains * 4);
        return st.rc;
    });
}

int kiss_hip_fmi_aln_merge_dev(kiss_hip_ctx *ctx, const kiss_hip_aln *alns_a, const uint64_t *chain_index_a, const uint32_t *cigar_a,
                               const uint64_t *cigar_index_a, const kiss_hip_aln *alns_b, const uint64_t *chain_index_b,
                               const uint32_t *cigar_b, const uint64_t *cigar_index_b, uint64_t V, kiss_hip_aln *alns,
                               uint64_t aln_capacity, uint64_t *chain_index, uint32_t *source, uint32_t *cigar, uint64_t *cigar_index,
                               uint64_t cigar_capacity, kiss_hip_merge_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_merge_report{};
        report->V = V;
    }
    const MergeIn A{alns_a, chain_index_a, cigar_a, cigar_index_a}, B{alns_b, chain_index_b, cigar_b, cigar_index_b};
    KTRY(merge_args_check(A, B, alns, chain_index, cigar, cigar_index, cigar_capacity));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    const int rc = merge_steps(ctx, A, B, V, alns, aln_capacity, chain_index, source, cigar, cigar_index, cigar_capacity, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_aln_merge_host(const kiss_hip_aln *alns_a, const uint64_t *chain_index_a, const uint32_t *cigar_a,
                                const uint64_t *cigar_index_a, const kiss_hip_aln *alns_b, const uint64_t *chain_index_b,
                                const uint32_t *cigar_b, const uint64_t *cigar_index_b, uint64_t V, kiss_hip_aln *alns,
                                uint64_t aln_capacity, uint64_t *chain_index, uint32_t *source, uint32_t *cigar, uint64_t *cigar_index,
                                uint64_t cigar_capacity, kiss_hip_merge_report *report, int device)
{
    if (report) {
        *report = kiss_hip_merge_report{};
        report->V = V;
    }
    const MergeIn A{alns_a, chain_index_a, cigar_a, cigar_index_a}, B{alns_b, chain_index_b, cigar_b, cigar_index_b};
    KTRY(merge_args_check(A, B, alns, chain_index, cigar, cigar_index, cigar_capacity));
    if (V > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (!fm_index_ascending(chain_index_a, V, false) || !fm_index_ascending(chain_index_b, V, false)) return KISS_HIP_E_INVALID;
    // (alns_a and alns_b are indexed from 0, as the align call writes them)
    const uint64_t CA = chain_index_a[V] - chain_index_a[0], CB = chain_index_b[V] - chain_index_b[0], C = CA + CB;
    if (report) {
        report->alignments_a = CA;
        report->alignments_b = CB;
        report->alignments = C;
    }
    if (CA > 0xFFFFFFFFull || CB > 0xFFFFFFFFull || C > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    const bool ops = cigar != nullptr;
    // (the ops are uploaded from the first one a set uses, its index from 0: the kernels see cigar_index[0] = 0)
    std::vector<uint64_t> ia(ops ? CA + 1 : 0), ib(ops ? CB + 1 : 0);
    if (ops) {
        if (!fm_index_ascending(cigar_index_a, CA, false) || !fm_index_ascending(cigar_index_b, CB, false)) return KISS_HIP_E_INVALID;
        for (uint64_t i = 0; i <= CA; i++) ia[i] = cigar_index_a[i] - cigar_index_a[0];
        for (uint64_t i = 0; i <= CB; i++) ib[i] = cigar_index_b[i] - cigar_index_b[0];
    }
    const uint64_t OA = ops ? ia[CA] : 0, OB = ops ? ib[CB] : 0, O = OA + OB; // the ops of either set
    return kiss_one_shot_cached(device, fm_host_max_n(0, C + 1, V + 1), [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t acap = aln_capacity < C ? aln_capacity : C, ocap = cigar_capacity < O ? cigar_capacity : O;
        FmStage st(ctx);
        const kiss_hip_aln *da = st.up(alns_a, CA * sizeof(kiss_hip_aln)), *db = st.up(alns_b, CB * sizeof(kiss_hip_aln));
        const uint64_t *dia = st.up(chain_index_a, (V + 1) * 8), *dib = st.up(chain_index_b, (V + 1) * 8);
        const uint32_t *dca = ops ? st.up(cigar_a + cigar_index_a[0], OA * 4) : nullptr;
        const uint32_t *dcb = ops ? st.up(cigar_b + cigar_index_b[0], OB * 4) : nullptr;
        const uint64_t *doa = ops ? st.up(ia.data(), (CA + 1) * 8) : nullptr, *dob = ops ? st.up(ib.data(), (CB + 1) * 8) : nullptr;
        kiss_hip_aln *dalns = st.room<kiss_hip_aln>(true, acap * sizeof(kiss_hip_aln));
        uint64_t *dcidx = st.room<uint64_t>(true, (V + 1) * 8);
        uint32_t *dsrc = st.room<uint32_t>(source != nullptr, acap * 4);
        uint32_t *dcig = st.room<uint32_t>(ops, ocap * 4);
        uint64_t *doidx = st.room<uint64_t>(ops, (C + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_merge_report r{};
        const int rc = kiss_hip_fmi_aln_merge_dev(ctx, da, dia, dca, doa, db, dib, dcb, dob, V, dalns, acap, dcidx, dsrc, dcig, doidx,
                                                  ops ? ocap : 0, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(alns, dalns, C * sizeof(kiss_hip_aln));
        st.down(chain_index, dcidx, (V + 1) * 8);
        if (source) st.down(source, dsrc, C * 4);
        if (ops) st.down(cigar_index, doidx, (C + 1) * 8);
        if (ops) st.down(cigar, dcig, r.cigar_ops * 4);
        return st.rc;
    });
}

} // extern "C"
