// fm_insert.hip -- FM-index: the insert size of a paired library, estimated from the pairs (kiss_hip_fmi_insert_*).
//
// The reference has no such function; the definition is in include/kiss_hip_insert.h and restated in
// tests/fm_insert_model.py.  The input is what kiss_hip_fmi_select_dev wrote (hits, hit_index) plus the alignment records its
// hits point at, as in fm_pair.hip.  No index, no text and no read is looked at.
//
//   hist  : ONE LANE PER PAIR, grid-stride.  A lane holds its three entries of hit_index against each other and against the last
//           one (so it reads no hit outside the array even when the index is broken; a broken index fails the call), classes
//           the pair from the first hit of either mate and, for a sample, counts T.  A library puts 10^5 .. 10^6 samples into a
//           few hundred bins, so the counts of a workgroup go into a histogram of its own in LDS over the first IN_WINDOW bins
//           (64 KiB: two workgroups per CU) and reach the global one once per non-zero bin at the end; a T past the window goes
//           to the global bin at once.  The class counts are ballots, one atomic per class and wave.
//   stats : ONE WORKGROUP.  Each wave sums a contiguous stretch of the bins; the wave that holds a rank walks its stretch again
//           with a prefix sum over 64 bins per step; the used range, its sum and its squared deviations are two coalesced
//           sweeps; one lane does the divisions and the square root and writes the report's words.
//   The host fetches those words once.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_insert.h"
#include <algorithm>

namespace {

constexpr int IN_THREADS = 256;
constexpr uint32_t IN_WINDOW = 16384; // bins of the workgroup's own histogram
constexpr unsigned IN_MAX_BLOCKS = 1024;
constexpr int ST_THREADS = 1024;
constexpr int ST_WAVES = ST_THREADS / 64;

// control block of a call (u64 words); the six classes in the order of the definition, then the words of k_insert_stats
enum {
    IN_BAD = 0, IN_TOTAL = 1, IN_CLASS = 2, // IN_CLASS + c: unmapped, bad_input, low_mapq, discordant, too_long, samples
    IN_USED = 8, IN_FLAGS = 9, IN_Q25 = 10, IN_Q50 = 11, IN_Q75 = 12, IN_MEAN = 13, IN_SD = 14, IN_MIN = 15, IN_MAX = 16, IN_CTL_WORDS = 18
};
enum { C_UNMAPPED = 0, C_BADIN = 1, C_LOWQ = 2, C_DISC = 3, C_LONG = 4, C_SAMPLE = 5, C_COUNT = 6, C_NONE = 6, C_BROKEN = 7 };

struct InsP {
    uint32_t min_mapq, max_insert, min_samples, out_mult, map_mult, sd_mult;
};

// every load starts at a multiple of its own size and is not merged with its neighbours, as in fm_pair.hip
__device__ __forceinline__ uint32_t in_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t in_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ unsigned long long in_wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(IN_THREADS) void k_insert_hist(const kiss_hip_hit *__restrict__ hits, const uint64_t *__restrict__ hit_index,
                                                           uint64_t Q, const kiss_hip_aln *__restrict__ alns, uint64_t aln_count, InsP P,
                                                           uint32_t *__restrict__ hist, unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t bins[IN_WINDOW];
    const uint32_t window = P.max_insert + 1 < IN_WINDOW ? P.max_insert + 1 : IN_WINDOW;
    for (uint32_t i = threadIdx.x; i < window; i += IN_THREADS) bins[i] = 0;
    __syncthreads();

    const uint64_t NP = Q / 2, total = in_ld64(hit_index + Q), stride = (uint64_t)gridDim.x * IN_THREADS;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[IN_TOTAL] = total;
    uint32_t acc[C_COUNT] = {0, 0, 0, 0, 0, 0}; // the same in all lanes of a wave
    bool broken = false;
    for (uint64_t first = (uint64_t)blockIdx.x * IN_THREADS; first < NP; first += stride) { // (the same trips for every lane)
        const uint64_t p = first + threadIdx.x;
        uint32_t cls = C_NONE, T = 0;
        if (p < NP) {
            const uint64_t s1 = in_ld64(hit_index + 2 * p), s2 = in_ld64(hit_index + 2 * p + 1), s3 = in_ld64(hit_index + 2 * p + 2);
            if (s1 > s2 || s2 > s3 || s3 > total) {
                cls = C_BROKEN;
            } else if (s1 == s2 || s2 == s3) {
                cls = C_UNMAPPED;
            } else {
                const kiss_hip_hit *h1 = hits + s1, *h2 = hits + s2; // (s1 < s2 < s3 <= total: inside hits)
                const uint32_t a1 = in_ld32(&h1->aln), a2 = in_ld32(&h2->aln), m1 = in_ld32(&h1->mapq), m2 = in_ld32(&h2->mapq);
                const uint32_t rev1 = in_ld32(&h1->flags) & KISS_HIP_HIT_REVERSE, rev2 = in_ld32(&h2->flags) & KISS_HIP_HIT_REVERSE;
                const uint32_t ref1 = in_ld32(&h1->ref), ref2 = in_ld32(&h2->ref);
                if (a1 >= aln_count || a2 >= aln_count) {
                    cls = C_BADIN;
                } else if (m1 < P.min_mapq || m2 < P.min_mapq) {
                    cls = C_LOWQ;
                } else {
                    const long long tb1 = in_ld32(&alns[a1].tbeg), te1 = in_ld32(&alns[a1].tend), tb2 = in_ld32(&alns[a2].tbeg),
                                    te2 = in_ld32(&alns[a2].tend);
                    const long long ftb = rev1 ? tb2 : tb1, fte = rev1 ? te2 : te1, rtb = rev1 ? tb1 : tb2, rte = rev1 ? te1 : te2;
                    const long long t = rte - ftb;
                    if (ref1 != ref2 || rev1 == rev2 || tb1 >= te1 || tb2 >= te2 || !(ftb <= rtb && fte <= rte)) {
                        cls = C_DISC;
                    } else if (t > (long long)P.max_insert) {
                        cls = C_LONG;
                    } else {
                        cls = C_SAMPLE;
                        T = (uint32_t)t; // (ftb <= rtb < rte: 1 <= t <= max_insert)
                    }
                }
            }
        }
        if (cls == C_SAMPLE) {
            if (T < IN_WINDOW) atomicAdd(&bins[T], 1u);
            else atomicAdd(&hist[T], 1u);
        }
        broken = broken || cls == C_BROKEN;
#pragma unroll
        for (uint32_t c = 0; c < C_COUNT; c++) acc[c] += (uint32_t)__popcll(__ballot(cls == c));
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < window; i += IN_THREADS) {
        const uint32_t c = bins[i];
        if (c) atomicAdd(&hist[i], c);
    }
    if (broken) ctl[IN_BAD] = 1;
    if (lane_id() == 0) {
#pragma unroll
        for (uint32_t c = 0; c < C_COUNT; c++)
            if (acc[c]) atomicAdd(&ctl[IN_CLASS + c], (unsigned long long)acc[c]);
    }
}

// the sum of v over the workgroup, in every thread (red: ST_WAVES words, free to be used again after the call's first barrier)
__device__ __forceinline__ unsigned long long st_block_sum(unsigned long long v, unsigned long long *red)
{
    v = in_wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int k = 0; k < ST_WAVES; k++) t += red[k];
    return t;
}

// One workgroup; ctl's words of the statistics are zero when it starts and stay zero without KISS_HIP_INSERT_OK.
__global__ __launch_bounds__(ST_THREADS) void k_insert_stats(const uint32_t *__restrict__ hist, InsP P, unsigned long long *__restrict__ ctl)
{
    __shared__ unsigned long long wsum[ST_WAVES], red[ST_WAVES];
    __shared__ uint32_t quart[3];
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t nbins = P.max_insert + 1;
    const uint32_t per = ((nbins + ST_WAVES - 1) / ST_WAVES + 63u) & ~63u; // the stretch of a wave, whole steps of 64
    const uint32_t lo = w * per < nbins ? w * per : nbins, hi = lo + per < nbins ? lo + per : nbins;

    unsigned long long s = 0;
    for (uint32_t i = lo + lane; i < hi; i += 64) s += in_ld32(hist + i);
    s = in_wave_sum(s);
    if (lane == 0) wsum[w] = s;
    __syncthreads();
    unsigned long long before = 0, N = 0; // the samples in front of this wave's stretch; all of them
    for (uint32_t k = 0; k < ST_WAVES; k++) {
        before += k < w ? wsum[k] : 0ull;
        N += wsum[k];
    }
    const unsigned long long need = P.min_samples > 1u ? P.min_samples : 1u;
    if (N < need) return;

    // the three ranks: the wave whose stretch holds one walks it again
    for (uint32_t j = 1; j <= 3; j++) {
        const unsigned long long r = (unsigned long long)j * N / 4ull;
        if (r < before || r >= before + wsum[w]) continue;
        unsigned long long cum = before;
        for (uint32_t g = lo; g < hi; g += 64) {
            unsigned long long incl = g + lane < hi ? in_ld32(hist + g + lane) : 0u;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = __shfl_up(incl, o, 64);
                if ((int)lane >= o) incl += t;
            }
            const unsigned long long tot = __shfl(incl, 63, 64);
            if (cum + tot > r) {
                const unsigned long long m = __ballot(cum + incl > r);
                if (lane == 0) quart[j - 1] = g + (uint32_t)__builtin_ctzll(m);
                break;
            }
            cum += tot;
        }
    }
    __syncthreads();
    const long long q25 = quart[0], q50 = quart[1], q75 = quart[2], iqr = q75 - q25;
    long long ulo = q25 - (long long)P.out_mult * iqr, uhi = q75 + (long long)P.out_mult * iqr;
    ulo = ulo < 0 ? 0 : ulo;
    uhi = uhi > (long long)P.max_insert ? (long long)P.max_insert : uhi;

    unsigned long long m = 0, sum = 0;
    for (long long T = ulo + threadIdx.x; T <= uhi; T += ST_THREADS) {
        const unsigned long long c = in_ld32(hist + T);
        m += c;
        sum += c * (unsigned long long)T;
    }
    const unsigned long long M = st_block_sum(m, red);
    sum = st_block_sum(sum, red);
    const long long mean = (long long)((sum + M / 2ull) / M); // (M >= 1: q25 lies inside the range)
    unsigned long long dev2 = 0;
    for (long long T = ulo + threadIdx.x; T <= uhi; T += ST_THREADS) {
        const unsigned long long c = in_ld32(hist + T), d = (unsigned long long)(T > mean ? T - mean : mean - T);
        dev2 += c * d * d;
    }
    dev2 = st_block_sum(dev2, red);
    if (threadIdx.x == 0) {
        const unsigned long long var = dev2 / M; // (below 2^32)
        unsigned long long sd = (unsigned long long)sqrt((double)var);
        while (sd * sd > var) sd--;
        while ((sd + 1) * (sd + 1) <= var) sd++;
        const long long a = q25 - (long long)P.map_mult * iqr, b = mean - (long long)P.sd_mult * (long long)sd;
        const long long c = q75 + (long long)P.map_mult * iqr, d = mean + (long long)P.sd_mult * (long long)sd;
        const long long ins_min = a < b ? a : b, ins_max = c > d ? c : d;
        ctl[IN_USED] = M;
        ctl[IN_FLAGS] = KISS_HIP_INSERT_OK;
        ctl[IN_Q25] = (unsigned long long)q25;
        ctl[IN_Q50] = (unsigned long long)q50;
        ctl[IN_Q75] = (unsigned long long)q75;
        ctl[IN_MEAN] = (unsigned long long)mean;
        ctl[IN_SD] = sd;
        ctl[IN_MIN] = (unsigned long long)(ins_min < 0 ? 0 : ins_min);
        ctl[IN_MAX] = (unsigned long long)ins_max;
    }
}

int insert_steps(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                 uint64_t aln_count, const InsP &P, uint32_t *hist, kiss_hip_insert_report *rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t NP = Q / 2, nbins = (uint64_t)P.max_insert + 1;
    FmCtl<IN_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_INSERT_CTL));
    DevBuf own;
    if (!hist) {
        KTRY(own.take(ctx, FM_SLOT_INSERT_HIST, nbins * 4));
        hist = (uint32_t *)own.p;
    }
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    KTRY(kiss_zero_u32(ctx, hist, nbins));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, NP);
        const uint64_t blocks = div_up(NP, IN_THREADS);
        hipLaunchKernelGGL(k_insert_hist, dim3((unsigned)(blocks < IN_MAX_BLOCKS ? blocks : IN_MAX_BLOCKS)), dim3(IN_THREADS), 0, ctx->stream,
                           hits, hit_index, Q, alns, aln_count, P, hist, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, nbins);
        hipLaunchKernelGGL(k_insert_stats, dim3(1), dim3(ST_THREADS), 0, ctx->stream, hist, P, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KTRY(ctl.fetch_sync());
    if (h[IN_BAD]) return KISS_HIP_E_INVALID;                        // hit_index decreases
    if (h[IN_TOTAL] >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED; // as the pair call
    rep->unmapped = h[IN_CLASS + C_UNMAPPED];
    rep->bad_input = h[IN_CLASS + C_BADIN];
    rep->low_mapq = h[IN_CLASS + C_LOWQ];
    rep->discordant = h[IN_CLASS + C_DISC];
    rep->too_long = h[IN_CLASS + C_LONG];
    rep->samples = h[IN_CLASS + C_SAMPLE];
    rep->used = h[IN_USED];
    rep->flags = (uint32_t)h[IN_FLAGS];
    rep->q25 = (uint32_t)h[IN_Q25];
    rep->q50 = (uint32_t)h[IN_Q50];
    rep->q75 = (uint32_t)h[IN_Q75];
    rep->mean = (uint32_t)h[IN_MEAN];
    rep->sd = (uint32_t)h[IN_SD];
    rep->ins_min = (uint32_t)h[IN_MIN];
    rep->ins_max = (uint32_t)h[IN_MAX];
    rep->ins_mean = rep->mean;
    rep->ms_hist = ev.ms(0, 1);
    rep->ms_stats = ev.ms(1, 2);
    return KISS_HIP_OK;
}

int insert_args_check(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                      const kiss_hip_insert_params *params, const kiss_hip_insert_report *report)
{
    if (!hits || !hit_index || !alns || !params || !report) return KISS_HIP_E_INVALID;
    if (Q & 1ull) return KISS_HIP_E_INVALID;
    if (params->max_insert < 1u || params->max_insert > KISS_HIP_INSERT_MAX) return KISS_HIP_E_INVALID;
    if (params->out_mult > 255u || params->map_mult > 255u || params->sd_mult > 255u) return KISS_HIP_E_INVALID;
    if (Q > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_insert_dev(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                            uint64_t aln_count, const kiss_hip_insert_params *params, uint32_t *hist, kiss_hip_insert_report *report,
                            void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_insert_report{};
        report->P = Q / 2;
    }
    KTRY(insert_args_check(hits, hit_index, Q, alns, params, report));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) { // an empty histogram, written when the call returns
        if (hist) {
            KTRY(kiss_zero_u32(ctx, hist, (uint64_t)params->max_insert + 1));
            KCHECK(hipStreamSynchronize(ctx->stream));
        }
        return KISS_HIP_OK;
    }
    InsP P;
    P.min_mapq = params->min_mapq;
    P.max_insert = params->max_insert;
    P.min_samples = params->min_samples;
    P.out_mult = params->out_mult;
    P.map_mult = params->map_mult;
    P.sd_mult = params->sd_mult;
    FmEvents ev(ctx, true);
    const int rc = insert_steps(ctx, hits, hit_index, Q, alns, aln_count, P, hist, report, ev);
    return fm_leave(ctx, ev, rc, &report->ms_total);
}

int kiss_hip_fmi_insert_host(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns, uint64_t aln_count,
                             const kiss_hip_insert_params *params, uint32_t *hist, kiss_hip_insert_report *report, int device)
{
    if (report) {
        *report = kiss_hip_insert_report{};
        report->P = Q / 2;
    }
    KTRY(insert_args_check(hits, hit_index, Q, alns, params, report));
    const uint64_t hist_bytes = ((uint64_t)params->max_insert + 1) * 4;
    if (Q == 0) {
        if (hist) std::fill_n(hist, (uint64_t)params->max_insert + 1, 0u);
        return KISS_HIP_OK;
    }
    if (!fm_index_ascending(hit_index, Q, false)) return KISS_HIP_E_INVALID;
    const uint64_t H = hit_index[Q];
    if (H >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return kiss_one_shot_cached(device, fm_host_max_n(0, 0), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const kiss_hip_hit *dhits = st.up(hits, H * sizeof(kiss_hip_hit));
        const uint64_t *dhidx = st.up(hit_index, (Q + 1) * 8);
        const kiss_hip_aln *dalns = st.up(alns, aln_count * sizeof(kiss_hip_aln));
        uint32_t *dhist = st.room<uint32_t>(hist != nullptr, hist_bytes);
        if (st.rc) return st.rc;
        kiss_hip_insert_report r{};
        const int rc = kiss_hip_fmi_insert_dev(ctx, dhits, dhidx, Q, dalns, aln_count, params, dhist, &r, nullptr);
        *report = r;
        if (rc) return rc;
        if (hist) st.down(hist, dhist, hist_bytes);
        return st.rc;
    });
}

} // extern "C"
