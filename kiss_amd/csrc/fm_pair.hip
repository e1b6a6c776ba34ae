// fm_pair.hip -- FM-index: the mappings of two mates paired (kiss_hip_fmi_pair_*).
//
// The reference has no such function; the definition is in include/kiss_hip.h and restated in tests/fm_pair_model.py.  The
// input is what kiss_hip_fmi_select_dev wrote (hits, hit_index) plus the alignment records its hits point at.  No index, no
// text and no read is looked at.
//
//   head  : one kernel checks that hit_index never decreases and fetches its last entry; the host looks at both once (pairs is
//           untouched when the call fails, and the kernel below can trust the segments).
//   walk  : ONE WAVE PER PAIR (a wave takes pairs p, p + waves, ...: its counts reach the control block once).  The hits of
//           mate 2 live in the lanes, 64 at a time; the eligible hits of mate 1 are loaded 64 at a time too and handed out by
//           shuffle, one per step: lane l scores (x, 64 k + l).  Sweep 1 keeps the best (S, x, y) per lane and reduces it
//           over the wave with the tie rule; sweep 2 goes over the same combinations again for sub1, sub2 and n_conc --
//           recomputing a score is cheaper than storing |E1| * |E2| of them.  The first chunk of either mate stays in
//           registers between the sweeps: a pair with at most 64 hits per mate (nearly all) loads its records once.
#include "fm_internal.hpp"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr unsigned PR_MAX_BLOCKS = 4096;
constexpr uint32_t PR_SCORE_TOP = 1u << 30; // select writes no score this large

// control block of a call (u64 words)
enum { PR_BAD = 0, PR_TOTAL = 1, PR_ELIG = 2, PR_COMB = 3, PR_CONC = 4, PR_PROPER = 5, PR_PROMOTED = 6, PR_LIFTED = 7, PR_BADIN = 8, PR_MAXC = 9, PR_CTL_WORDS = 12 };

struct PairP {
    uint32_t ins_min, ins_max, ins_mean, pen_coef, pen_max, mapq_coef, mapq_max;
};

// Every load of this file starts at a multiple of its own size, as in fm_select.hip: the fields of a record
// and the entries of an index are fetched through relaxed loads of wavefront scope -- ordinary global_load_dword / _dwordx2
// that the compiler does not merge with their neighbours into a 16-byte load at an address that is only 4- or 8-byte aligned
// (hits + 32 h + 12, alns + 48 a + 16, pairs + 40 p).  pr_st32: the same for the fields of a pair.
__device__ __forceinline__ uint32_t pr_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t pr_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void pr_st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

__device__ __forceinline__ uint64_t pr_wave_max64(uint64_t v)
{
    for (int o = 32; o; o >>= 1) {
        const uint64_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t pr_wave_max32(uint32_t v)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t pr_wave_min32(uint32_t v)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t pr_wave_sum64(uint64_t v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a hit_index that decreases; its last entry
__global__ __launch_bounds__(PR_THREADS) void k_mate_head(const uint64_t *__restrict__ hit_index, uint64_t Q, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (g == 0) ctl[PR_TOTAL] = pr_ld64(hit_index + Q);
    const bool bad = g < Q && pr_ld64(hit_index + g + 1) < pr_ld64(hit_index + g);
    if (__ballot(bad) && lane_id() == 0) ctl[PR_BAD] = 1;
}

// what a lane knows of one hit
struct Row {
    uint32_t tb, te, ref, rev, score;
    bool elig, bad;
};

// lane l: hit first + l of a segment of which `left` hits are left from `first` on (no hit: not eligible, not bad)
__device__ __forceinline__ Row pr_row(const kiss_hip_hit *__restrict__ hits, const kiss_hip_aln *__restrict__ alns, uint64_t aln_count,
                                      uint64_t first, uint64_t left)
{
    Row r{};
    const uint32_t lane = lane_id();
    if (lane < left) {
        const kiss_hip_hit *h = hits + first + lane;
        const uint32_t aln = pr_ld32(&h->aln), flags = pr_ld32(&h->flags), score = pr_ld32(&h->score), head = pr_ld32(&h->head);
        r.ref = pr_ld32(&h->ref);
        r.rev = flags & KISS_HIP_HIT_REVERSE;
        r.score = score;
        r.bad = aln >= aln_count || score >= PR_SCORE_TOP;
        if (!r.bad) {
            r.tb = pr_ld32(&alns[aln].tbeg);
            r.te = pr_ld32(&alns[aln].tend);
            r.elig = head == 0 && r.tb < r.te;
        }
    }
    return r;
}

// the insert of a forward and a reverse hit on one record: false when they do not face each other in order
__device__ __forceinline__ bool pr_insert(uint32_t x_tb, uint32_t x_te, uint32_t x_rev, uint32_t y_tb, uint32_t y_te, long long &T)
{
    const long long ftb = x_rev ? y_tb : x_tb, fte = x_rev ? y_te : x_te, rtb = x_rev ? x_tb : y_tb, rte = x_rev ? x_te : y_te;
    T = rte - ftb;
    return ftb <= rtb && fte <= rte;
}

// S(x, y) of the hit x (the same in all lanes) and the lane's hit y; 0: not concordant
__device__ __forceinline__ uint32_t pr_score(const PairP &P, uint32_t x_tb, uint32_t x_te, uint32_t x_ref, uint32_t x_rev, uint32_t x_score,
                                             const Row &y)
{
    long long T;
    if (!y.elig || y.ref != x_ref || y.rev == x_rev || !pr_insert(x_tb, x_te, x_rev, y.tb, y.te, T)) return 0;
    if (T < (long long)P.ins_min || T > (long long)P.ins_max) return 0;
    const unsigned long long dev = (unsigned long long)(T > (long long)P.ins_mean ? T - (long long)P.ins_mean : (long long)P.ins_mean - T);
    unsigned long long pen = dev * (unsigned long long)P.pen_coef / 256ull; // (dev < 2^32, pen_coef < 2^16)
    pen = pen < (unsigned long long)P.pen_max ? pen : (unsigned long long)P.pen_max;
    const long long S = (long long)x_score + (long long)y.score - (long long)pen;
    return S < 1 ? 1u : (uint32_t)S; // (both scores are below 2^30)
}

// every combination of an eligible hit of mate 1 and a hit of mate 2, once: f(S, x, y) in the lane that holds y, S = 0 when the
// combination is not concordant.  x0 / y0: the first chunk of either mate, already loaded.
template <typename F>
__device__ __forceinline__ void pr_sweep(const kiss_hip_hit *__restrict__ hits, const kiss_hip_aln *__restrict__ alns, uint64_t aln_count,
                                         const PairP &P, uint64_t s1, uint64_t n1, uint64_t s2, uint64_t n2, const Row &x0, const Row &y0, F f)
{
    const uint32_t lane = lane_id();
    for (uint64_t b2 = 0; b2 < n2; b2 += 64) {
        const Row y = b2 ? pr_row(hits, alns, aln_count, s2 + b2, n2 - b2) : y0;
        if (!__ballot(y.elig)) continue;
        for (uint64_t b1 = 0; b1 < n1; b1 += 64) {
            const Row xs = b1 ? pr_row(hits, alns, aln_count, s1 + b1, n1 - b1) : x0;
            unsigned long long m = __ballot(xs.elig);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t x_tb = __shfl(xs.tb, j, 64), x_te = __shfl(xs.te, j, 64), x_ref = __shfl(xs.ref, j, 64),
                               x_rev = __shfl(xs.rev, j, 64), x_score = __shfl(xs.score, j, 64);
                f(pr_score(P, x_tb, x_te, x_ref, x_rev, x_score, y), (uint32_t)(b1 + (uint64_t)j), (uint32_t)(b2 + lane));
            }
        }
    }
}

// the chosen hit of a mate, the same in all lanes
struct Chosen {
    uint32_t tb, te, ref, rev, score, mapq;
};
__device__ __forceinline__ Chosen pr_chosen(const kiss_hip_hit *__restrict__ hits, const kiss_hip_aln *__restrict__ alns, uint64_t at)
{
    const kiss_hip_hit *h = hits + at;
    const uint32_t aln = pr_ld32(&h->aln); // (inside alns: the pair is not bad input)
    Chosen c;
    c.rev = pr_ld32(&h->flags) & KISS_HIP_HIT_REVERSE;
    c.mapq = pr_ld32(&h->mapq);
    c.score = pr_ld32(&h->score);
    c.ref = pr_ld32(&h->ref);
    c.tb = pr_ld32(&alns[aln].tbeg);
    c.te = pr_ld32(&alns[aln].tend);
    return c;
}

__device__ __forceinline__ uint32_t pr_mapq(const PairP &P, uint32_t own, uint32_t S, uint32_t sub)
{
    const unsigned long long m = (unsigned long long)P.mapq_coef * (unsigned long long)(S - sub) / (unsigned long long)S; // (sub <= S)
    const uint32_t pm = m < (unsigned long long)P.mapq_max ? (uint32_t)m : P.mapq_max;
    return own > pm ? own : pm;
}

// One wave per pair; hit_index never decreases (k_mate_head), so n1 and n2 are what they say.
__global__ __launch_bounds__(PR_THREADS) void k_mate_walk(const kiss_hip_hit *__restrict__ hits, const uint64_t *__restrict__ hit_index,
                                                         uint64_t NP, const kiss_hip_aln *__restrict__ alns, uint64_t aln_count, PairP P,
                                                         kiss_hip_pair *__restrict__ pairs, unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = lane_id();
    const uint64_t waves = (uint64_t)gridDim.x * PR_WAVES;
    unsigned long long a_elig = 0, a_comb = 0, a_conc = 0, a_maxc = 0, a_proper = 0, a_promoted = 0, a_lifted = 0, a_bad = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * PR_WAVES + (threadIdx.x >> 6); p < NP; p += waves) {
        const uint64_t s1 = pr_ld64(hit_index + 2 * p), s2 = pr_ld64(hit_index + 2 * p + 1), s3 = pr_ld64(hit_index + 2 * p + 2);
        const uint64_t n1 = s2 - s1, n2 = s3 - s2;
        uint32_t *const o = &pairs[p].hit1; // (ten dword stores: the caller's array need not be 8-byte aligned)

        // the eligible hits of either mate counted, a hit that cannot be used found
        const Row x0 = pr_row(hits, alns, aln_count, s1, n1), y0 = pr_row(hits, alns, aln_count, s2, n2);
        uint64_t e1 = (uint64_t)__popcll(__ballot(x0.elig)), e2 = (uint64_t)__popcll(__ballot(y0.elig));
        bool bad = __ballot(x0.bad || y0.bad) != 0;
        for (uint64_t b = 64; b < n1; b += 64) {
            const Row r = pr_row(hits, alns, aln_count, s1 + b, n1 - b);
            e1 += (uint64_t)__popcll(__ballot(r.elig));
            bad = bad || __ballot(r.bad) != 0;
        }
        for (uint64_t b = 64; b < n2; b += 64) {
            const Row r = pr_row(hits, alns, aln_count, s2 + b, n2 - b);
            e2 += (uint64_t)__popcll(__ballot(r.elig));
            bad = bad || __ballot(r.bad) != 0;
        }
        if (bad) {
            if (lane < 10) pr_st32(o + lane, lane == 2 ? (uint32_t)KISS_HIP_PAIR_BAD_INPUT : 0u);
            a_bad++;
            continue;
        }
        a_elig += e1 + e2;
        a_comb += e1 * e2;
        a_maxc = a_maxc > e1 * e2 ? a_maxc : e1 * e2;

        // sweep 1: the best (S, x, y) -- the largest S, then the smallest x, then the smallest y
        uint32_t bS = 0, bx = 0, by = 0;
        pr_sweep(hits, alns, aln_count, P, s1, n1, s2, n2, x0, y0, [&](uint32_t S, uint32_t x, uint32_t y) {
            if (S > bS || (S == bS && S && (x < bx || (x == bx && y < by)))) {
                bS = S;
                bx = x;
                by = y;
            }
        });
        const uint64_t key = bS ? ((uint64_t)bS << 32) | (uint64_t)(0xFFFFFFFFu - bx) : 0ull;
        const uint64_t top = pr_wave_max64(key);
        const uint32_t S = (uint32_t)(top >> 32);
        const bool proper = S != 0;
        uint32_t X = 0, Y = 0, sub1 = 0, sub2 = 0, n_conc = 0;
        if (proper) {
            X = 0xFFFFFFFFu - (uint32_t)top;
            Y = pr_wave_min32(key == top ? by : 0xFFFFFFFFu);
            // sweep 2: the best without x, the best without y, the concordant combinations
            uint32_t m1 = 0, m2 = 0;
            uint64_t cnt = 0;
            pr_sweep(hits, alns, aln_count, P, s1, n1, s2, n2, x0, y0, [&](uint32_t S2, uint32_t x, uint32_t y) {
                if (S2) {
                    cnt++;
                    if (x != X) m1 = m1 > S2 ? m1 : S2;
                    if (y != Y) m2 = m2 > S2 ? m2 : S2;
                }
            });
            sub1 = pr_wave_max32(m1);
            sub2 = pr_wave_max32(m2);
            const uint64_t total = pr_wave_sum64(cnt);
            a_conc += total;
            n_conc = total < 0xFFFFFFFFull ? (uint32_t)total : 0xFFFFFFFFu;
        }

        // the record, from the chosen hits (the same values in all lanes)
        uint32_t flags = 0, tlen = 0, score = 0, mapq1 = 0, mapq2 = 0;
        Chosen c1{}, c2{};
        if (n1) {
            c1 = pr_chosen(hits, alns, s1 + X);
            flags |= KISS_HIP_PAIR_MATE1_MAPPED;
        }
        if (n2) {
            c2 = pr_chosen(hits, alns, s2 + Y);
            flags |= KISS_HIP_PAIR_MATE2_MAPPED;
        }
        if (n1 && n2 && c1.ref == c2.ref) flags |= KISS_HIP_PAIR_SAME_REF;
        if (proper) {
            long long T;
            (void)pr_insert(c1.tb, c1.te, c1.rev, c2.tb, c2.te, T);
            flags |= KISS_HIP_PAIR_PROPER | (X ? (uint32_t)KISS_HIP_PAIR_PROMOTED1 : 0u) | (Y ? (uint32_t)KISS_HIP_PAIR_PROMOTED2 : 0u);
            tlen = (uint32_t)T;
            score = S;
            mapq1 = pr_mapq(P, c1.mapq, S, sub1);
            mapq2 = pr_mapq(P, c2.mapq, S, sub2);
            a_proper++;
            a_promoted += (X ? 1u : 0u) + (Y ? 1u : 0u);
            a_lifted += (mapq1 > c1.mapq ? 1u : 0u) + (mapq2 > c2.mapq ? 1u : 0u);
        } else {
            score = (n1 ? c1.score : 0u) + (n2 ? c2.score : 0u);
            mapq1 = n1 ? c1.mapq : 0u;
            mapq2 = n2 ? c2.mapq : 0u;
            if (flags & KISS_HIP_PAIR_SAME_REF) {
                const long long hi = c1.te > c2.te ? c1.te : c2.te, lo = c1.tb < c2.tb ? c1.tb : c2.tb;
                tlen = hi > lo ? (uint32_t)(hi - lo) : 0u;
            }
        }
        if (lane == 0) {
            pr_st32(o + 0, n1 ? (uint32_t)(s1 + X) : (uint32_t)KISS_HIP_PAIR_NONE); // (hit_index[Q] < 2^32 - 1)
            pr_st32(o + 1, n2 ? (uint32_t)(s2 + Y) : (uint32_t)KISS_HIP_PAIR_NONE);
            pr_st32(o + 2, flags);
            pr_st32(o + 3, tlen);
            pr_st32(o + 4, score);
            pr_st32(o + 5, sub1);
            pr_st32(o + 6, sub2);
            pr_st32(o + 7, mapq1);
            pr_st32(o + 8, mapq2);
            pr_st32(o + 9, n_conc);
        }
    }
    if (lane == 0) {
        if (a_elig) atomicAdd(&ctl[PR_ELIG], a_elig);
        if (a_comb) atomicAdd(&ctl[PR_COMB], a_comb);
        if (a_conc) atomicAdd(&ctl[PR_CONC], a_conc);
        if (a_proper) atomicAdd(&ctl[PR_PROPER], a_proper);
        if (a_promoted) atomicAdd(&ctl[PR_PROMOTED], a_promoted);
        if (a_lifted) atomicAdd(&ctl[PR_LIFTED], a_lifted);
        if (a_bad) atomicAdd(&ctl[PR_BADIN], a_bad);
        if (a_maxc) atomicMax(&ctl[PR_MAXC], a_maxc);
    }
}

int pair_steps(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
               uint64_t aln_count, const PairP &P, kiss_hip_pair *pairs, kiss_hip_pair_report *rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t NP = Q / 2;
    FmCtl<PR_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_PAIR_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_mate_head, dim3(fm_grid(Q + 1, PR_THREADS)), dim3(PR_THREADS), 0, ctx->stream, hit_index, Q, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[PR_BAD]) return KISS_HIP_E_INVALID;                  // hit_index decreases
    if (h[PR_TOTAL] >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED; // hit1 / hit2 are u32, and 0xFFFFFFFF is NONE
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, NP);
        const uint64_t blocks = div_up(NP, PR_WAVES);
        hipLaunchKernelGGL(k_mate_walk, dim3((unsigned)(blocks < PR_MAX_BLOCKS ? blocks : PR_MAX_BLOCKS)), dim3(PR_THREADS), 0, ctx->stream, hits,
                           hit_index, NP, alns, aln_count, P, pairs, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KTRY(ctl.fetch_sync());
    if (rep) {
        rep->eligible = h[PR_ELIG];
        rep->combinations = h[PR_COMB];
        rep->concordant = h[PR_CONC];
        rep->proper = h[PR_PROPER];
        rep->promoted = h[PR_PROMOTED];
        rep->lifted = h[PR_LIFTED];
        rep->bad_input = h[PR_BADIN];
        rep->max_combinations = h[PR_MAXC];
        rep->ms_check = ev.ms(0, 1);
        rep->ms_pair = ev.ms(1, 2);
    }
    return KISS_HIP_OK;
}

int pair_args_check(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                    const kiss_hip_pair_params *params, const kiss_hip_pair *pairs)
{
    if (!hits || !hit_index || !alns || !params || !pairs) return KISS_HIP_E_INVALID;
    if (Q & 1ull) return KISS_HIP_E_INVALID;
    if (params->ins_min > params->ins_max) return KISS_HIP_E_INVALID;
    if (params->pen_coef > 65535u || params->pen_max > 65535u || params->mapq_coef > 65535u || params->mapq_max > 255u) return KISS_HIP_E_INVALID;
    if (Q > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_pair_dev(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                          uint64_t aln_count, const kiss_hip_pair_params *params, kiss_hip_pair *pairs, kiss_hip_pair_report *report,
                          void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_pair_report{};
        report->P = Q / 2;
    }
    KTRY(pair_args_check(hits, hit_index, Q, alns, params, pairs));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) return KISS_HIP_OK;
    PairP P;
    P.ins_min = params->ins_min;
    P.ins_max = params->ins_max;
    P.ins_mean = params->ins_mean;
    P.pen_coef = params->pen_coef;
    P.pen_max = params->pen_max;
    P.mapq_coef = params->mapq_coef;
    P.mapq_max = params->mapq_max;
    FmEvents ev(ctx, report != nullptr);
    const int rc = pair_steps(ctx, hits, hit_index, Q, alns, aln_count, P, pairs, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_pair_host(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns, uint64_t aln_count,
                           const kiss_hip_pair_params *params, kiss_hip_pair *pairs, kiss_hip_pair_report *report, int device)
{
    if (report) {
        *report = kiss_hip_pair_report{};
        report->P = Q / 2;
    }
    KTRY(pair_args_check(hits, hit_index, Q, alns, params, pairs));
    if (Q == 0) return KISS_HIP_OK;
    if (!fm_index_ascending(hit_index, Q, false)) return KISS_HIP_E_INVALID;
    const uint64_t H = hit_index[Q];
    if (H >= 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return kiss_one_shot_cached(device, fm_host_max_n(0, 0), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const kiss_hip_hit *dhits = st.up(hits, H * sizeof(kiss_hip_hit));
        const uint64_t *dhidx = st.up(hit_index, (Q + 1) * 8);
        const kiss_hip_aln *dalns = st.up(alns, aln_count * sizeof(kiss_hip_aln));
        kiss_hip_pair *dpairs = st.room<kiss_hip_pair>(true, (Q / 2) * sizeof(kiss_hip_pair));
        if (st.rc) return st.rc;
        kiss_hip_pair_report r{};
        const int rc = kiss_hip_fmi_pair_dev(ctx, dhits, dhidx, Q, dalns, aln_count, params, dpairs, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(pairs, dpairs, (Q / 2) * sizeof(kiss_hip_pair));
        return st.rc;
    });
}

} // extern "C"
