// fm_select.hip -- FM-index: the alignments of a read turned into its mappings (kiss_hip_fmi_select_*).
//
// The reference has no such function; the definition is in include/kiss_hip.h and restated in tests/fm_select_model.py.  The
// input is what kiss_hip_fmi_align_dev wrote plus the read lengths and, optionally, the record starts of the text.  No index,
// no text and no read is looked at.
//
//   head  : one kernel checks chain_index, read_index and bounds and fetches the two ends of chain_index; the host looks at
//           them once (C sizes every grid below).
//   key   : ONE LANE PER ALIGNMENT finds its virtual read by search in chain_index and its record by search in bounds, decides
//           whether it is a candidate and writes the sort key (read, ~score) -- a non-candidate gets the score 0, which no
//           candidate has, so it sorts behind all candidates of its read.
//   sort  : the library's stable LSD radix sort over ALL alignments of the call (form A of the issue); stability gives the
//           order by a on equal scores.  A read's stretch of the sorted array is where its alignments were.
//   walk  : ONE WAVE PER READ goes through its candidates in order.  The kept hits live in the lanes, 64 at a time: the chunk
//           that is being filled in registers, the full chunks before it in scratch (written once with plain stores, the
//           stores awaited, then read with loads that bypass the L1: the same wave wrote them).  One candidate is tested
//           against a chunk by two ballots: text overlap on its strand (redundant), read overlap with a head (the lowest set
//           bit of the first chunk that has one is the head it belongs to).  c * ceil(|K| / 64) wave steps per read.
//   emit  : the u64 scan of the hit counts, ONE look at the total from the host (the capacity check: the caller's arrays are
//           untouched before it), one lane per sorted slot writes its hit with its mapq, one lane per read hit_index.
#include "fm_internal.hpp"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr uint32_t SL_NONE = 0xFFFFFFFFu;

// control block of a call (u64 words)
enum { SL_BAD = 0, SL_C0 = 1, SL_C1 = 2, SL_CAND = 3, SL_SPAN = 4, SL_RED = 5, SL_HEADS = 6, SL_MAPPED = 7, SL_MAXC = 8, SL_CTL_WORDS = 12 };

struct SelectP {
    uint32_t min_score, overlap, mapq_coef, mapq_max, max_hits;
};

// the kept hits of the call, one entry per sorted slot (a read keeps no more hits than it has alignments)
struct Kept {
    uint32_t *rb, *re, *tb, *te, *fl, *aln, *score, *sub, *nsec, *head, *ref;
};

// one kept hit in registers
struct KeptRow {
    uint32_t rb, re, tb, te, fl, aln, score, sub, nsec, head, ref;
};
// (eleven arrays: no two of these stores are neighbours)
__device__ __forceinline__ void sl_put(const Kept &K, uint64_t at, const KeptRow &k)
{
    K.rb[at] = k.rb;
    K.re[at] = k.re;
    K.tb[at] = k.tb;
    K.te[at] = k.te;
    K.fl[at] = k.fl;
    K.aln[at] = k.aln;
    K.score[at] = k.score;
    K.sub[at] = k.sub;
    K.nsec[at] = k.nsec;
    K.head[at] = k.head;
    K.ref[at] = k.ref;
}

// X and Y overlap by more than the share; a length below 0 counts as 0
__host__ __device__ inline bool sl_over(long long x0, long long x1, long long y0, long long y1, uint32_t share)
{
    const long long lo = x0 > y0 ? x0 : y0, hi = x1 < y1 ? x1 : y1;
    const long long ov = hi > lo ? hi - lo : 0;
    long long lx = x1 - x0, ly = y1 - y0;
    lx = lx > 0 ? lx : 0;
    ly = ly > 0 ? ly : 0;
    const long long mn = lx < ly ? lx : ly;
    return (unsigned long long)ov * 256ull > (unsigned long long)share * (unsigned long long)mn;
}

// Every load of this file starts at a multiple of its own size.  Neighbouring fields of a record, and
// neighbouring entries of an index, are fetched through these two: a relaxed load of wavefront scope is an ordinary
// global_load_dword / _dwordx2, and the compiler does not merge it with its neighbours into a 16-byte load at an address that
// is only 4- or 8-byte aligned (alns + 48 a + 8, index + 8 v).  sl_st32: the same for the fields of a hit.
__device__ __forceinline__ uint32_t sl_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t sl_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void sl_st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// the last v with index[v] <= x (index[0] <= x)
__device__ __forceinline__ uint64_t sl_last_le(const uint64_t *__restrict__ index, uint64_t count, uint64_t x)
{
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sl_ld64(index + mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a chain_index that decreases, a read_index that does not ascend, bounds that do not start at 0 or do not ascend; the two
// ends of chain_index
__global__ __launch_bounds__(SL_THREADS) void k_select_head(const uint64_t *__restrict__ chain_index, uint64_t V,
                                                           const uint64_t *__restrict__ read_index, uint64_t Q,
                                                           const uint64_t *__restrict__ bounds, uint64_t R,
                                                           unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (g == 0) {
        ctl[SL_C0] = sl_ld64(chain_index);
        ctl[SL_C1] = sl_ld64(chain_index + V);
    }
    bool bad = g < V && sl_ld64(chain_index + g + 1) < sl_ld64(chain_index + g);
    if (g < Q && sl_ld64(read_index + g + 1) <= sl_ld64(read_index + g)) bad = true; // (a zero-length read too)
    if (bounds) {
        if (g == 0 && sl_ld64(bounds) != 0) bad = true;
        if (g < R && sl_ld64(bounds + g + 1) <= sl_ld64(bounds + g)) bad = true;
    }
    if (__ballot(bad) && lane_id() == 0) ctl[SL_BAD] = 1;
}

// one lane per alignment a: candidate or not, its record of the text, its sort key
__global__ __launch_bounds__(SL_THREADS) void k_select_key(const kiss_hip_aln *__restrict__ alns, const uint64_t *__restrict__ chain_index,
                                                          uint64_t V, uint64_t c0, uint64_t C, int both,
                                                          const uint64_t *__restrict__ bounds, uint64_t R, uint32_t min_score,
                                                          int key_shift, uint64_t *__restrict__ keys, uint32_t *__restrict__ pos,
                                                          uint32_t *__restrict__ refs, unsigned long long *__restrict__ ctl)
{
    const uint64_t a = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x;
    bool cand = false, span = false;
    if (a < C) {
        const uint64_t v = sl_last_le(chain_index, V, c0 + a);
        const uint64_t q = both ? v >> 1 : v;
        const uint32_t score = sl_ld32(&alns[a].score), flags = sl_ld32(&alns[a].flags);
        uint32_t ref = 0;
        cand = flags == 0 && score >= (min_score > 1u ? min_score : 1u);
        if (cand && bounds) {
            const uint64_t tbeg = sl_ld32(&alns[a].tbeg), tend = sl_ld32(&alns[a].tend);
            const uint64_t rho = sl_last_le(bounds, R + 1, tbeg);
            span = rho >= R || tend > sl_ld64(bounds + rho + 1);
            ref = span ? 0u : (uint32_t)rho;
            cand = !span;
        }
        keys[a] = ((q << 32) | (uint64_t)(uint32_t)~(cand ? score : 0u)) << key_shift;
        pos[a] = (uint32_t)a;
        refs[a] = ref;
    }
    const unsigned long long nc = (unsigned long long)__popcll(__ballot(cand)), ns = (unsigned long long)__popcll(__ballot(span));
    if (lane_id() == 0) {
        if (nc) atomicAdd(&ctl[SL_CAND], nc);
        if (ns) atomicAdd(&ctl[SL_SPAN], ns);
    }
}

// a word that this wave stored earlier in the kernel: the store has been awaited (sl_stores_done), the load bypasses the L1
__device__ __forceinline__ uint32_t sl_reload(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sl_stores_done()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One wave per read.  nkept[q] = the hits of read q that will be written (after the cap); entry Q closes the array for the scan.
__global__ __launch_bounds__(SL_THREADS) void k_select_walk(const kiss_hip_aln *__restrict__ alns, const uint64_t *__restrict__ chain_index,
                                                           uint64_t c0, const uint64_t *__restrict__ read_index, uint64_t Q, int both,
                                                           const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos,
                                                           const uint32_t *__restrict__ refs, int key_shift, SelectP P, Kept K,
                                                           uint64_t *__restrict__ nkept, unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = lane_id();
    const uint64_t q = (uint64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6);
    if (q > Q) return;
    if (q == Q) {
        if (lane == 0) nkept[Q] = 0;
        return;
    }
    const uint64_t v0 = both ? 2 * q : q;
    const uint64_t s0 = sl_ld64(chain_index + v0) - c0, s1 = sl_ld64(chain_index + (both ? v0 + 2 : v0 + 1)) - c0;
    const uint64_t mid = both ? sl_ld64(chain_index + v0 + 1) - c0 : s1; // alignments from here on are on the reverse strand
    const long long L = (long long)(sl_ld64(read_index + q + 1) - sl_ld64(read_index + q));
    const uint32_t cap = P.max_hits ? P.max_hits : SL_NONE;

    // the chunk that is being filled: lane l holds hit 64 * (nK / 64) + l
    KeptRow kr{};
    uint32_t nK = 0, ncand = 0, nred = 0, nheads = 0, nheads_cap = 0;

    for (uint64_t base = s0; base < s1; base += 64) {
        const uint64_t s = base + lane;
        uint32_t c_score = 0, c_a = 0;
        if (s < s1) {
            c_score = ~(uint32_t)(sl_ld64(keys + s) >> key_shift); // 0: not a candidate, and none after it
            c_a = pos[s];
        }
        uint32_t c_rb = 0, c_re = 0, c_tb = 0, c_te = 0, c_ref = 0;
        if (c_score) {
            c_rb = sl_ld32(&alns[c_a].rbeg); // (four dword loads: alns + 48 a + 8 is no 16-byte address)
            c_re = sl_ld32(&alns[c_a].rend);
            c_tb = sl_ld32(&alns[c_a].tbeg);
            c_te = sl_ld32(&alns[c_a].tend);
            c_ref = refs[c_a];
        }
        const uint32_t n = (uint32_t)__popcll(__ballot(c_score != 0)); // (a prefix of the lanes)
        ncand += n;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t x_score = __shfl(c_score, j, 64), x_a = __shfl(c_a, j, 64), x_rb = __shfl(c_rb, j, 64),
                           x_re = __shfl(c_re, j, 64), x_tb = __shfl(c_tb, j, 64), x_te = __shfl(c_te, j, 64),
                           x_ref = __shfl(c_ref, j, 64);
            const uint32_t x_rev = (uint64_t)x_a >= mid ? 1u : 0u;
            const long long x_r0 = x_rev ? L - (long long)x_re : (long long)x_rb, x_r1 = x_rev ? L - (long long)x_rb : (long long)x_re;
            const uint32_t cur = nK >> 6, fill = nK & 63u;
            bool red = false;
            uint32_t g = SL_NONE;
            for (uint32_t k = 0; k <= cur; k++) {
                uint32_t y_rb, y_re, y_tb, y_te, y_fl;
                bool have;
                if (k < cur) {
                    const uint64_t at = s0 + 64ull * k + lane;
                    y_rb = sl_reload(K.rb + at);
                    y_re = sl_reload(K.re + at);
                    y_tb = sl_reload(K.tb + at);
                    y_te = sl_reload(K.te + at);
                    y_fl = sl_reload(K.fl + at);
                    have = true;
                } else {
                    y_rb = kr.rb;
                    y_re = kr.re;
                    y_tb = kr.tb;
                    y_te = kr.te;
                    y_fl = kr.fl;
                    have = lane < fill;
                }
                const uint32_t y_rev = y_fl & KISS_HIP_HIT_REVERSE;
                const bool t_over = have && y_rev == x_rev && sl_over((long long)x_tb, (long long)x_te, (long long)y_tb, (long long)y_te, P.overlap);
                if (__ballot(t_over)) {
                    red = true;
                    break;
                }
                const long long y_r0 = y_rev ? L - (long long)y_re : (long long)y_rb, y_r1 = y_rev ? L - (long long)y_rb : (long long)y_re;
                const bool r_over = have && !(y_fl & KISS_HIP_HIT_SECONDARY) && sl_over(x_r0, x_r1, y_r0, y_r1, P.overlap);
                const unsigned long long hb = __ballot(r_over);
                if (g == SL_NONE && hb) g = 64u * k + (uint32_t)__builtin_ctzll(hb);
            }
            if (red) {
                nred++;
                continue;
            }
            const uint32_t h = nK;
            const bool is_head = g == SL_NONE;
            if (lane == fill) {
                kr.rb = x_rb;
                kr.re = x_re;
                kr.tb = x_tb;
                kr.te = x_te;
                kr.fl = x_rev | (is_head ? (nheads ? (uint32_t)KISS_HIP_HIT_SUPPLEMENTARY : 0u) : (uint32_t)KISS_HIP_HIT_SECONDARY);
                kr.aln = x_a;
                kr.score = x_score;
                kr.sub = 0;
                kr.nsec = 0;
                kr.head = is_head ? h : g;
                kr.ref = x_ref;
            }
            if (is_head) {
                nheads++;
                if (h < cap) nheads_cap++;
            } else if ((g >> 6) == cur) {
                if (lane == (g & 63u)) {
                    kr.nsec++;
                    kr.sub = kr.sub > x_score ? kr.sub : x_score;
                }
            } else if (lane == 0) { // the head is in a chunk that was stored: its store has been awaited
                atomicAdd(K.nsec + s0 + g, 1u);
                atomicMax(K.sub + s0 + g, x_score);
            }
            nK++;
            if ((nK & 63u) == 0) { // the chunk is full: all 64 lanes store theirs (s0 + nK <= s1: no more kept than candidates)
                const uint64_t at = s0 + (nK - 64u) + lane;
                sl_put(K, at, kr);
                sl_stores_done();
            }
        }
        if (n < 64) break;
    }
    if (lane < (nK & 63u)) { // what is left of the last chunk
        const uint64_t at = s0 + (nK & ~63u) + lane;
        sl_put(K, at, kr);
    }
    if (lane == 0) {
        nkept[q] = nK < cap ? nK : cap;
        if (nred) atomicAdd(&ctl[SL_RED], (unsigned long long)nred);
        if (nheads_cap) atomicAdd(&ctl[SL_HEADS], (unsigned long long)nheads_cap);
        if (nK) atomicAdd(&ctl[SL_MAPPED], 1ull);
        if (ncand) atomicMax(&ctl[SL_MAXC], (unsigned long long)ncand);
    }
}

// one lane per sorted slot: the hit it holds, if its read writes that many, with its mapq; lanes 0 .. Q write hit_index
__global__ __launch_bounds__(SL_THREADS) void k_select_emit(const uint64_t *__restrict__ chain_index, uint64_t V, uint64_t c0, uint64_t C,
                                                           uint64_t Q, int both, const uint64_t *__restrict__ hit_off, SelectP P, Kept K,
                                                           kiss_hip_hit *__restrict__ hits, uint64_t *__restrict__ hit_index)
{
    const uint64_t s = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x;
    if (s <= Q) hit_index[s] = sl_ld64(hit_off + s);
    if (s >= C) return;
    const uint64_t v = sl_last_le(chain_index, V, c0 + s);
    const uint64_t q = both ? v >> 1 : v;
    const uint64_t h = s - (sl_ld64(chain_index + (both ? 2 * q : q)) - c0);
    const uint64_t first = sl_ld64(hit_off + q);
    if (h >= sl_ld64(hit_off + q + 1) - first) return;
    const uint32_t fl = K.fl[s], score = K.score[s];
    const bool is_head = !(fl & KISS_HIP_HIT_SECONDARY);
    const uint32_t nsec = is_head ? K.nsec[s] : 0u, sub = is_head && nsec ? K.sub[s] : 0u;
    uint32_t mapq = 0;
    if (is_head && score) { // (sub <= score: the candidates came in descending score)
        const unsigned long long m = (unsigned long long)P.mapq_coef * (unsigned long long)(score - sub) / (unsigned long long)score;
        mapq = m < (unsigned long long)P.mapq_max ? (uint32_t)m : P.mapq_max;
    }
    kiss_hip_hit *o = hits + first + h; // (eight dword stores: the caller's array need not be 16-byte aligned)
    sl_st32(&o->aln, K.aln[s]);
    sl_st32(&o->flags, fl);
    sl_st32(&o->mapq, mapq);
    sl_st32(&o->score, score);
    sl_st32(&o->sub, sub);
    sl_st32(&o->n_sec, nsec);
    sl_st32(&o->head, K.head[s]);
    sl_st32(&o->ref, K.ref[s]);
}

int select_steps(kiss_hip_ctx *ctx, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index, uint64_t Q, int both,
                 uint64_t V, const uint64_t *bounds, uint64_t R, const SelectP &P, kiss_hip_hit *hits, uint64_t *hit_index,
                 uint64_t hit_capacity, kiss_hip_select_report *rep, FmEvents &ev)
{
    if (V > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if ((Q + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    DevBuf slab;
    FmCtl<SL_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_SELECT_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    {
        uint64_t items = V + 1 > Q ? V + 1 : Q;
        if (bounds && R + 1 > items) items = R + 1;
        hipLaunchKernelGGL(k_select_head, dim3(fm_grid(items, SL_THREADS)), dim3(SL_THREADS), 0, ctx->stream, chain_index, V, read_index, Q, bounds, R,
                           d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(ctl.fetch_sync());
    if (h[SL_BAD]) return KISS_HIP_E_INVALID; // chain_index or read_index decreases, a read of length 0, bounds out of order
    const uint64_t c0 = h[SL_C0], C = h[SL_C1] - c0;
    if (rep) rep->alignments = C;
    if (C > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (C == 0) {
        KTRY(kiss_zero_u32(ctx, hit_index, 2 * (Q + 1)));
        ev.mark(1);
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    // one call: its alignments are sorted in the ctx's LMS key arrays
    if (C > ctx->m_cap) return KISS_HIP_E_UNSUPPORTED;
    const int key_shift = (32 - fm_bits(Q)) & ~7; // the sort takes whole bytes from the top of the key

    // the per-alignment arrays of the call, one slab
    FmSlab lay;
    uint64_t o_kept[11];
    for (auto &o : o_kept) o = lay.carve(C * 4);
    const uint64_t o_refs = lay.carve(C * 4), o_nkept = lay.carve((Q + 1) * 8);
    KTRY(slab.take(ctx, FM_SLOT_SELECT_SLAB, lay.size));
    char *sb = (char *)slab.p;
    Kept K;
    uint32_t **kf[11] = {&K.rb, &K.re, &K.tb, &K.te, &K.fl, &K.aln, &K.score, &K.sub, &K.nsec, &K.head, &K.ref};
    for (int i = 0; i < 11; i++) *kf[i] = (uint32_t *)(sb + o_kept[i]);
    uint32_t *refs = (uint32_t *)(sb + o_refs);
    uint64_t *nkept = (uint64_t *)(sb + o_nkept);

    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_select_key, dim3(fm_grid(C, SL_THREADS)), dim3(SL_THREADS), 0, ctx->stream, alns, chain_index, V, c0, C, both, bounds, R,
                           P.min_score, key_shift, ctx->keyA, ctx->posA, refs, d_ctl);
        KCHECK(hipGetLastError());
    }
    RadixBufs rb = kiss_ctx_radix_bufs(ctx); // (the positions: a)
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, C, key_shift, 0, &res));
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_select_walk, dim3((unsigned)div_up(Q + 1, SL_WAVES)), dim3(SL_THREADS), 0, ctx->stream, alns, chain_index, c0,
                           read_index, Q, both, (const uint64_t *)rb.key[res], (const uint32_t *)rb.pos[res], (const uint32_t *)refs,
                           key_shift, P, K, nkept, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KTRY(kiss_scan_u64(ctx, nkept, nkept, Q + 1));
    uint64_t total = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total, nkept + Q, 8, hipMemcpyDeviceToHost, ctx->stream));
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    if (rep) {
        rep->candidates = h[SL_CAND];
        rep->spanning = h[SL_SPAN];
        rep->redundant = h[SL_RED];
        rep->hits = total;
        rep->heads = h[SL_HEADS];
        rep->mapped = h[SL_MAPPED];
        rep->max_candidates = (uint32_t)h[SL_MAXC];
        rep->ms_sort = ev.ms(0, 1);
        rep->ms_walk = ev.ms(1, 2);
    }
    // (the totals are in the report: the caller's second call)
    if (hit_capacity < total) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_select_emit, dim3(fm_grid(C > Q + 1 ? C : Q + 1, SL_THREADS)), dim3(SL_THREADS), 0, ctx->stream, chain_index, V, c0, C, Q,
                           both, (const uint64_t *)nkept, P, K, hits, hit_index);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) rep->ms_emit = ev.ms(2, 3); // the scan, one look at the totals from the host, the records
    return KISS_HIP_OK;
}

int select_args_check(const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index, const uint64_t *bounds, uint64_t R,
                      const kiss_hip_select_params *params, const kiss_hip_hit *hits, const uint64_t *hit_index)
{
    if (!alns || !chain_index || !read_index || !params || !hits || !hit_index) return KISS_HIP_E_INVALID;
    if (bounds && (R == 0 || R > 0xFFFFFFFFull)) return KISS_HIP_E_INVALID;
    if (params->overlap > 256u || params->mapq_coef > 65535u || params->mapq_max > 255u) return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_select_dev(kiss_hip_ctx *ctx, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index,
                            uint64_t Q, int both_strands, const uint64_t *bounds, uint64_t R, const kiss_hip_select_params *params,
                            kiss_hip_hit *hits, uint64_t *hit_index, uint64_t hit_capacity, kiss_hip_select_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (report) {
        *report = kiss_hip_select_report{};
        report->Q = Q;
        report->V = V;
    }
    KTRY(select_args_check(alns, chain_index, read_index, bounds, R, params, hits, hit_index));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) { // hit_index[0] = 0
        KTRY(kiss_zero_u32(ctx, hit_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    SelectP P;
    P.min_score = params->min_score;
    P.overlap = params->overlap;
    P.mapq_coef = params->mapq_coef;
    P.mapq_max = params->mapq_max;
    P.max_hits = params->max_hits;
    FmEvents ev(ctx, report != nullptr);
    const int rc = select_steps(ctx, alns, chain_index, read_index, Q, both_strands ? 1 : 0, V, bounds, R, P, hits, hit_index, hit_capacity,
                                report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_select_host(const kiss_hip_aln *alns, const uint64_t *chain_index, const uint64_t *read_index, uint64_t Q,
                             int both_strands, const uint64_t *bounds, uint64_t R, const kiss_hip_select_params *params,
                             kiss_hip_hit *hits, uint64_t *hit_index, uint64_t hit_capacity, kiss_hip_select_report *report, int device)
{
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (report) {
        *report = kiss_hip_select_report{};
        report->Q = Q;
        report->V = V;
    }
    KTRY(select_args_check(alns, chain_index, read_index, bounds, R, params, hits, hit_index));
    if (V > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (!fm_index_ascending(read_index, Q, true) || !fm_index_ascending(chain_index, V, false)) return KISS_HIP_E_INVALID;
    const uint64_t C = chain_index[V] - chain_index[0]; // (alns is indexed from 0, as the align call writes it)
    if (report) report->alignments = C;
    if (C > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    // the alignments of a call are sorted in the ctx's LMS arrays and the reads scanned in its scratch
    return kiss_one_shot_cached(device, fm_host_max_n(0, C + 1, V + 1), [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t hcap = hit_capacity < C ? hit_capacity : C; // (no more hits than alignments)
        FmStage st(ctx);
        const kiss_hip_aln *dalns = st.up(alns, C * sizeof(kiss_hip_aln));
        const uint64_t *dcidx = st.up(chain_index, (V + 1) * 8);
        const uint64_t *dridx = st.up(read_index, (Q + 1) * 8);
        const uint64_t *dbounds = st.up(bounds, (R + 1) * 8);
        kiss_hip_hit *dhits = st.room<kiss_hip_hit>(true, hcap * sizeof(kiss_hip_hit));
        uint64_t *dhidx = st.room<uint64_t>(true, (Q + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_select_report r{};
        const int rc = kiss_hip_fmi_select_dev(ctx, dalns, dcidx, dridx, Q, both_strands ? 1 : 0, dbounds, R, params, dhits, dhidx, hcap, &r,
                                               nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(hit_index, dhidx, (Q + 1) * 8);
        st.down(hits, dhits, r.hits * sizeof(kiss_hip_hit));
        return st.rc;
    });
}

} // extern "C"
