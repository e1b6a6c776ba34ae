// fm_chain.hip -- FM-index: the seeds of a read chained into candidate loci (kiss_hip_fmi_chain_*).
//
// The reference has no such function; the definition is in include/kiss_hip.h and restated in tests/fm_chain_model.py.  The
// input is what kiss_hip_fmi_seeds_dev wrote: an anchor (r, t, l) per position of every located seed, slot = its index in
// `positions`.  No index and no text are read.
//
//   expand : ONE LANE PER SLOT finds its seed by search in pos_index and its virtual read by search in seed_index and writes
//            the sort key (v << tbits | t) with the slot as payload; the library's stable LSD radix sort in the ctx's LMS key
//            arrays (they bound the anchors of one call) over the bits that V and the largest t need.  Stability gives the
//            (t, slot) order.  A gather then lays the anchors out in that order, 16 bytes each.
//   dp     : ONE WAVE PER VIRTUAL READ.  Lane k keeps (r, t, f, root, depth) of anchor i - 1 - k in registers; a step
//            scores all 64 predecessors at once, takes the wave's largest score, picks the nearest lane that has it by
//            ballot, and shifts the ring by one lane.  No LDS and no global re-reads for max_lookback <= 64; a longer or
//            unbounded lookback goes on over earlier chunks of 64 from memory, nearest first, and stops at the first chunk
//            that lies wholly beyond max_gap (t ascends).  The results of 64 anchors are stored at once, one per lane.
//   emit   : the largest f of a tree by atomic max at its root, the smallest anchor that has it by atomic min; one packed
//            u64 scan over the anchors gives the chain number of every reported root and the offset of its anchors; the
//            host looks at the totals once; one lane per chain writes the record and walks pred back from the end.
#include "fm_internal.hpp"

#include <climits>
#include <vector>

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_WAVES = CH_THREADS / 64;

// control block of a call (u64 words)
enum { CH_BAD = 0, CH_S0 = 1, CH_S1 = 2, CH_P0 = 3, CH_P1 = 4, CH_MAXT = 5, CH_LEN0 = 6, CH_PAIRS = 7, CH_MAXA = 8, CH_BEST = 9,
       CH_CTL_WORDS = 12 };

struct ChainP {
    uint32_t max_gap, band, gap_cost, look, min_score;
};

// a seed_index that decreases; its two ends for the host
__global__ __launch_bounds__(CH_THREADS) void k_chain_head(const uint64_t *__restrict__ seed_index, uint64_t V,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint64_t v = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (v == 0) {
        ctl[CH_S0] = seed_index[0];
        ctl[CH_S1] = seed_index[V];
    }
    if (v < V && seed_index[v + 1] < seed_index[v]) ctl[CH_BAD] = 1;
}

// a pos_index that decreases over the seeds [s0, s1); its two ends and the largest position between them (grid-stride: the
// host does not know the number of positions yet)
__global__ __launch_bounds__(CH_THREADS) void k_chain_input(const uint64_t *__restrict__ pos_index, uint64_t s0, uint64_t s1,
                                                           const uint32_t *__restrict__ positions,
                                                           unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * CH_THREADS;
    const uint64_t p0 = pos_index[s0], p1 = pos_index[s1];
    if (g == 0) {
        ctl[CH_P0] = p0;
        ctl[CH_P1] = p1;
    }
    bool bad = p1 < p0;
    for (uint64_t s = s0 + g; s < s1; s += stride)
        if (pos_index[s + 1] < pos_index[s]) bad = true;
    uint32_t mx = 0;
    if (p1 >= p0)
        for (uint64_t h = p0 + g; h < p1; h += stride) {
            const uint32_t t = positions[h];
            mx = t > mx ? t : mx;
        }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = __shfl_xor(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if (__ballot(bad) && lane_id() == 0) ctl[CH_BAD] = 1;
    if (mx && lane_id() == 0) atomicMax(&ctl[CH_MAXT], (unsigned long long)mx);
}

// vstart[v] = the first anchor of virtual read v in the sorted order (v-major, and the anchors of a v are contiguous in
// slots); vstart[V] = the total
__global__ __launch_bounds__(CH_THREADS) void k_chain_vstart(const uint64_t *__restrict__ seed_index, uint64_t V,
                                                            const uint64_t *__restrict__ pos_index, uint64_t p0,
                                                            uint32_t *__restrict__ vstart)
{
    const uint64_t v = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (v <= V) vstart[v] = (uint32_t)(pos_index[seed_index[v]] - p0);
}

// one lane per slot p0 + h: its seed (the last s in [s0, s1) with pos_index[s] <= slot: seeds over max_occ own empty
// segments), its virtual read (the last v with seed_index[v] <= s: reads without seeds own empty segments), the key
__global__ __launch_bounds__(CH_THREADS) void k_chain_expand(const kiss_hip_fmi_seed *__restrict__ seeds,
                                                            const uint64_t *__restrict__ seed_index, uint64_t V, uint64_t s0,
                                                            uint64_t s1, const uint32_t *__restrict__ positions,
                                                            const uint64_t *__restrict__ pos_index, uint64_t p0, uint64_t total,
                                                            int tbits, int key_shift, uint64_t *__restrict__ keys,
                                                            uint32_t *__restrict__ payload, uint32_t *__restrict__ seed_of,
                                                            unsigned long long *__restrict__ ctl)
{
    const uint64_t h = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    bool len0 = false;
    if (h < total) {
        const uint64_t slot = p0 + h;
        uint64_t lo = s0, hi = s1;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pos_index[mid] <= slot) lo = mid;
            else hi = mid;
        }
        const uint64_t s = lo;
        lo = 0;
        hi = V;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (seed_index[mid] <= s) lo = mid;
            else hi = mid;
        }
        len0 = seeds[s].len == 0;
        keys[h] = ((lo << tbits) | (uint64_t)positions[slot]) << key_shift;
        payload[h] = (uint32_t)h;
        seed_of[h] = (uint32_t)(s - s0);
    }
    if (__ballot(len0) && lane_id() == 0) ctl[CH_LEN0] = 1;
}

// the anchors in sorted order: (r, t, l, slot - p0)
__global__ __launch_bounds__(CH_THREADS) void k_chain_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ payload,
                                                            const uint32_t *__restrict__ seed_of,
                                                            const kiss_hip_fmi_seed *__restrict__ seeds, uint64_t s0, uint64_t total,
                                                            int tbits, int key_shift, uint4 *__restrict__ anc)
{
    const uint64_t i = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint32_t h = payload[i];
    const kiss_hip_fmi_seed sd = seeds[s0 + seed_of[h]];
    const uint64_t t = (keys[i] >> key_shift) & ((1ull << tbits) - 1ull);
    anc[i] = make_uint4(sd.start, (uint32_t)t, sd.len, h);
}

__device__ __forceinline__ long long wave_max_i64(long long x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const long long o = __shfl_xor(x, s, 64);
        x = o > x ? o : x;
    }
    return x;
}

// may (rj, tj) precede (ri, ti), the order and the lookback aside; sc = the score through it
__device__ __forceinline__ bool chain_eval(const ChainP &P, uint32_t ri, uint32_t ti, uint32_t li, uint32_t rj, uint32_t tj,
                                           long long fj, long long &sc)
{
    const long long dt = (long long)ti - (long long)tj, dr = (long long)ri - (long long)rj;
    const long long d = dt - dr;
    const unsigned long long g = (unsigned long long)(d < 0 ? -d : d);
    long long gain = dr < dt ? dr : dt;
    gain = (long long)li < gain ? (long long)li : gain;
    sc = fj + gain - (long long)((g * P.gap_cost) >> 3); // g < 2^33, gap_cost < 2^16
    return dt > 0 && dr > 0 && dt <= (long long)P.max_gap && dr <= (long long)P.max_gap && g <= P.band;
}

// One wave per virtual read.  f is signed 64-bit throughout; pred1 = the predecessor's index + 1 in the sorted order (0:
// none), root an index in that order too.  bestf[root] (zeroed by the host; f >= 1) becomes the largest f of the tree.
__global__ __launch_bounds__(CH_THREADS) void k_chain_dp(const uint4 *__restrict__ anc, const uint32_t *__restrict__ vstart,
                                                        uint64_t V, ChainP P, long long *f, uint32_t *pred1, uint32_t *root,
                                                        uint32_t *depth, unsigned long long *__restrict__ bestf,
                                                        unsigned long long *__restrict__ ctl)
{
    const uint64_t v = (uint64_t)blockIdx.x * CH_WAVES + (threadIdx.x >> 6);
    if (v >= V) return;
    const uint32_t lane = lane_id();
    const uint32_t a0 = vstart[v], A = vstart[v + 1] - a0;
    if (A == 0) return;
    if (lane == 0) { // sum over i of min(i, lookback)
        const unsigned long long n = A, w = P.look;
        const unsigned long long pairs = (w == 0 || w >= n - 1) ? n * (n - 1) / 2 : w * (w + 1) / 2 + (n - 1 - w) * w;
        if (pairs) atomicAdd(&ctl[CH_PAIRS], pairs);
        atomicMax(&ctl[CH_MAXA], n);
    }
    const bool far = P.look == 0 || P.look > 64;
    // the ring: lane k holds anchor i - 1 - k
    uint32_t rr = 0, rt = 0, rroot = 0, rdepth = 0;
    long long rf = 0;
    for (uint32_t base = 0; base < A; base += 64) {
        const uint32_t n = A - base < 64u ? A - base : 64u;
        const uint4 mine = lane < n ? anc[a0 + base + lane] : make_uint4(0, 0, 0, 0);
        long long of = 0;
        uint32_t op = 0, oroot = 0, od = 0;
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t i = base + s;
            const uint32_t ri = __shfl(mine.x, (int)s, 64), ti = __shfl(mine.y, (int)s, 64), li = __shfl(mine.z, (int)s, 64);
            long long best = li; // (l_i, 0)
            uint32_t bj1 = 0;    // j + 1 within the read
            {
                long long sc;
                const bool ok = chain_eval(P, ri, ti, li, rr, rt, rf, sc) && lane < i && (P.look == 0 || lane < P.look);
                if (__ballot(ok)) {
                    const long long m = wave_max_i64(ok ? sc : LLONG_MIN);
                    if (m >= best) { // a predecessor that ties with starting afresh wins
                        const uint32_t k = (uint32_t)__ffsll((unsigned long long)__ballot(ok && sc == m)) - 1u; // the nearest
                        best = m;
                        bj1 = i - k;
                    }
                }
            }
            if (far && i > 64) { // the anchors before the ring, nearest chunk first
                const long long lo = (P.look && i > P.look) ? (long long)(i - P.look) : 0;
                for (long long top = (long long)i - 65; top >= lo; top -= 64) {
                    const long long j = top - (long long)lane;
                    const bool in = j >= lo;
                    const uint4 a = in ? anc[a0 + j] : make_uint4(0, 0, 0, 0);
                    const long long fj = in ? f[a0 + j] : 0;
                    if ((long long)ti - (long long)__shfl(a.y, 0, 64) > (long long)P.max_gap) break; // every earlier t is smaller still
                    long long sc;
                    const bool ok = chain_eval(P, ri, ti, li, a.x, a.y, fj, sc) && in;
                    if (__ballot(ok)) {
                        const long long m = wave_max_i64(ok ? sc : LLONG_MIN);
                        if (m > best || (m == best && bj1 == 0)) { // (a nearer predecessor keeps a tie)
                            const uint32_t k = (uint32_t)__ffsll((unsigned long long)__ballot(ok && sc == m)) - 1u;
                            best = m;
                            bj1 = (uint32_t)(top - k) + 1u;
                        }
                    }
                }
            }
            uint32_t ro = a0 + i, dp = 0;
            if (bj1) {
                const uint32_t k = i - bj1; // the predecessor's lane of the ring
                if (k < 64) {
                    ro = __shfl(rroot, (int)k, 64);
                    dp = __shfl(rdepth, (int)k, 64) + 1u;
                } else { // stored with an earlier chunk
                    ro = root[a0 + bj1 - 1];
                    dp = depth[a0 + bj1 - 1] + 1u;
                }
            }
            if (lane == s) {
                of = best;
                op = bj1 ? a0 + bj1 : 0u;
                oroot = ro;
                od = dp;
            }
            rr = __shfl_up(rr, 1, 64);
            rt = __shfl_up(rt, 1, 64);
            rf = __shfl_up(rf, 1, 64);
            rroot = __shfl_up(rroot, 1, 64);
            rdepth = __shfl_up(rdepth, 1, 64);
            if (lane == 0) {
                rr = ri;
                rt = ti;
                rf = best;
                rroot = ro;
                rdepth = dp;
            }
        }
        if (lane < n) {
            const uint32_t i = a0 + base + lane;
            f[i] = of;
            pred1[i] = op;
            root[i] = oroot;
            depth[i] = od;
            atomicMax(&bestf[oroot], (unsigned long long)of);
        }
        if (far) __threadfence(); // the next chunks read these from memory, other lanes than the ones that wrote them
    }
}

// the end of a tree: the smallest anchor that has the tree's largest f (bestend filled with 0xFFFFFFFF by the host)
__global__ __launch_bounds__(CH_THREADS) void k_chain_end(const long long *__restrict__ f, const uint32_t *__restrict__ root,
                                                         const unsigned long long *__restrict__ bestf, uint64_t total,
                                                         uint32_t *__restrict__ bestend)
{
    const uint64_t i = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= total) return;
    const uint32_t ro = root[i];
    if ((unsigned long long)f[i] == bestf[ro]) atomicMin(&bestend[ro], (uint32_t)i);
}

// packed[i] = (1 << 32 | anchors of the chain) for a root whose tree is reported, else 0; packed[total] = 0: the exclusive
// scan gives (chain number, first chain anchor) at every root and both totals at the end (neither sum reaches 2^32)
__global__ __launch_bounds__(CH_THREADS) void k_chain_flag(const uint32_t *__restrict__ root, const uint32_t *__restrict__ depth,
                                                          const unsigned long long *__restrict__ bestf,
                                                          const uint32_t *__restrict__ bestend, uint64_t total, uint32_t min_score,
                                                          uint64_t *__restrict__ packed, unsigned long long *__restrict__ ctl)
{
    const uint64_t i = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    unsigned long long best = 0;
    if (i < total) {
        const bool rep = root[i] == (uint32_t)i && bestf[i] >= (unsigned long long)min_score;
        packed[i] = rep ? ((1ull << 32) | (uint64_t)(depth[bestend[i]] + 1u)) : 0ull;
        if (rep) best = bestf[i];
    } else if (i == total) {
        packed[i] = 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(best, s, 64);
        best = o > best ? o : best;
    }
    if (best && lane_id() == 0) atomicMax(&ctl[CH_BEST], best);
}

// chain_index[v] = the chain number at the first anchor of v (V + 1 entries)
__global__ __launch_bounds__(CH_THREADS) void k_chain_index(const uint32_t *__restrict__ vstart, uint64_t V,
                                                           const uint64_t *__restrict__ scanned, uint64_t *__restrict__ chain_index)
{
    const uint64_t v = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (v <= V) chain_index[v] = scanned[vstart[v]] >> 32;
}

// one lane per anchor; the root of a reported tree writes the record and walks pred back from the end, anchor of depth d at
// anchor_index[c] + d.  Lane `total` closes anchor_index.
__global__ __launch_bounds__(CH_THREADS) void k_chain_emit(const uint4 *__restrict__ anc, const long long *__restrict__ f,
                                                          const uint32_t *__restrict__ pred1, const uint32_t *__restrict__ root,
                                                          const uint32_t *__restrict__ depth,
                                                          const unsigned long long *__restrict__ bestf,
                                                          const uint32_t *__restrict__ bestend, const uint64_t *__restrict__ scanned,
                                                          uint64_t total, uint32_t min_score, kiss_hip_chain *__restrict__ chains,
                                                          kiss_hip_chain_anchor *__restrict__ chain_anchors,
                                                          uint64_t *__restrict__ anchor_index)
{
    const uint64_t i = (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i > total) return;
    const uint64_t sc = scanned[i];
    const uint64_t c = sc >> 32, at = sc & 0xFFFFFFFFull;
    if (i == total) {
        if (anchor_index) anchor_index[c] = at;
        return;
    }
    if (root[i] != (uint32_t)i || bestf[i] < (unsigned long long)min_score) return;
    uint32_t e = bestend[i];
    const uint4 first = anc[i], last = anc[e];
    uint32_t d = depth[e];
    kiss_hip_chain out;
    out.score = (uint32_t)f[e];
    out.anchors = d + 1u;
    out.rbeg = first.x;
    out.rend = last.x + last.z;
    out.tbeg = first.y;
    out.tend = last.y + last.z;
    chains[c] = out;
    if (!chain_anchors) return;
    anchor_index[c] = at;
    for (;;) {
        const uint4 a = anc[e];
        kiss_hip_chain_anchor w;
        w.rstart = a.x;
        w.tpos = a.y;
        w.len = a.z;
        chain_anchors[at + d] = w;
        const uint32_t p = pred1[e];
        if (!p || !d) break; // (both at the root)
        e = p - 1u;
        d--;
    }
}

int chain_steps(kiss_hip_ctx *ctx, const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, uint64_t V, const uint32_t *positions,
                const uint64_t *pos_index, const ChainP &P, kiss_hip_chain *chains, uint64_t *chain_index, uint64_t chain_capacity,
                kiss_hip_chain_anchor *chain_anchors, uint64_t *anchor_index, uint64_t anchor_capacity, kiss_hip_chain_report *rep,
                FmEvents &ev)
{
    if (V > 0x7FFFFFFFull || (V + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    DevBuf slab, vs;
    FmCtl<CH_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_CHAIN_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_chain_head, dim3(fm_grid(V, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, seed_index, V, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[CH_BAD]) return KISS_HIP_E_INVALID; // seed_index decreases
    const uint64_t s0 = h[CH_S0], s1 = h[CH_S1], nseeds = s1 - s0;
    if (nseeds > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_chain_input, dim3(nseeds > (1u << 18) ? 1024u : 64u), dim3(CH_THREADS), 0, ctx->stream, pos_index, s0, s1,
                       positions, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[CH_BAD]) return KISS_HIP_E_INVALID; // pos_index decreases
    const uint64_t p0 = h[CH_P0], total = h[CH_P1] - p0;
    if (rep) rep->anchors = total;
    // one call: its anchors are sorted in the ctx's LMS key arrays and scanned in its scratch
    if (total > ctx->m_cap || total >= 0xFFFFFFFFull || (total + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    if (total == 0) { // no anchors: no chains
        KTRY(kiss_zero_u32(ctx, chain_index, 2 * (V + 1)));
        if (anchor_index) KTRY(kiss_zero_u32(ctx, anchor_index, 2));
        ev.mark(1);
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    const int vbits = fm_bits(V), tbits = fm_bits(h[CH_MAXT] + 1);
    const int key_shift = (64 - vbits - tbits) & ~7; // the sort takes whole bytes from the top of the key

    // the per-anchor arrays of the call, one slab
    FmSlab lay;
    const uint64_t o_anc = lay.carve(total * 16), o_f = lay.carve(total * 8), o_bestf = lay.carve(total * 8),
                   o_packed = lay.carve((total + 1) * 8), o_seedof = lay.carve(total * 4), o_pred = lay.carve(total * 4),
                   o_root = lay.carve(total * 4), o_depth = lay.carve(total * 4), o_bestend = lay.carve(total * 4);
    KTRY(slab.take(ctx, FM_SLOT_CHAIN_SLAB, lay.size));
    KTRY(vs.take(ctx, FM_SLOT_CHAIN_VSTART, (V + 1) * 4));
    char *sb = (char *)slab.p;
    uint4 *anc = (uint4 *)(sb + o_anc);
    long long *f = (long long *)(sb + o_f);
    unsigned long long *bestf = (unsigned long long *)(sb + o_bestf);
    uint64_t *packed = (uint64_t *)(sb + o_packed);
    uint32_t *seed_of = (uint32_t *)(sb + o_seedof), *pred1 = (uint32_t *)(sb + o_pred), *root = (uint32_t *)(sb + o_root),
             *depth = (uint32_t *)(sb + o_depth), *bestend = (uint32_t *)(sb + o_bestend), *vstart = (uint32_t *)vs.p;

    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_chain_vstart, dim3(fm_grid(V + 1, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, seed_index, V, pos_index, p0, vstart);
        hipLaunchKernelGGL(k_chain_expand, dim3(fm_grid(total, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, seeds, seed_index, V, s0, s1,
                           positions, pos_index, p0, total, tbits, key_shift, ctx->keyA, ctx->posA, seed_of, d_ctl);
        KCHECK(hipGetLastError());
    }
    RadixBufs rb = kiss_ctx_radix_bufs(ctx); // (the positions: the slots)
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, total, key_shift, 0, &res));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_chain_gather, dim3(fm_grid(total, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, (const uint64_t *)rb.key[res],
                           (const uint32_t *)rb.pos[res], (const uint32_t *)seed_of, seeds, s0, total, tbits, key_shift, anc);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_zero_u32(ctx, bestf, 2 * total));
    KTRY(kiss_fill_u32(ctx, bestend, 0xFFFFFFFFu, total));
    ev.mark(2);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_chain_dp, dim3((unsigned)div_up(V, CH_WAVES)), dim3(CH_THREADS), 0, ctx->stream, (const uint4 *)anc,
                           (const uint32_t *)vstart, V, P, f, pred1, root, depth, bestf, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_chain_end, dim3(fm_grid(total, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, (const long long *)f,
                           (const uint32_t *)root, (const unsigned long long *)bestf, total, bestend);
        hipLaunchKernelGGL(k_chain_flag, dim3(fm_grid(total + 1, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, (const uint32_t *)root,
                           (const uint32_t *)depth, (const unsigned long long *)bestf, (const uint32_t *)bestend, total, P.min_score,
                           packed, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, packed, packed, total + 1));
    uint64_t totals = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&totals, packed + total, 8, hipMemcpyDeviceToHost, ctx->stream));
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    if (h[CH_LEN0]) return KISS_HIP_E_INVALID; // a located seed of length 0
    const uint64_t nchains = totals >> 32, nanchors = totals & 0xFFFFFFFFull;
    if (rep) {
        rep->chains = nchains;
        rep->chain_anchors = nanchors;
        rep->dp_pairs = h[CH_PAIRS];
        rep->max_anchors = (uint32_t)h[CH_MAXA];
        rep->best_score = (uint32_t)h[CH_BEST];
        rep->ms_sort = ev.ms(1, 2);
        rep->ms_dp = ev.ms(2, 3);
    }
    // (the totals are in the report: the caller's second call)
    if (chain_capacity < nchains || (chain_anchors && anchor_capacity < nanchors)) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_chain_index, dim3(fm_grid(V + 1, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, (const uint32_t *)vstart, V,
                           (const uint64_t *)packed, chain_index);
        hipLaunchKernelGGL(k_chain_emit, dim3(fm_grid(total + 1, CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, (const uint4 *)anc,
                           (const long long *)f, (const uint32_t *)pred1, (const uint32_t *)root, (const uint32_t *)depth,
                           (const unsigned long long *)bestf, (const uint32_t *)bestend, (const uint64_t *)packed, total, P.min_score,
                           chains, chain_anchors, anchor_index);
        KCHECK(hipGetLastError());
    }
    ev.mark(4);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) rep->ms_emit = ev.ms(3, 4); // the tree ends, the scan, one look at the totals from the host, the records
    return KISS_HIP_OK;
}

int chain_args_check(const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, const uint32_t *positions, const uint64_t *pos_index,
                     const kiss_hip_chain_params *params, const kiss_hip_chain *chains, const uint64_t *chain_index,
                     const kiss_hip_chain_anchor *chain_anchors, const uint64_t *anchor_index, uint64_t anchor_capacity)
{
    const bool any = chain_anchors || anchor_index, all = chain_anchors && anchor_index;
    if (!seeds || !seed_index || !positions || !pos_index || !params || !chains || !chain_index || any != all ||
        (!any && anchor_capacity))
        return KISS_HIP_E_INVALID;
    if (params->max_gap > 0x7FFFFFFFu || params->band > 0x7FFFFFFFu || params->gap_cost > 65535u) return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_chain_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, uint64_t V,
                           const uint32_t *positions, const uint64_t *pos_index, const kiss_hip_chain_params *params,
                           kiss_hip_chain *chains, uint64_t *chain_index, uint64_t chain_capacity, kiss_hip_chain_anchor *chain_anchors,
                           uint64_t *anchor_index, uint64_t anchor_capacity, kiss_hip_chain_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_chain_report{};
        report->V = V;
    }
    KTRY(chain_args_check(seeds, seed_index, positions, pos_index, params, chains, chain_index, chain_anchors, anchor_index,
                          anchor_capacity));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (V == 0) { // chain_index[0] = anchor_index[0] = 0
        KTRY(kiss_zero_u32(ctx, chain_index, 2));
        if (anchor_index) KTRY(kiss_zero_u32(ctx, anchor_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    ChainP P;
    P.max_gap = params->max_gap;
    P.band = params->band;
    P.gap_cost = params->gap_cost;
    P.look = params->max_lookback;
    P.min_score = params->min_score;
    FmEvents ev(ctx, report != nullptr);
    const int rc = chain_steps(ctx, seeds, seed_index, V, positions, pos_index, P, chains, chain_index, chain_capacity, chain_anchors,
                               anchor_index, anchor_capacity, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_chain_host(const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, uint64_t V, const uint32_t *positions,
                            const uint64_t *pos_index, const kiss_hip_chain_params *params, kiss_hip_chain *chains,
                            uint64_t *chain_index, uint64_t chain_capacity, kiss_hip_chain_anchor *chain_anchors, uint64_t *anchor_index,
                            uint64_t anchor_capacity, kiss_hip_chain_report *report, int device)
{
    if (report) {
        *report = kiss_hip_chain_report{};
        report->V = V;
    }
    KTRY(chain_args_check(seeds, seed_index, positions, pos_index, params, chains, chain_index, chain_anchors, anchor_index,
                          anchor_capacity));
    if (!fm_index_ascending(seed_index, V, false)) return KISS_HIP_E_INVALID;
    const uint64_t nseeds = seed_index[V]; // (the arrays are uploaded from their first entry)
    if (!fm_index_ascending(pos_index, nseeds, false)) return KISS_HIP_E_INVALID;
    const uint64_t npos = pos_index[nseeds];
    // the anchors of a call are sorted in the ctx's LMS arrays and scanned in its scratch
    return kiss_one_shot_cached(device, fm_host_max_n(0, npos + 1, V + 1), [&](kiss_hip_ctx *ctx) -> int {
        const bool all = chain_anchors != nullptr;
        // (no more chains than anchors, no more chain anchors than anchors)
        const uint64_t ccap = chain_capacity < npos ? chain_capacity : npos, acap = anchor_capacity < npos ? anchor_capacity : npos;
        FmStage st(ctx);
        const kiss_hip_fmi_seed *dseeds = st.up(seeds, nseeds * 16);
        const uint64_t *dsidx = st.up(seed_index, (V + 1) * 8);
        const uint32_t *dpos = st.up(positions, npos * 4);
        const uint64_t *dpidx = st.up(pos_index, (nseeds + 1) * 8);
        kiss_hip_chain *dchains = st.room<kiss_hip_chain>(true, ccap * sizeof(kiss_hip_chain));
        uint64_t *dcidx = st.room<uint64_t>(true, (V + 1) * 8);
        kiss_hip_chain_anchor *danc = st.room<kiss_hip_chain_anchor>(all, acap * sizeof(kiss_hip_chain_anchor));
        uint64_t *daidx = st.room<uint64_t>(all, (ccap + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_chain_report r{};
        const int rc = kiss_hip_fmi_chain_dev(ctx, dseeds, dsidx, V, dpos, dpidx, params, dchains, dcidx, ccap, danc, daidx, all ? acap : 0,
                                              &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(chain_index, dcidx, (V + 1) * 8);
        st.down(chains, dchains, r.chains * sizeof(kiss_hip_chain));
        if (all) st.down(anchor_index, daidx, (r.chains + 1) * 8);
        if (all) st.down(chain_anchors, danc, r.chain_anchors * sizeof(kiss_hip_chain_anchor));
        return st.rc;
    });
}

} // extern "C"
