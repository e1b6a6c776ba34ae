// fm8.hip -- FM-index over a byte text (values 0..255): build, batched backward search over ragged patterns, locate
// (kiss_hip_fmi8_*).
//
// The reference has no such index (its -g commands are a TODO); ground truth is the text itself (tests/fm8_model.py).
//
//   layout  : the BWT as plain bytes, 256 rows to a block (one block = 256 bytes, 16-byte aligned by construction), and
//             cumulative counts SYMBOL-MAJOR, only for the sigma byte values that occur (dense codes in value order):
//             occ1[c][j] (u32) = occurrences of c before row 65536 j, occ2[c][j] (u16) = occurrences between the start of the
//             superblock and row 256 j.  rank(c, i) = occ1 + occ2 + the matches among the i % 256 bytes in front of row i in
//             its block (SWAR byte compare + popcount on aligned 16-byte loads).  The three addresses follow from (c, i)
//             alone: ONE level of dependent loads per LF pair.  The primary row stores 0 and is left out of every count.
//   search  : one lane per pattern (k_fm8_search<false>), or 16 lanes -- one DPP row -- per pattern, each lane one 16-byte
//             chunk of the block, the partial counts summed over the row (k_fm8_search<true>; the A-B of the hooks build,
//             KissOpts::fm8_group; DESIGN.md 4.7 has the numbers).  From the right, until the range is empty; a pattern byte
//             that does not occur in the text ends it at once.
//   locate  : counts -> exclusive scan = index; one lane per hit row finds its pattern by binary search, walks LF to a
//             sampled row (at most sa_intv - 1 steps, never from the primary row) and writes the sort key
//             (q << 32 | position); the library's radix sort in the ctx's LMS arrays gives ascending positions per pattern.
#include "fm_internal.hpp"
#include <cstring>

namespace {

constexpr int F8_THREADS = 256;
constexpr uint32_t F8_TILE = 32;  // blocks whose occ2 rows are staged in shared memory before they are written out
constexpr uint32_t F8_GROUP = 16; // lanes per pattern of the group form: one DPP row, one 16-byte chunk per lane

struct Fm8D {
    uint64_t N, nblk, nsb;
    uint32_t pri, sigma;
    const uint32_t *C;
    const uint8_t *map;
    const uint8_t *bwt;
    const uint32_t *occ1;
    const uint16_t *occ2;
    const uint32_t *sa;
    const uint64_t *b;
    const uint32_t *b_occ;
};

// control block of a call (u64 words)
enum { F8_HITS = 0, F8_LF = 1, F8_WALKFAIL = 2, F8_CHECKSUM = 3, F8_BAD = 4, F8_CTL_WORDS = 8 };

// 0x80 in every byte of x that is zero (exact: no carry leaves a byte)
__device__ __forceinline__ uint64_t f8_zero_bytes(uint64_t x)
{
    const uint64_t m = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & m) + m) | x | m);
}
// how many of the first `left` bytes of a 16-byte chunk equal the byte vv is made of (left <= 0: none, >= 16: all sixteen)
__device__ __forceinline__ uint32_t f8_count16(const uint4 &w, uint64_t vv, int left)
{
    uint64_t zl = f8_zero_bytes((((uint64_t)w.y << 32) | w.x) ^ vv), zh = f8_zero_bytes((((uint64_t)w.w << 32) | w.z) ^ vv);
    const int l0 = left < 0 ? 0 : (left > 8 ? 8 : left), l1 = left < 8 ? 0 : (left > 16 ? 8 : left - 8);
    zl = l0 >= 8 ? zl : (zl & ((1ull << (8 * l0)) - 1ull));
    zh = l1 >= 8 ? zh : (zh & ((1ull << (8 * l1)) - 1ull));
    return (uint32_t)__popcll(zl) + (uint32_t)__popcll(zh);
}
__device__ __forceinline__ const uint4 *f8_block(const Fm8D &f, uint64_t j)
{
    return reinterpret_cast<const uint4 *>(__builtin_assume_aligned(f.bwt + (j << 8), 16));
}
__device__ __forceinline__ uint32_t f8_base(const Fm8D &f, uint32_t c, uint64_t i)
{
    return f.occ1[(uint64_t)c * f.nsb + (i >> 16)] + (uint32_t)f.occ2[(uint64_t)c * f.nblk + (i >> 8)];
}
// the primary row holds the placeholder 0: not an occurrence of byte 0
__device__ __forceinline__ uint32_t f8_pass_pri(const Fm8D &f, uint32_t v, uint64_t i)
{
    return (v == 0 && (i & ~255ull) <= f.pri && f.pri < i) ? 1u : 0u;
}

// rank(c, i), i <= N, by one lane: the block is read 64 bytes at a time (four independent loads; a block is whole, so the
// chunks behind row i are inside the array and only masked out of the count)
__device__ __forceinline__ uint32_t f8_rank(const Fm8D &f, uint32_t c, uint32_t v, uint64_t i)
{
    const uint64_t vv = (uint64_t)v * 0x0101010101010101ull;
    const int r = (int)(i & 255u);
    const uint32_t base = f8_base(f, c, i);
    const uint4 *p = f8_block(f, i >> 8);
    uint32_t cnt = 0;
    for (int k = 0; 16 * k < r; k += 4) {
        const uint4 w0 = p[k], w1 = p[k + 1], w2 = p[k + 2], w3 = p[k + 3];
        cnt += f8_count16(w0, vv, r - 16 * k) + f8_count16(w1, vv, r - 16 * k - 16) + f8_count16(w2, vv, r - 16 * k - 32) +
               f8_count16(w3, vv, r - 16 * k - 48);
    }
    return base + cnt - f8_pass_pri(f, v, i);
}
// both ends of a range (beg <= end <= N) for one byte: the loads are shared when they fall into the same block
__device__ __forceinline__ void f8_rank2(const Fm8D &f, uint32_t c, uint32_t v, uint64_t beg, uint64_t end, uint32_t &rb, uint32_t &re)
{
    if ((beg >> 8) != (end >> 8)) {
        rb = f8_rank(f, c, v, beg);
        re = f8_rank(f, c, v, end);
        return;
    }
    const uint64_t vv = (uint64_t)v * 0x0101010101010101ull;
    const int r0 = (int)(beg & 255u), r1 = (int)(end & 255u);
    const uint32_t base = f8_base(f, c, beg);
    const uint4 *p = f8_block(f, beg >> 8);
    uint32_t cb = 0, ce = 0;
    for (int k = 0; 16 * k < r1; k += 4) {
        const uint4 w0 = p[k], w1 = p[k + 1], w2 = p[k + 2], w3 = p[k + 3];
        ce += f8_count16(w0, vv, r1 - 16 * k) + f8_count16(w1, vv, r1 - 16 * k - 16) + f8_count16(w2, vv, r1 - 16 * k - 32) +
              f8_count16(w3, vv, r1 - 16 * k - 48);
        cb += f8_count16(w0, vv, r0 - 16 * k) + f8_count16(w1, vv, r0 - 16 * k - 16) + f8_count16(w2, vv, r0 - 16 * k - 32) +
              f8_count16(w3, vv, r0 - 16 * k - 48);
    }
    rb = base + cb - f8_pass_pri(f, v, beg);
    re = base + ce - f8_pass_pri(f, v, end);
}

// sum over the 16 lanes of a DPP row, the result in every lane of the row (quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror)
__device__ __forceinline__ uint32_t f8_row_sum(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true);
    return x;
}
// the same pair by the 16 lanes of a row (all of them active, all with the same arguments): lane g counts chunk g of each block
__device__ __forceinline__ void f8_rank2_row(const Fm8D &f, uint32_t c, uint32_t v, uint64_t beg, uint64_t end, uint32_t g,
                                             uint32_t &rb, uint32_t &re)
{
    const uint64_t vv = (uint64_t)v * 0x0101010101010101ull;
    const int r0 = (int)(beg & 255u) - 16 * (int)g, r1 = (int)(end & 255u) - 16 * (int)g;
    const bool same = (beg >> 8) == (end >> 8);
    const uint32_t bb = f8_base(f, c, beg), be = same ? bb : f8_base(f, c, end);
    const uint4 wb = f8_block(f, beg >> 8)[g];
    const uint4 we = same ? wb : f8_block(f, end >> 8)[g];
    const uint32_t s = f8_row_sum(f8_count16(wb, vv, r0) | (f8_count16(we, vv, r1) << 16)); // (each sum <= 255)
    rb = bb + (s & 0xFFFFu) - f8_pass_pri(f, v, beg);
    re = be + (s >> 16) - f8_pass_pri(f, v, end);
}

// GROUP = false: one lane per pattern; true: F8_GROUP lanes per pattern.  counts (u64, may be null) feeds the scan of the locate.
template <bool GROUP>
__global__ __launch_bounds__(F8_THREADS) void k_fm8_search(Fm8D f, const uint8_t *__restrict__ pat,
                                                          const uint64_t *__restrict__ pidx, uint64_t Q,
                                                          uint32_t *__restrict__ beg_out, uint32_t *__restrict__ end_out,
                                                          uint64_t *__restrict__ counts, unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t sC[257];
    __shared__ uint8_t smap[256];
    const uint32_t tid = threadIdx.x;
    sC[tid] = f.C[tid];
    if (tid == 0) sC[256] = f.C[256];
    smap[tid] = f.map[tid];
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * F8_THREADS + tid;
    const uint64_t q = GROUP ? t / F8_GROUP : t;
    const uint32_t g = GROUP ? tid % F8_GROUP : 0u;
    const uint32_t N = (uint32_t)f.N;
    uint32_t beg = 0, end = 0;
    unsigned long long lf = 0, hits = 0, bad = 0;
    if (q < Q) {
        const uint64_t lo = pidx[q], hi = pidx[q + 1];
        if (hi <= lo) {
            bad = g == 0;
        } else {
            end = N;
            for (uint64_t p = hi; p > lo && beg < end; p--) {
                const uint32_t v = pat[p - 1];
                const uint32_t c = smap[v];
                if (sC[v + 1] == sC[v]) { // a byte the text does not hold (map says 0xFF, which is also a code at sigma = 256)
                    beg = end = 0;
                    break;
                }
                uint32_t rb, re;
                if (GROUP) f8_rank2_row(f, c, v, beg, end, g, rb, re);
                else f8_rank2(f, c, v, beg, end, rb, re);
                beg = sC[v] + rb;
                end = sC[v] + re;
                beg = beg < N ? beg : N;
                end = end < N ? end : N;
                lf++;
            }
            if (beg >= end) beg = end = 0;
        }
        if (g == 0) {
            beg_out[q] = beg;
            end_out[q] = end;
            if (counts) counts[q] = end - beg;
            hits = end - beg;
        } else {
            lf = 0;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lf += __shfl_xor(lf, s, 64);
        hits += __shfl_xor(hits, s, 64);
        bad += __shfl_xor(bad, s, 64);
    }
    if (lane_id() == 0) {
        if (lf) atomicAdd(&ctl[F8_LF], lf);
        if (hits) atomicAdd(&ctl[F8_HITS], hits);
        if (bad) atomicAdd(&ctl[F8_BAD], bad);
    }
}

// one lane per hit row: its pattern by binary search in index (Q + 1 entries), then LF to a sampled row.  A row that finds no
// sampled row inside the bound (an index that was not built from an exact suffix array) is counted and gets 0xFFFFFFFF.
__global__ __launch_bounds__(F8_THREADS) void k_fm8_locate(Fm8D f, uint32_t sa_intv, uint64_t sa_entries,
                                                          const uint32_t *__restrict__ beg_in,
                                                          const uint64_t *__restrict__ index, uint64_t Q, uint64_t total,
                                                          int key_shift, uint64_t *__restrict__ keys,
                                                          unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t sC[257];
    __shared__ uint8_t smap[256];
    sC[threadIdx.x] = f.C[threadIdx.x];
    if (threadIdx.x == 0) sC[256] = f.C[256];
    smap[threadIdx.x] = f.map[threadIdx.x];
    __syncthreads();
    const uint64_t h = (uint64_t)blockIdx.x * F8_THREADS + threadIdx.x;
    unsigned long long sum = 0;
    bool fail = false;
    if (h < total) {
        uint64_t lo = 0, hi = Q; // the last pattern with index[q] <= h (patterns without hits share an entry: the last one wins)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (index[mid] <= h) lo = mid;
            else hi = mid;
        }
        uint64_t row = (uint64_t)beg_in[lo] + (h - index[lo]);
        uint32_t position = 0xFFFFFFFFu;
        fail = true;
        for (uint32_t step = 0; step < sa_intv && row < f.N; step++) {
            const bool sampled = !f.b || ((f.b[row >> 6] >> (row & 63u)) & 1ull);
            if (sampled) {
                const uint64_t r = fm_b_rank(f.b, f.b_occ, row);
                if (r < sa_entries) {
                    position = f.sa[r] + step;
                    fail = false;
                }
                break;
            }
            if (row == f.pri || step + 1 == sa_intv) break;
            const uint32_t v = f.bwt[row];
            const uint32_t c = smap[v];
            if (sC[v + 1] == sC[v]) break; // (not a byte of the text: not this index's BWT)
            row = (uint64_t)sC[v] + f8_rank(f, c, v, row);
        }
        keys[h] = (((uint64_t)lo << 32) | position) << key_shift;
        if (!fail) sum = position;
    }
    const unsigned long long nf = (unsigned long long)__popcll(__ballot(fail));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if (lane_id() == 0) {
        if (sum) atomicAdd(&ctl[F8_CHECKSUM], sum);
        if (nf) atomicAdd(&ctl[F8_WALKFAIL], nf);
    }
}

__global__ __launch_bounds__(F8_THREADS) void k_fm8_unpack(const uint64_t *__restrict__ keys, uint64_t total, int key_shift,
                                                          uint32_t *__restrict__ positions)
{
    const uint64_t i = (uint64_t)blockIdx.x * F8_THREADS + threadIdx.x;
    if (i < total) positions[i] = (uint32_t)(keys[i] >> key_shift);
}

// ---- construction ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(F8_THREADS) void k_fm8_hist(const uint8_t *__restrict__ S, uint64_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * F8_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * F8_THREADS)
        atomicAdd(&h[S[i]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// One workgroup per superblock of 65536 rows, one thread per row of the block in hand: the BWT bytes, the primary row, the
// block's symbol histogram in shared memory, and from it -- thread c keeps the running count of code c -- the occ2 rows,
// staged F8_TILE blocks at a time so that every symbol writes a run of consecutive entries, and the superblock's totals.
__global__ __launch_bounds__(F8_THREADS) void k_fm8_bwt(const uint8_t *__restrict__ S, const uint32_t *__restrict__ SA, uint64_t N,
                                                       uint64_t nblk, uint64_t nsb, uint32_t sigma,
                                                       const uint8_t *__restrict__ map, uint8_t *__restrict__ bwt,
                                                       uint16_t *__restrict__ occ2, uint32_t *__restrict__ sbtot,
                                                       uint32_t *__restrict__ pri)
{
    __shared__ uint32_t hist[256];
    __shared__ uint16_t tile[256][F8_TILE];
    __shared__ uint8_t smap[256];
    const uint32_t t = threadIdx.x;
    const uint64_t sb = blockIdx.x, blk0 = sb * 256;
    smap[t] = map[t];
    hist[t] = 0;
    uint32_t run = 0;
    __syncthreads();
    const uint32_t nb = (uint32_t)(nblk - blk0 < 256 ? nblk - blk0 : 256);
    for (uint32_t k = 0; k < nb; k++) {
        const uint64_t i = (blk0 + k) * 256 + t;
        uint8_t byte = 0;
        if (i < N) {
            const uint32_t v = SA[i];
            if (v == 0) {
                *pri = (uint32_t)i;
            } else if (v < N) {
                byte = S[v - 1];
                const uint32_t c = smap[byte];
                if (c < sigma) atomicAdd(&hist[c], 1u);
            }
        }
        bwt[i] = byte; // (the rows >= N of the last block: 0)
        __syncthreads();
        tile[t][k % F8_TILE] = (uint16_t)run;
        run += hist[t];
        hist[t] = 0;
        __syncthreads();
        if (k % F8_TILE == F8_TILE - 1 || k == nb - 1) {
            const uint32_t k0 = k - k % F8_TILE, cnt = k % F8_TILE + 1;
            for (uint32_t e = t; e < sigma * cnt; e += F8_THREADS) {
                const uint32_t c = e / cnt, kk = e % cnt;
                occ2[(uint64_t)c * nblk + blk0 + k0 + kk] = tile[c][kk];
            }
            __syncthreads();
        }
    }
    if (t < sigma) sbtot[(uint64_t)t * nsb + sb] = run;
}

// occ1[c][j] = the scanned (symbol, superblock) matrix minus the total of the smaller symbols
__global__ __launch_bounds__(F8_THREADS) void k_fm8_occ1(const uint32_t *__restrict__ scanned, uint64_t nsb, uint64_t entries,
                                                        uint32_t *__restrict__ occ1)
{
    const uint64_t i = (uint64_t)blockIdx.x * F8_THREADS + threadIdx.x;
    if (i < entries) occ1[i] = scanned[i] - scanned[(i / nsb) * nsb];
}

// the census: C, map and sigma of a device text (synchronises)
int f8_census(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, uint32_t C[257], uint8_t map[256], uint32_t *sigma)
{
    DevBuf hist;
    KTRY(hist.alloc(ctx, 256 * 4));
    KTRY(kiss_zero_u32(ctx, hist.p, 256));
    if (n) {
        const uint64_t blocks = div_up(n, (uint64_t)F8_THREADS * 64);
        hipLaunchKernelGGL(k_fm8_hist, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(F8_THREADS), 0, ctx->stream, d_S, n,
                           (uint32_t *)hist.p);
        KCHECK(hipGetLastError());
    }
    uint32_t h[256];
    KCHECK(hipMemcpyAsync(h, hist.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    uint32_t sum = 1, s = 0;
    for (int v = 0; v < 256; v++) {
        C[v] = sum;
        sum += h[v];
        map[v] = h[v] ? (uint8_t)s++ : (uint8_t)0xFF;
    }
    C[256] = sum;
    *sigma = s;
    return KISS_HIP_OK;
}

int f8_build(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t sa_intv, uint32_t sigma_capacity,
             uint32_t *d_C, uint8_t *d_map, uint8_t *d_bwt, uint32_t *d_occ1, uint16_t *d_occ2, uint32_t *d_sa, uint64_t *d_b,
             uint32_t *d_b_occ, uint32_t *sigma_out, uint32_t *pri_out, void *stream)
{
    KTRY(fm_enter(ctx, stream));
    KTimer t(ctx, KISS_HIP_K_FM_BUILD, n + 1);
    uint32_t C[257], sigma = 0;
    uint8_t map[256];
    KTRY(f8_census(ctx, d_S, n, C, map, &sigma));
    *sigma_out = sigma;
    if (d_C) KCHECK(hipMemcpy(d_C, C, sizeof C, hipMemcpyHostToDevice));
    if (d_map) KCHECK(hipMemcpy(d_map, map, sizeof map, hipMemcpyHostToDevice));
    if (!d_bwt) return KISS_HIP_OK; // the census only
    if (sigma > sigma_capacity) return KISS_HIP_E_INVALID;
    const uint64_t N = n + 1, nblk = N / 256 + 1, nsb = N / 65536 + 1;
    const uint64_t entries = (uint64_t)sigma * nsb;
    if (entries / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    DevBuf sbtot, scanned, pri;
    KTRY(sbtot.alloc(ctx, (entries + 1) * 4));
    KTRY(scanned.alloc(ctx, (entries + 1) * 4));
    KTRY(pri.alloc(ctx, 4));
    KTRY(kiss_zero_u32(ctx, pri.p, 1));
    hipLaunchKernelGGL(k_fm8_bwt, dim3((unsigned)nsb), dim3(F8_THREADS), 0, ctx->stream, d_S, d_SA, N, nblk, nsb, sigma,
                       (const uint8_t *)d_map, d_bwt, d_occ2, (uint32_t *)sbtot.p, (uint32_t *)pri.p);
    KCHECK(hipGetLastError());
    if (entries) {
        KTRY(kiss_scan_u32(ctx, (const uint32_t *)sbtot.p, (uint32_t *)scanned.p, entries));
        hipLaunchKernelGGL(k_fm8_occ1, dim3((unsigned)div_up(entries, F8_THREADS)), dim3(F8_THREADS), 0, ctx->stream,
                           (const uint32_t *)scanned.p, nsb, entries, d_occ1);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_fm_sample_sa(ctx, d_SA, N, sa_intv, d_sa, d_b, d_b_occ));
    uint32_t h_pri = 0;
    KCHECK(hipMemcpyAsync(&h_pri, pri.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    *pri_out = h_pri;
    return KISS_HIP_OK;
}

int f8_query_steps(kiss_hip_ctx *ctx, const kiss_hip_fmi8_view *fmi, const uint8_t *patterns, const uint64_t *pat_index, uint64_t Q,
                   uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum, uint32_t *positions,
                   uint64_t *index, uint64_t capacity, kiss_hip_fmi8_report *rep, FmEvents &ev)
{
    const bool want = positions != nullptr;
    if (Q > 0x7FFFFFFFull || Q / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    kiss_opts_refresh(ctx);
    Fm8D f;
    f.N = fmi->n_sa;
    f.nblk = f.N / 256 + 1;
    f.nsb = f.N / 65536 + 1;
    f.pri = fmi->pri;
    f.sigma = fmi->sigma;
    f.C = fmi->C;
    f.map = fmi->map;
    f.bwt = fmi->bwt;
    f.occ1 = fmi->occ1;
    f.occ2 = fmi->occ2;
    f.sa = fmi->sa;
    f.b = fmi->sa_intv == 1 ? nullptr : fmi->b;
    f.b_occ = fmi->b_occ;
    const uint64_t sa_entries = (f.N + fmi->sa_intv - 1) / fmi->sa_intv;
    DevBuf counts;
    FmCtl<F8_CTL_WORDS> ctl;
    unsigned long long *const h = ctl.h;
    KTRY(ctl.take(ctx, FM_SLOT_FM8_CTL));
    if (want) KTRY(counts.take(ctx, FM_SLOT_FM8_COUNTS, (Q + 1) * 8));
    KTRY(ctl.zero());
    ev.mark(0);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, Q);
        if (ctx->opts.fm8_group)
            hipLaunchKernelGGL((k_fm8_search<true>), dim3((unsigned)div_up(Q * F8_GROUP, F8_THREADS)), dim3(F8_THREADS), 0, ctx->stream,
                               f, patterns, pat_index, Q, beg, end, (uint64_t *)counts.p, ctl.d);
        else
            hipLaunchKernelGGL((k_fm8_search<false>), dim3((unsigned)div_up(Q, F8_THREADS)), dim3(F8_THREADS), 0, ctx->stream, f,
                               patterns, pat_index, Q, beg, end, (uint64_t *)counts.p, ctl.d);
        KCHECK(hipGetLastError());
        ev.mark(1);
    }
    KTRY(ctl.fetch_sync());
    if (h[F8_BAD]) return KISS_HIP_E_INVALID; // a pattern of length zero, or pat_index decreases
    const uint64_t total = h[F8_HITS];
    if (hit_count_total) *hit_count_total = total;
    if (rep) {
        rep->hits = total;
        rep->lf_pairs = h[F8_LF];
        rep->ms_search = ev.ms(0, 1);
    }
    if (!want) return KISS_HIP_OK;
    if (capacity < total) return KISS_HIP_E_INVALID; // (the total is reported: the caller's second call)
    if (total > ctx->m_cap) return KISS_HIP_E_UNSUPPORTED; // the sort runs in the ctx's LMS key arrays
    KTRY(kiss_zero_u32(ctx, (uint8_t *)counts.p + Q * 8, 2));
    KTRY(kiss_scan_u64(ctx, (const uint64_t *)counts.p, index, Q + 1));
    if (!total) {
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    const int key_shift = (32 - fm_bits(Q, 32, 0)) & ~7; // the sort takes whole bytes from the top of the key
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        ev.mark(2);
        hipLaunchKernelGGL(k_fm8_locate, dim3((unsigned)div_up(total, F8_THREADS)), dim3(F8_THREADS), 0, ctx->stream, f,
                           fmi->sa_intv, sa_entries, (const uint32_t *)beg, (const uint64_t *)index, Q, total, key_shift, ctx->keyA,
                           ctl.d);
        KCHECK(hipGetLastError());
        ev.mark(3);
    }
    RadixBufs rb = kiss_ctx_radix_bufs(ctx); // (a payload nobody reads)
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, total, key_shift, 0, &res));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
        hipLaunchKernelGGL(k_fm8_unpack, dim3((unsigned)div_up(total, F8_THREADS)), dim3(F8_THREADS), 0, ctx->stream, rb.key[res],
                           total, key_shift, positions);
        KCHECK(hipGetLastError());
    }
    ev.mark(4);
    KTRY(ctl.fetch());
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    if (checksum) *checksum = h[F8_CHECKSUM];
    if (rep) {
        rep->walk_failures = h[F8_WALKFAIL];
        rep->checksum = h[F8_CHECKSUM];
        rep->ms_locate = ev.ms(2, 3);
        rep->ms_sort = ev.ms(3, 4);
    }
    return h[F8_WALKFAIL] ? KISS_HIP_E_INVALID : KISS_HIP_OK; // not an index of an exact suffix array: positions undefined
}

int f8_view_check(const kiss_hip_fmi8_view *v, bool want)
{
    if (!v) return KISS_HIP_E_INVALID;
    if (!fm_sa_intv_ok(v->sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    if (v->n_sa == 0 || v->n_sa > KISS_HIP_MAX_N + 1 || v->sigma > 256 || !v->C || !v->map || !v->bwt ||
        (v->sigma && (!v->occ1 || !v->occ2)))
        return KISS_HIP_E_INVALID;
    if (want && (!v->sa || (v->sa_intv != 1 && (!v->b || !v->b_occ)))) return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

// a host view (f8_view_check passed, z: the sizes of its arrays) on the device.  Another kind of view than fm_upload_index
// uploads: C, map, 16-bit occ2.  sigma == 0 has no occ1 / occ2 entries, sa_intv == 1 no b / b_occ: allocated all the same,
// the last two null in the view.
kiss_hip_fmi8_view f8_upload_view(FmStage &st, const kiss_hip_fmi8_view &h, const kiss_hip_fmi8_sizes &z)
{
    const bool bits = h.sa_intv != 1;
    kiss_hip_fmi8_view v = h;
    v.C = st.up(h.C, 257 * 4);
    v.map = st.up(h.map, 256);
    v.bwt = st.up(h.bwt, z.bwt_bytes);
    v.occ1 = h.occ1 ? st.up(h.occ1, z.occ1_entries * 4) : st.room<uint32_t>(true, 0);
    v.occ2 = h.occ2 ? st.up(h.occ2, z.occ2_entries * 2) : st.room<uint16_t>(true, 0);
    v.sa = st.up(h.sa, z.sa_entries * 4);
    v.b = bits ? st.up(h.b, z.b_words * 8, 8) : nullptr;
    v.b_occ = bits ? st.up(h.b_occ, z.b_occ_entries * 4) : nullptr;
    if (!bits) (void)(st.room<uint64_t>(true, z.b_words * 8, 8), st.room<uint32_t>(true, z.b_occ_entries * 4));
    return v;
}

} // namespace

extern "C" {

int kiss_hip_fmi8_sizes_for(uint64_t n, uint32_t sa_intv, uint32_t sigma, kiss_hip_fmi8_sizes *out)
{
    if (!fm_sa_intv_ok(sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    if (!out || n > KISS_HIP_MAX_N || sigma > 256) return KISS_HIP_E_INVALID;
    const uint64_t N = n + 1;
    out->n_sa = N;
    out->bwt_bytes = (N / 256 + 1) * 256;
    out->occ1_entries = (uint64_t)sigma * (N / 65536 + 1);
    out->occ2_entries = (uint64_t)sigma * (N / 256 + 1);
    out->sa_entries = (N + sa_intv - 1) / sa_intv;
    out->b_words = sa_intv == 1 ? 0 : (N + 63) / 64;
    out->b_occ_entries = sa_intv == 1 ? 0 : N / 64 + 1;
    return KISS_HIP_OK;
}

int kiss_hip_fmi8_build_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t sa_intv,
                            uint32_t sigma_capacity, uint32_t *d_C, uint8_t *d_map, uint8_t *d_bwt, uint32_t *d_occ1,
                            uint16_t *d_occ2, uint32_t *d_sa, uint64_t *d_b, uint32_t *d_b_occ, uint32_t *sigma_out,
                            uint32_t *pri_out, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (!fm_sa_intv_ok(sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    if (!ctx || (n && !d_S) || n > KISS_HIP_MAX_N || !sigma_out) return KISS_HIP_E_INVALID;
    if (d_bwt && (!d_SA || !d_C || !d_map || !d_sa || !pri_out || ((uintptr_t)d_bwt & 15) || (n && (!d_occ1 || !d_occ2)) ||
                  (sa_intv != 1 && (!d_b || !d_b_occ))))
        return KISS_HIP_E_INVALID;
    const int rc = f8_build(ctx, d_S, n, d_SA, sa_intv, sigma_capacity, d_C, d_map, d_bwt, d_occ1, d_occ2, d_sa, d_b, d_b_occ,
                            sigma_out, pri_out, stream);
    (void)hipStreamSynchronize(ctx->stream);
    ktimer_collect(ctx);
    return rc;
}

int kiss_hip_fmi8_query_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi8_view *fmi, const uint8_t *patterns, const uint64_t *pat_index,
                            uint64_t Q, uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum,
                            uint32_t *positions, uint64_t *index, uint64_t capacity, kiss_hip_fmi8_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_fmi8_report{};
        report->Q = Q;
    }
    if (hit_count_total) *hit_count_total = 0;
    if (checksum) *checksum = 0;
    const bool any = positions || index, all = positions && index;
    KTRY(f8_view_check(fmi, all));
    if (!ctx || (Q && (!patterns || !pat_index || !beg || !end)) || any != all || (!any && capacity) || ((uintptr_t)fmi->bwt & 15))
        return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) {
        if (all) { // index[0] = 0
            KTRY(kiss_zero_u32(ctx, index, 2));
            KCHECK(hipStreamSynchronize(ctx->stream));
        }
        return KISS_HIP_OK;
    }
    FmEvents ev(ctx, report != nullptr);
    const int rc = f8_query_steps(ctx, fmi, patterns, pat_index, Q, beg, end, hit_count_total, checksum, positions, index, capacity,
                                  report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi8_build_host(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t sa_intv, uint32_t sigma_capacity,
                             uint32_t *C, uint8_t *map, uint8_t *bwt, uint32_t *occ1, uint16_t *occ2, uint32_t *sa, uint64_t *b,
                             uint32_t *b_occ, uint32_t *sigma_out, uint32_t *pri_out, int device)
{
    kiss_hip_fmi8_sizes z;
    KTRY(kiss_hip_fmi8_sizes_for(n, sa_intv, sigma_capacity > 256 ? 256 : sigma_capacity, &z));
    if ((n && !S) || !sigma_out) return KISS_HIP_E_INVALID;
    if (bwt && (!C || !map || !sa || !pri_out || (n && (!occ1 || !occ2)) || (sa_intv != 1 && (!b || !b_occ)))) return KISS_HIP_E_INVALID;
    return kiss_one_shot_own(device, n < (1u << 20) ? (1u << 20) : n, [&](kiss_hip_ctx *ctx) -> int {
        const bool full = bwt != nullptr; // (else the census: C, map and sigma alone)
        FmStage st(ctx);
        const uint8_t *dS = S ? st.up(S, n) : st.room<uint8_t>(true, 0); // (n == 0: no text, still a pointer)
        uint32_t *dC = st.room<uint32_t>(true, 257 * 4);
        uint8_t *dmap = st.room<uint8_t>(true, 256);
        const uint32_t *dSA = full ? st.up(SA_or_null, (n + 1) * 4) : nullptr;
        uint32_t *sorted = st.room<uint32_t>(full && !SA_or_null, (n + 1) * 4);
        uint8_t *dbwt = st.room<uint8_t>(full, z.bwt_bytes);
        uint32_t *docc1 = st.room<uint32_t>(full, z.occ1_entries * 4);
        uint16_t *docc2 = st.room<uint16_t>(full, z.occ2_entries * 2);
        uint32_t *dsa = st.room<uint32_t>(full, z.sa_entries * 4);
        uint64_t *db = st.room<uint64_t>(full, z.b_words * 8, 8);
        uint32_t *dbocc = st.room<uint32_t>(full, z.b_occ_entries * 4);
        if (st.rc) return st.rc;
        if (sorted) {
            KTRY(kiss_hip_ctx_suffix_sort_u8_dev(ctx, dS, n, sorted, nullptr));
            dSA = sorted;
        }
        KTRY(kiss_hip_fmi8_build_dev(ctx, dS, n, dSA, sa_intv, full ? sigma_capacity : 0, dC, dmap, dbwt, docc1, docc2, dsa, db, dbocc,
                                     sigma_out, full ? pri_out : nullptr, nullptr));
        if (C) st.down(C, dC, 257 * 4);
        if (map) st.down(map, dmap, 256);
        if (full) {
            kiss_hip_fmi8_sizes zs; // occ1 / occ2 are laid out for the text's own sigma
            (void)kiss_hip_fmi8_sizes_for(n, sa_intv, *sigma_out, &zs);
            st.down(bwt, dbwt, zs.bwt_bytes);
            st.down(occ1, docc1, zs.occ1_entries * 4);
            st.down(occ2, docc2, zs.occ2_entries * 2);
            st.down(sa, dsa, zs.sa_entries * 4);
            st.down(b, db, zs.b_words * 8);
            st.down(b_occ, dbocc, zs.b_occ_entries * 4);
        }
        return st.rc;
    });
}

int kiss_hip_fmi8_query_host(const kiss_hip_fmi8_view *fmi, const uint8_t *patterns, const uint64_t *pat_index, uint64_t Q,
                             uint32_t *beg, uint32_t *end, uint64_t *hit_count_total, uint64_t *checksum, uint32_t *positions,
                             uint64_t *index, uint64_t capacity, kiss_hip_fmi8_report *report, int device)
{
    if (report) {
        *report = kiss_hip_fmi8_report{};
        report->Q = Q;
    }
    if (hit_count_total) *hit_count_total = 0;
    if (checksum) *checksum = 0;
    const bool any = positions || index, all = positions && index;
    KTRY(f8_view_check(fmi, true));
    if ((Q && (!patterns || !pat_index || !beg || !end)) || any != all || (!any && capacity)) return KISS_HIP_E_INVALID;
    if (!fm_index_ascending(pat_index, Q, true)) return KISS_HIP_E_INVALID;
    kiss_hip_fmi8_sizes z;
    KTRY(kiss_hip_fmi8_sizes_for(fmi->n_sa - 1, fmi->sa_intv, fmi->sigma, &z));
    const uint64_t pat_bytes = Q ? pat_index[Q] : 0;
    // (the hits of a call are sorted in the ctx's LMS arrays)
    return kiss_one_shot_own(device, fm_host_max_n(fmi->n_sa, Q, capacity), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const kiss_hip_fmi8_view v = f8_upload_view(st, *fmi, z);
        const uint8_t *dpat = st.up(patterns, pat_bytes);
        const uint64_t *dpidx = st.up(Q ? pat_index : nullptr, (Q + 1) * 8);
        uint32_t *dbeg = st.room<uint32_t>(true, Q * 4), *dend = st.room<uint32_t>(true, Q * 4);
        uint32_t *dpos = st.room<uint32_t>(all, capacity * 4);
        uint64_t *didx = st.room<uint64_t>(all, (Q + 1) * 8);
        if (st.rc) return st.rc;
        uint64_t total = 0;
        const int rc = kiss_hip_fmi8_query_dev(ctx, &v, dpat, dpidx, Q, dbeg, dend, &total, checksum, dpos, didx, all ? capacity : 0, report,
                                               nullptr);
        if (hit_count_total) *hit_count_total = total;
        if (rc) return rc;
        st.down(beg, dbeg, Q * 4);
        st.down(end, dend, Q * 4);
        if (all) st.down(index, didx, (Q + 1) * 8);
        if (all) st.down(positions, dpos, total * 4);
        return st.rc;
    });
}

} // extern "C"
