// lcp.hip -- the LCP array of a text from its exact suffix array, DNA (2-bit codes) and bytes.
//
// LCP[0] = 0, LCP[i] = lcp(SA[i-1], SA[i]) for i >= 1 (SA[0] = n, the empty suffix, so LCP[1] = 0).  Computed through the
// permuted LCP array with irreducible values (Kaerkkaeinen, Manzini, Puglisi 2009, "Permuted Longest-Common-Prefix
// Array"): no Kasai chain, every pass is data-parallel.
//   1. Phi      : Phi[SA[i]] = SA[i-1] (i >= 1), over an array first filled with n, so that a duplicate in a bad SA leaves
//                 no stale index behind.  The same pass checks SA[0] == n and SA[i] <= n.
//   2. short    : one lane per text position i.  i is REDUCIBLE when i >= 1, Phi(i) >= 1, Phi(i) != n and
//                 S[i-1] == S[Phi(i)-1]: then PLCP[i] = PLCP[i-1] - 1 and nothing is compared.  Otherwise lcp(i, Phi(i))
//                 is computed directly, clamped at n - max(i, Phi(i)).  One chunk gathered at Phi(i) - 1 (32 bases / 8
//                 bytes) holds the symbol of the test and the first 31 bases / 7 bytes of the compare.  Compares that are
//                 still equal after LCP_SHORT_CHUNKS more chunks go to an overflow list.
//   3. long     : the list, one wave per pair (64 chunks per step, LCP_WAVE_STEPS steps); what is still equal after that
//                 goes to a second list that the whole grid walks one pair at a time (workgroups take segments of the
//                 pair from a ticket and stop at the first mismatch any of them has found).  An all-A text has one
//                 irreducible pair, of lcp n - 1: it is read at the memory rate, not by a lane.
//   4. max-scan : PLCP[i] + i is non-decreasing and equals the computed value at every irreducible position, so the
//                 inclusive running maximum of X[i] = (irreducible ? i + lcp : 0) is PLCP[i] + i everywhere.
//   5. gather   : LCP[i] = PLCP[SA[i]] (in place allowed: d_LCP may be d_SA), plus the sum and the maximum.
// The sum of the irreducible lcps is at most 2 n log2 n (ibid.), about n on real texts: the compare work is linear in
// practice.  For an SA that is a permutation but not the exact order (a k-ordered SA) the Phi relation does not hold:
// the values are then unspecified, the call still stays inside its arrays and returns KISS_HIP_OK.
//
// Workspace: nothing of its own.  X / PLCP live in ctx->CTX (n + 1 words), the overflow lists in keyA / keyB, the
// per-pair state of the grid-wide compare in posA / posB, the block maxima of the scan in flags, the byte text's
// padded copy in ctx->CLS, the packed DNA text in ctx->pk.  After an exact sort of the same n all of them exist.
#include "kiss_internal.hpp"
#include <cstring>

namespace {

constexpr int LCP_THREADS = 256;
constexpr uint32_t LCP_SHORT_CHUNKS = 4; // lane compare: chunks after the first, then the overflow list
constexpr uint32_t LCP_WAVE_STEPS = 64;  // wave compare: 64 chunks per step, then the grid-wide list
constexpr uint32_t LCP_WIDE_CHUNKS = 4;  // grid-wide compare: chunks per lane and segment
constexpr unsigned LCP_WAVE_BLOCKS = 1024, LCP_WIDE_BLOCKS = 256;
constexpr unsigned LCP_STRIDE_BLOCKS = 8192; // grid of the short compare and the gather (32 workgroups per CU)
constexpr int LCP_SCAN_ROWS = 4, LCP_SCAN_VEC = 4;
constexpr uint64_t LCP_SCAN_ROW = (uint64_t)LCP_THREADS * LCP_SCAN_VEC, LCP_SCAN_BLOCK = LCP_SCAN_ROW * LCP_SCAN_ROWS;

// control words in ctx->d_small[0, 8): bad SA, overflow list entries, grid-wide list entries, irreducible positions,
// lcp sum (u64 at 4..5), max lcp
enum { C_BAD = 0, C_LIST = 1, C_WIDE = 2, C_IRR = 3, C_SUM = 4, C_MAX = 6, C_WORDS = 8 };

// ---- the two texts: a chunk of consecutive symbols starting at any position, through naturally aligned loads --------
struct DnaText {
    const uint64_t *pk; // 2-bit packed (kiss_pack_text), spare zero words behind the text
    static constexpr uint32_t SYMS = 32;
    __device__ __forceinline__ uint64_t chunk(uint64_t p) const { return kiss_key32(pk, p); }
    __device__ static __forceinline__ uint32_t first_sym(uint64_t c) { return (uint32_t)(c >> 62); }
    __device__ static __forceinline__ uint64_t drop_first(uint64_t x) { return x << 2; }
    __device__ static __forceinline__ uint32_t first_diff(uint64_t x) { return (uint32_t)__clzll((long long)x) >> 1; } // x != 0
};
struct ByteText {
    const uint64_t *w; // padded copy of the bytes (byte p = bits 8(p%8).. of word p/8), >= 7 spare words behind the text
    static constexpr uint32_t SYMS = 8;
    __device__ __forceinline__ uint64_t chunk(uint64_t p) const
    {
        uint64_t a, b;
        kiss_words2(w, p >> 3, a, b);
        const uint32_t s = (uint32_t)(p & 7u) * 8u;
        return (a >> s) | ((b << 1) << (63u - s)); // branch-free: s == 0 gives a
    }
    __device__ static __forceinline__ uint32_t first_sym(uint64_t c) { return (uint32_t)(c & 0xFFu); }
    __device__ static __forceinline__ uint64_t drop_first(uint64_t x) { return x >> 8; }
    __device__ static __forceinline__ uint32_t first_diff(uint64_t x) { return (uint32_t)__builtin_ctzll(x) >> 3; }
};

// the caller's n bytes into the padded words (zeros behind the text): the caller's buffer is never read past n
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_copy_bytes(const uint8_t *__restrict__ S, uint64_t n,
                                                               uint64_t *__restrict__ out, uint64_t words)
{
    const uint64_t w = (uint64_t)blockIdx.x * LCP_THREADS + threadIdx.x;
    if (w >= words) return;
    uint64_t v = 0;
    const uint64_t base = w * 8;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
        if (base + j < n) v |= (uint64_t)S[base + j] << (8u * j);
    out[w] = v;
}

// Phi[SA[i]] = SA[i-1] (Phi filled with n before); validation of SA folded in
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_phi(const uint32_t *SA, uint64_t n, uint32_t *__restrict__ phi,
                                                        uint32_t *__restrict__ ctl)
{
    const uint64_t i = (uint64_t)blockIdx.x * LCP_THREADS + threadIdx.x;
    if (i > n) return;
    const uint32_t s = SA[i];
    const bool bad = s > n || (i == 0 && s != (uint32_t)n);
    if (bad) atomicOr(&ctl[C_BAD], 1u);
    else if (i >= 1) {
        const uint32_t prev = SA[i - 1];
        if (prev <= n) phi[s] = prev;
    }
}

template <class T>
__device__ __forceinline__ uint64_t lcp_serial(const T &t, uint64_t i, uint64_t ph, uint64_t off, uint64_t L)
{
    for (;; off += T::SYMS) {
        if (off >= L) return L;
        const uint64_t x = t.chunk(i + off) ^ t.chunk(ph + off);
        if (x) {
            const uint64_t r = off + T::first_diff(x);
            return r < L ? r : L;
        }
    }
}

// sum over the workgroup, one atomic per workgroup: a same-address atomic per wave costs ~20 ns each and there are n / 64
// waves (measured: 48 M of them made up most of a 1.9 s LCP call at chm13 size)
template <typename V, typename Op>
__device__ __forceinline__ V block_reduce(V v, Op op)
{
    __shared__ V lds[LCP_THREADS / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, (V)__shfl_xor(v, d, 64));
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < LCP_THREADS / 64; w++) v = op(v, lds[w]);
    return v; // (thread 0)
}

// X[i] (Phi(i) in) -> i + lcp(i, Phi(i)) at irreducible positions, 0 at reducible ones; left as it is for positions
// handed to the overflow list (the long passes write it).  X[n] = n.  A fixed grid strides over the positions.
template <class T>
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_short(T t, uint64_t n, uint32_t *__restrict__ X,
                                                          uint64_t *__restrict__ list, uint64_t cap, uint32_t *__restrict__ ctl)
{
    uint32_t irr_count = 0;
    const uint64_t stride = (uint64_t)gridDim.x * LCP_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * LCP_THREADS + threadIdx.x; i <= n; i += stride) {
        if (i == n) {
            X[n] = (uint32_t)n;
            continue;
        }
        const uint64_t ph = X[i];
        const uint64_t L = n - (i > ph ? i : ph);
        bool irr = true, listed = false, done = false;
        uint64_t lcp = 0, off = 0;
        if (i >= 1 && ph >= 1 && ph < n) {
            const uint64_t a = t.chunk(i - 1), b = t.chunk(ph - 1);
            if (T::first_sym(a) == T::first_sym(b)) {
                irr = false;
                done = true;
            } else {
                const uint64_t x = T::drop_first(a ^ b);
                if (x) {
                    lcp = T::first_diff(x);
                    done = true;
                } else {
                    off = T::SYMS - 1;
                }
            }
        }
        if (irr && !done) {
            for (;; off += T::SYMS) {
                if (off >= L) {
                    lcp = L;
                    break;
                }
                if (off >= (uint64_t)LCP_SHORT_CHUNKS * T::SYMS) { // [0, off) equal: to the long passes
                    const uint32_t e = atomicAdd(&ctl[C_LIST], 1u);
                    if (e < cap) {
                        list[e] = (i << 32) | ph;
                        listed = true;
                    } else {
                        lcp = lcp_serial(t, i, ph, off, L); // (list full: see lcp_passes)
                    }
                    break;
                }
                const uint64_t x = t.chunk(i + off) ^ t.chunk(ph + off);
                if (x) {
                    lcp = off + T::first_diff(x);
                    break;
                }
            }
        }
        if (!listed) X[i] = irr ? (uint32_t)(i + (lcp < L ? lcp : L)) : 0u;
        irr_count += irr ? 1u : 0u;
    }
    irr_count = block_reduce(irr_count, [](uint32_t a, uint32_t b) { return a + b; });
    if (threadIdx.x == 0 && irr_count) atomicAdd(&ctl[C_IRR], irr_count);
}

// the overflow list, one wave per pair; [0, LCP_SHORT_CHUNKS * SYMS) is known to be equal
template <class T>
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_wave(T t, uint64_t n, uint32_t *__restrict__ X,
                                                         const uint64_t *__restrict__ list, uint64_t cap,
                                                         uint64_t *__restrict__ wide, uint32_t *__restrict__ wfound,
                                                         uint32_t *__restrict__ wticket, uint32_t *__restrict__ ctl)
{
    const uint64_t listed = ctl[C_LIST];
    const uint64_t count = listed < cap ? listed : cap;
    const uint64_t waves = (uint64_t)gridDim.x * (LCP_THREADS / 64);
    const uint32_t lane = lane_id();
    for (uint64_t e = (uint64_t)blockIdx.x * (LCP_THREADS / 64) + (threadIdx.x >> 6); e < count; e += waves) {
        const uint64_t pr = list[e];
        const uint64_t i = pr >> 32, ph = pr & 0xFFFFFFFFull;
        const uint64_t L = n - (i > ph ? i : ph);
        uint64_t off = (uint64_t)LCP_SHORT_CHUNKS * T::SYMS;
        uint64_t lcp = ~0ull;
        for (uint32_t step = 0;; step++, off += 64ull * T::SYMS) {
            if (step == LCP_WAVE_STEPS && off < L) { // still equal: to the grid-wide compare
                uint32_t w = 0;
                if (lane == 0) w = atomicAdd(&ctl[C_WIDE], 1u);
                w = (uint32_t)__shfl((int)w, 0, 64);
                if (w < cap) {
                    if (lane == 0) {
                        wide[w] = pr;
                        wfound[w] = (uint32_t)L;
                        wticket[w] = 0;
                    }
                    break;
                } // (list full: this wave walks on)
            }
            const uint64_t o = off + (uint64_t)lane * T::SYMS;
            const bool past = o >= L;
            uint64_t x = 0;
            if (!past) x = t.chunk(i + o) ^ t.chunk(ph + o);
            const uint64_t hit = __ballot(past || x != 0);
            if (hit) {
                const uint64_t v = past ? L : o + T::first_diff(x);
                lcp = __shfl(v, (int)__builtin_ctzll(hit), 64);
                if (lcp > L) lcp = L;
                break;
            }
        }
        if (lcp != ~0ull && lane == 0) X[i] = (uint32_t)(i + lcp);
    }
}

// the grid-wide list, one pair at a time: workgroups take segments of LCP_THREADS * LCP_WIDE_CHUNKS chunks from the
// pair's ticket and lower wfound to every mismatch they see; a segment that starts at or behind wfound is not needed
template <class T>
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_wide(T t, uint64_t n, const uint64_t *__restrict__ wide, uint32_t *wfound,
                                                         uint32_t *wticket, const uint32_t *__restrict__ ctl, uint64_t cap)
{
    __shared__ uint32_t s_seg, s_found;
    const uint64_t listed = ctl[C_WIDE];
    const uint64_t count = listed < cap ? listed : cap;
    constexpr uint64_t SEG = (uint64_t)LCP_THREADS * LCP_WIDE_CHUNKS * T::SYMS;
    const uint64_t start = (uint64_t)LCP_SHORT_CHUNKS * T::SYMS + (uint64_t)LCP_WAVE_STEPS * 64 * T::SYMS;
    for (uint64_t p = 0; p < count; p++) {
        const uint64_t pr = wide[p];
        const uint64_t i = pr >> 32, ph = pr & 0xFFFFFFFFull;
        for (;;) {
            if (threadIdx.x == 0) {
                s_seg = atomicAdd(&wticket[p], 1u);
                s_found = __hip_atomic_load(&wfound[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            const uint64_t base = start + (uint64_t)s_seg * SEG;
            const uint64_t found = s_found;
            __syncthreads();
            if (base >= found) break; // (the same decision in every lane of the workgroup)
            for (uint32_t c = 0; c < LCP_WIDE_CHUNKS; c++) {
                const uint64_t o = base + ((uint64_t)c * LCP_THREADS + threadIdx.x) * T::SYMS;
                if (o < found) {
                    const uint64_t x = t.chunk(i + o) ^ t.chunk(ph + o);
                    if (x) atomicMin(&wfound[p], (uint32_t)(o + T::first_diff(x)));
                }
            }
        }
    }
}

__global__ __launch_bounds__(LCP_THREADS) void k_lcp_wide_done(uint64_t n, uint32_t *__restrict__ X, const uint64_t *__restrict__ wide,
                                                              const uint32_t *__restrict__ wfound, const uint32_t *__restrict__ ctl,
                                                              uint64_t cap)
{
    const uint64_t listed = ctl[C_WIDE];
    const uint64_t count = listed < cap ? listed : cap;
    for (uint64_t p = (uint64_t)blockIdx.x * LCP_THREADS + threadIdx.x; p < count; p += (uint64_t)gridDim.x * LCP_THREADS) {
        const uint64_t i = wide[p] >> 32, ph = wide[p] & 0xFFFFFFFFull;
        const uint64_t L = n - (i > ph ? i : ph);
        const uint64_t f = wfound[p];
        X[i] = (uint32_t)(i + (f < L ? f : L));
    }
}

// ---- inclusive max-scan of X[0, count) (three launches, as scan.hip's sums), then PLCP[i] = max - i in place --------
__device__ __forceinline__ void lcp_load4(const uint32_t *X, uint64_t base, uint64_t count, uint32_t v[4])
{
    if (base + 4 <= count) { // base is a multiple of 4 and X 16-byte aligned (ctx->CTX)
        const uint4 q = *reinterpret_cast<const uint4 *>(X + base);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = base + e < count ? X[base + e] : 0u;
    }
}

__device__ __forceinline__ uint32_t wave_max_inclusive(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if ((int)lane_id() >= d) v = v > o ? v : o;
    }
    return v;
}

__global__ __launch_bounds__(LCP_THREADS) void k_lcp_max_reduce(const uint32_t *__restrict__ X, uint64_t count,
                                                               uint32_t *__restrict__ bmax)
{
    __shared__ uint32_t lds[LCP_THREADS / 64];
    const uint64_t b = (uint64_t)blockIdx.x * LCP_SCAN_BLOCK + (uint64_t)threadIdx.x * LCP_SCAN_VEC;
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < LCP_SCAN_ROWS; r++) {
        uint32_t v[4];
        lcp_load4(X, b + r * LCP_SCAN_ROW, count, v);
        m = max(m, max(max(v[0], v[1]), max(v[2], v[3])));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if (lane_id() == 0) lds[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < LCP_THREADS / 64; w++) t = max(t, lds[w]);
        bmax[blockIdx.x] = t;
    }
}

// exclusive max-scan of the block maxima in place (one workgroup)
__global__ __launch_bounds__(1024) void k_lcp_max_single(uint32_t *__restrict__ data, uint64_t count)
{
    __shared__ uint32_t lds[1024 / 64];
    const uint64_t chunk = (count + 1023) / 1024;
    const uint64_t beg = (uint64_t)threadIdx.x * chunk;
    const uint64_t end = beg + chunk < count ? beg + chunk : count;
    uint32_t s = 0;
    for (uint64_t i = beg; i < end; i++) s = max(s, data[i]);
    const int wave = threadIdx.x >> 6;
    const uint32_t inc = wave_max_inclusive(s);
    if (lane_id() == 63) lds[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < 1024 / 64; w++) {
            const uint32_t t = lds[w];
            lds[w] = acc;
            acc = max(acc, t);
        }
    }
    __syncthreads();
    uint32_t excl = (uint32_t)__shfl_up((int)inc, 1, 64);
    if (lane_id() == 0) excl = 0;
    uint32_t run = max(excl, lds[wave]);
    for (uint64_t i = beg; i < end; i++) {
        const uint32_t t = data[i];
        data[i] = run;
        run = max(run, t);
    }
}

__global__ __launch_bounds__(LCP_THREADS) void k_lcp_max_final(uint32_t *X, uint64_t count, const uint32_t *__restrict__ bmax)
{
    __shared__ uint32_t wmax[LCP_SCAN_ROWS][LCP_THREADS / 64];
    const int wave = threadIdx.x >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * LCP_SCAN_BLOCK + (uint64_t)threadIdx.x * LCP_SCAN_VEC;
    uint32_t v[LCP_SCAN_ROWS][4], inc[LCP_SCAN_ROWS];
#pragma unroll
    for (int r = 0; r < LCP_SCAN_ROWS; r++) {
        lcp_load4(X, b + r * LCP_SCAN_ROW, count, v[r]);
        v[r][1] = max(v[r][1], v[r][0]);
        v[r][2] = max(v[r][2], v[r][1]);
        v[r][3] = max(v[r][3], v[r][2]);
        inc[r] = wave_max_inclusive(v[r][3]);
        if (lane_id() == 63) wmax[r][wave] = inc[r];
    }
    __syncthreads();
    uint32_t run = bmax[blockIdx.x];
#pragma unroll
    for (int r = 0; r < LCP_SCAN_ROWS; r++) {
        uint32_t pre = run;
#pragma unroll
        for (int w = 0; w < LCP_THREADS / 64; w++) {
            if (w < wave) pre = max(pre, wmax[r][w]);
            run = max(run, wmax[r][w]);
        }
        uint32_t excl = (uint32_t)__shfl_up((int)inc[r], 1, 64);
        if (lane_id() == 0) excl = 0;
        pre = max(pre, excl);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint64_t j = b + r * LCP_SCAN_ROW + e;
            if (j < count) X[j] = max(pre, v[r][e]) - (uint32_t)j; // PLCP[j]
        }
    }
}

// LCP[i] = PLCP[SA[i]] (LCP may be SA: every lane reads its own entry before it writes it); sum and maximum of LCP[1..n]
__global__ __launch_bounds__(LCP_THREADS) void k_lcp_gather(const uint32_t *SA, uint64_t n, const uint32_t *__restrict__ P,
                                                           uint32_t *LCP, uint32_t *__restrict__ ctl)
{
    uint64_t sum = 0;
    uint32_t m = 0;
    const uint64_t stride = (uint64_t)gridDim.x * LCP_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * LCP_THREADS + threadIdx.x; i <= n; i += stride) {
        uint32_t v = 0;
        if (i >= 1) {
            const uint32_t s = SA[i];
            v = P[s <= n ? s : n];
        }
        LCP[i] = v;
        sum += v;
        m = max(m, v);
    }
    sum = block_reduce(sum, [](uint64_t a, uint64_t b) { return a + b; });
    m = block_reduce(m, [](uint32_t a, uint32_t b) { return max(a, b); });
    if (threadIdx.x == 0 && sum) {
        atomicAdd(reinterpret_cast<unsigned long long *>(ctl + C_SUM), (unsigned long long)sum);
        atomicMax(&ctl[C_MAX], m);
    }
}

struct LcpEvents {
    hipEvent_t e[5] = {};
    bool ok = true;
    LcpEvents()
    {
        for (auto &x : e)
            if (hipEventCreate(&x) != hipSuccess) ok = false;
    }
    ~LcpEvents()
    {
        for (auto &x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

template <class T>
int lcp_passes(kiss_hip_ctx *ctx, const T &t, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP, kiss_hip_lcp_report *rep,
               LcpEvents &ev)
{
    uint32_t *X = ctx->CTX, *ctl = ctx->d_small;
    const uint64_t cap = ctx->m_cap;
    const unsigned grid = (unsigned)div_up(n + 1, LCP_THREADS);
    const unsigned grid_fixed = grid < LCP_STRIDE_BLOCKS ? grid : LCP_STRIDE_BLOCKS; // (kernels that stride)
    KTRY(kiss_fill_u32(ctx, X, (uint32_t)n, n + 1));
    hipLaunchKernelGGL(k_lcp_phi, dim3(grid), dim3(LCP_THREADS), 0, ctx->stream, d_SA, n, X, ctl);
    KCHECK(hipGetLastError());
    (void)hipEventRecord(ev.e[1], ctx->stream);
    KTRY(kiss_readback(ctx, ctl + C_BAD, 1));
    if (ctx->h_pinned[0]) return KISS_HIP_E_INVALID; // (nothing written to d_LCP)
    // The overflow list holds the irreducible pairs with an lcp of LCP_SHORT_CHUNKS chunks or more: 0.03 % of the
    // positions at chm13 size, against a capacity of >= 0.32 max_n.  (The bound 2 n log2 n / 128 of an exact SA can exceed
    // it: what does not fit is compared by the lane that found it.)
    hipLaunchKernelGGL((k_lcp_short<T>), dim3(grid_fixed), dim3(LCP_THREADS), 0, ctx->stream, t, n, X, ctx->keyA, cap, ctl);
    KCHECK(hipGetLastError());
    (void)hipEventRecord(ev.e[2], ctx->stream);
    hipLaunchKernelGGL((k_lcp_wave<T>), dim3(LCP_WAVE_BLOCKS), dim3(LCP_THREADS), 0, ctx->stream, t, n, X, ctx->keyA, cap,
                       ctx->keyB, ctx->posA, ctx->posB, ctl);
    hipLaunchKernelGGL((k_lcp_wide<T>), dim3(LCP_WIDE_BLOCKS), dim3(LCP_THREADS), 0, ctx->stream, t, n, ctx->keyB, ctx->posA,
                       ctx->posB, ctl, cap);
    hipLaunchKernelGGL(k_lcp_wide_done, dim3(LCP_WIDE_BLOCKS), dim3(LCP_THREADS), 0, ctx->stream, n, X, ctx->keyB, ctx->posA,
                       ctl, cap);
    KCHECK(hipGetLastError());
    (void)hipEventRecord(ev.e[3], ctx->stream);
    const uint64_t count = n + 1, nb = div_up(count, LCP_SCAN_BLOCK);
    // block maxima in `flags`: >= 2 ((max_n + 1) / 2048 + 2) u64 whatever the LMS capacity (api.hip: kiss_tied_reserve)
    if (nb > 2 * ctx->flags_cap) return KINTERNAL();
    uint32_t *bmax = reinterpret_cast<uint32_t *>(ctx->flags);
    hipLaunchKernelGGL(k_lcp_max_reduce, dim3((unsigned)nb), dim3(LCP_THREADS), 0, ctx->stream, X, count, bmax);
    hipLaunchKernelGGL(k_lcp_max_single, dim3(1), dim3(1024), 0, ctx->stream, bmax, nb);
    hipLaunchKernelGGL(k_lcp_max_final, dim3((unsigned)nb), dim3(LCP_THREADS), 0, ctx->stream, X, count, bmax);
    hipLaunchKernelGGL(k_lcp_gather, dim3(grid_fixed), dim3(LCP_THREADS), 0, ctx->stream, d_SA, n, X, d_LCP, ctl);
    KCHECK(hipGetLastError());
    (void)hipEventRecord(ev.e[4], ctx->stream);
    KTRY(kiss_readback(ctx, ctl, C_WORDS));
    if (rep) {
        const uint32_t *h = ctx->h_pinned;
        rep->irreducible = h[C_IRR];
        rep->long_pairs = h[C_LIST];
        rep->lcp_sum = (uint64_t)h[C_SUM] | ((uint64_t)h[C_SUM + 1] << 32);
        rep->max_lcp = h[C_MAX];
    }
    return KISS_HIP_OK;
}

int lcp_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP,
            kiss_hip_lcp_report *report, void *stream, bool bytes)
{
    if (!ctx || !d_SA || !d_LCP || (n && !d_S)) return KISS_HIP_E_INVALID;
    if (n > KISS_HIP_MAX_N || n > ctx->max_n) return KISS_HIP_E_INVALID;
    kiss_opts_refresh(ctx);
    std::unique_lock<std::mutex> lock(kiss_device_mutex(ctx->device), std::defer_lock);
    if (!ctx->opts.no_serialize) lock.lock(); // the lock of the sorts (api.hip: sort_dev)
    KCHECK(hipSetDevice(ctx->device));
    KissCallStream call_stream(ctx, stream); // the caller's stream for this call, the ctx's own again on every way out
    KTRY(kiss_workspace_ready(ctx));
    KTRY(kiss_need_ctx_words(ctx));
    ctx->ctx_words_valid = false; // CTX is about to hold Phi / PLCP (and CLS the byte text): no taint words to reuse
    kiss_hip_lcp_report rep{};
    rep.n = n;
    LcpEvents ev;
    if (!ev.ok) return KISS_HIP_E_HIP;
    KTRY(kiss_zero_u32(ctx, ctx->d_small, C_WORDS));
    (void)hipEventRecord(ev.e[0], ctx->stream);
    int rc;
    if (bytes) {
        const uint64_t words = div_up(n, 8) + 7; // <= (max_n + 66) / 8: the size of ctx->CLS
        uint64_t *w = reinterpret_cast<uint64_t *>(ctx->CLS);
        hipLaunchKernelGGL(k_lcp_copy_bytes, dim3((unsigned)div_up(words, LCP_THREADS)), dim3(LCP_THREADS), 0, ctx->stream, d_S, n,
                           w, words);
        KCHECK(hipGetLastError());
        rc = lcp_passes(ctx, ByteText{w}, n, d_SA, d_LCP, &rep, ev);
    } else {
        const uint64_t mask = ctx->profile_mask; // (kernel-class timing belongs to the sort statistics: none from here)
        ctx->profile_mask = 0;
        rc = n ? kiss_pack_text(ctx, d_S, n) : KISS_HIP_OK;
        ctx->profile_mask = mask;
        KTRY(rc);
        rc = lcp_passes(ctx, DnaText{ctx->pk}, n, d_SA, d_LCP, &rep, ev);
    }
    if (rc != KISS_HIP_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    float *ms[4] = {&rep.ms_phi, &rep.ms_short, &rep.ms_long, &rep.ms_scan_gather};
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]);
    (void)hipEventElapsedTime(&rep.ms_total, ev.e[0], ev.e[4]);
    if (report) *report = rep;
    return KISS_HIP_OK;
}

// host-pointer one-shot on the device's cached context: S (and SA when given) up, SA down when it was sorted here,
// LCP computed over the device copy of SA in place and brought down
int lcp_host(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t *SA_out, uint32_t *LCP, int device, bool bytes)
{
    if (!LCP || (n && !S)) return KISS_HIP_E_INVALID;
    if (n > KISS_HIP_MAX_N) return KISS_HIP_E_INVALID;
    if (n == 0) { // no device work, as kiss_hip_suffix_sort_dna_u32
        if (SA_or_null && SA_or_null[0] != 0) return KISS_HIP_E_INVALID;
        if (SA_out) SA_out[0] = 0;
        LCP[0] = 0;
        return KISS_HIP_OK;
    }
    return kiss_one_shot_cached(device, n, [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t sa_bytes = (n + 1) * sizeof(uint32_t);
        KCHECK(hipSetDevice(ctx->device));
        if (!SA_or_null && !bytes) {
            // the DNA sort's own host-pointer path: S goes up into ctx->io_S, the exact SA stays in ctx->io_SA as well
            uint32_t *dst = SA_out ? SA_out : LCP;
            KTRY(kiss_hip_ctx_suffix_sort_dna_u32(ctx, S, n, 0xFFFFFFFFu, KISS_HIP_ALGO_PREFIX_DOUBLING, dst));
        } else {
            KTRY(kiss_io_reserve(ctx, n));
            KTRY(kiss_xfer_h2d(ctx, ctx->io_S, S, n));
            if (SA_or_null) {
                KTRY(kiss_xfer_h2d(ctx, ctx->io_SA, SA_or_null, sa_bytes));
            } else {
                KTRY(kiss_hip_ctx_suffix_sort_u8_dev(ctx, ctx->io_S, n, ctx->io_SA, nullptr));
                if (SA_out) KTRY(kiss_xfer_d2h(ctx, SA_out, ctx->io_SA, sa_bytes));
            }
            if (SA_or_null && SA_out && SA_out != SA_or_null) std::memcpy(SA_out, SA_or_null, sa_bytes);
        }
        KTRY(lcp_dev(ctx, ctx->io_S, n, ctx->io_SA, ctx->io_SA, nullptr, nullptr, bytes));
        return kiss_xfer_d2h(ctx, LCP, ctx->io_SA, sa_bytes);
    });
}

} // namespace

extern "C" {

int kiss_hip_ctx_lcp_dna_u32_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP,
                                 kiss_hip_lcp_report *report, void *stream)
{
    return lcp_dev(ctx, d_S, n, d_SA, d_LCP, report, stream, false);
}

int kiss_hip_ctx_lcp_u8_dev(kiss_hip_ctx *ctx, const uint8_t *d_S, uint64_t n, const uint32_t *d_SA, uint32_t *d_LCP,
                            kiss_hip_lcp_report *report, void *stream)
{
    return lcp_dev(ctx, d_S, n, d_SA, d_LCP, report, stream, true);
}

int kiss_hip_lcp_dna_u32(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t *SA_out, uint32_t *LCP, int device)
{
    return lcp_host(S, n, SA_or_null, SA_out, LCP, device, false);
}

int kiss_hip_lcp_u8(const uint8_t *S, uint64_t n, const uint32_t *SA_or_null, uint32_t *SA_out, uint32_t *LCP, int device)
{
    return lcp_host(S, n, SA_or_null, SA_out, LCP, device, true);
}

} // extern "C"
