// fm_seed.hip -- FM-index: maximal exact match seeds of a ragged batch of reads (kiss_hip_fmi_seeds_*).
//
// The reference has no such function; ground truth is the text itself (tests/fm_seed_model.py).  For a read R of L bytes
// (0..3 = a base, anything else = no base: no match contains it) and an end e in 1..L, ms[e] is the length of the longest
// suffix of R[0, e) -- at most max_len bases when max_len != 0 -- that occurs in the text, start[e] = e - ms[e].  End e
// closes a seed iff ms[e] >= min_len and (e == L or start[e + 1] > start[e]): the seeds are the substrings of R of at most
// max_len bases that occur in the text and are contained in no other such substring.
//
//   search  : ONE LANE PER (virtual read, end).  The index is unidirectional, so the sweeps of the sequential algorithms do
//             not apply, and a read is too little work for a wave; every end is a backward search of its own from (0, N)
//             over R[e - 1], R[e - 2], ... that stops at an empty range, a no-base, the read's start or max_len steps.
//             start[] is monotone, so neighbouring lanes run nearly equal trip counts (ms[e] >= ms[e + 1] - 1) and read
//             consecutive bytes at every step.  A step is one or two random 32-byte block gathers (fm_lf2); occupancy hides
//             them.  The reverse complement of a read (virtual read 2 q + 1 with both_strands) is read in place, mirrored.
//             A lane finds its read by a search over read_index: two lanes of the workgroup search the whole batch for the
//             workgroup's first and last end, the others only between those two reads.
//   compact : a lane flags its end from ms[e], ms[e + 1]; the library's exclusive scan over the flags; flagged lanes write
//             their seed; seed_index[v] is the scan value at the first end of virtual read v.
//   locate  : seeds within max_occ: sizes -> scan (pos_index); one lane per position finds its seed by binary search, walks
//             to a sampled row (fm_locate_row, bounded) and writes the sort key (seed << 32 | position); the library's radix
//             sort in the ctx's LMS key arrays, which bound the positions of one call; unpack.
#include "fm_internal.hpp"

#include <vector>

namespace {

constexpr int SD_THREADS = 256;

// control block of a call (u64 words)
enum { SD_BAD = 0, SD_R0 = 1, SD_RQ = 2, SD_LF = 3, SD_MAXMS = 4, SD_LOCATED = 5, SD_POSITIONS = 6, SD_WALKFAIL = 7,
       SD_CHECKSUM = 8, SD_CTL_WORDS = 10 };

// the batch as the kernels see it.  sh = 1 with both strands: the ends of read q are then the 2 L_q ends
// [2 (read_index[q] - r0), 2 (read_index[q + 1] - r0)), the forward read first.
struct SeedBatch {
    const uint8_t *reads;
    const uint64_t *read_index;
    uint64_t Q, r0, bases;
    uint32_t sh;
};

// a read of length zero, an index that decreases or a read too long for the u32 coordinates of a seed; and the two ends of
// read_index for the host
__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_check(const uint64_t *__restrict__ read_index, uint64_t Q,
                                                             unsigned long long *__restrict__ ctl)
{
    const uint64_t q = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    if (q == 0) {
        ctl[SD_R0] = read_index[0];
        ctl[SD_RQ] = read_index[Q];
    }
    if (q < Q) {
        const uint64_t a = read_index[q], b = read_index[q + 1];
        if (b <= a || b - a > 0x7FFFFFFFull) ctl[SD_BAD] = 1;
    }
}

// last q in [lo, hi] with read_index[q] - r0 <= t
__device__ __forceinline__ uint64_t seed_read_at(const SeedBatch &B, uint64_t lo, uint64_t hi, uint64_t t)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (B.read_index[mid] - B.r0 <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the reads of the first and the last end of this workgroup (every lane of the workgroup calls this; one barrier)
__device__ __forceinline__ void seed_block_reads(const SeedBatch &B, uint64_t *s_q)
{
    if (threadIdx.x < 2) {
        uint64_t g = (uint64_t)blockIdx.x * SD_THREADS + (threadIdx.x ? SD_THREADS - 1 : 0);
        if (g >= B.bases) g = B.bases - 1;
        s_q[threadIdx.x] = seed_read_at(B, 0, B.Q - 1, g >> B.sh);
    }
    __syncthreads();
}

struct SeedEnd {
    uint64_t q;      // the read
    uint32_t L, j;   // its length; the end is e = j + 1 of the virtual read
    uint32_t strand; // 1: the reverse complement
};
__device__ __forceinline__ SeedEnd seed_end_of(const SeedBatch &B, const uint64_t *s_q, uint64_t g)
{
    SeedEnd e;
    e.q = seed_read_at(B, s_q[0], s_q[1], g >> B.sh);
    const uint64_t a = B.read_index[e.q];
    e.L = (uint32_t)(B.read_index[e.q + 1] - a);
    const uint64_t off = g - ((a - B.r0) << B.sh);
    e.strand = off >= e.L ? 1u : 0u;
    e.j = (uint32_t)(off - (e.strand ? e.L : 0u));
    return e;
}

__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_ms(FmiD f, SeedBatch B, uint32_t max_len, uint32_t *__restrict__ ms,
                                                          uint2 *__restrict__ rng, unsigned long long *__restrict__ ctl)
{
    __shared__ uint64_t s_q[2];
    seed_block_reads(B, s_q);
    const uint64_t g = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    uint32_t l = 0;
    unsigned long long lf = 0; // (range, base) pairs evaluated
    if (g < B.bases) {
        const SeedEnd e = seed_end_of(B, s_q, g);
        uint32_t cap = e.j + 1;
        if (max_len && max_len < cap) cap = max_len;
        // virtual position i of the reverse complement is byte L - 1 - i of the read, complemented: the walk runs forwards
        const uint8_t *p = B.reads + B.read_index[e.q] + (e.strand ? e.L - 1 - e.j : e.j);
        const int dir = e.strand ? 1 : -1;
        const uint32_t flip = e.strand ? 3u : 0u;
        uint64_t beg = 0, end = f.N;
        while (l < cap) {
            const uint32_t c = *p;
            if (c > 3u) break; // no base
            uint64_t nb = beg, ne = end;
            fm_lf2(f, c ^ flip, nb, ne);
            lf++;
            if (nb >= ne || ne > f.N) break;
            beg = nb;
            end = ne;
            l++;
            p += dir;
        }
        ms[g] = l;
        rng[g] = make_uint2((uint32_t)beg, (uint32_t)end); // the last range that was not empty
    }
    uint32_t mx = l;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lf += __shfl_xor(lf, s, 64);
        const uint32_t o = __shfl_xor(mx, s, 64);
        mx = o > mx ? o : mx;
    }
    if (lane_id() == 0) {
        if (lf) atomicAdd(&ctl[SD_LF], lf);
        if (mx) atomicMax(&ctl[SD_MAXMS], (unsigned long long)mx);
    }
}

// flags[g] = 1 iff end g closes a seed; flags[bases] = 0 (the scan turns it into the total).  Also the totals of the locate:
// seeds within max_occ and their occurrences.
__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_flag(SeedBatch B, uint32_t min_len, uint32_t max_occ,
                                                            const uint32_t *__restrict__ ms, const uint2 *__restrict__ rng,
                                                            uint32_t *__restrict__ flags, unsigned long long *__restrict__ ctl)
{
    __shared__ uint64_t s_q[2];
    seed_block_reads(B, s_q);
    const uint64_t g = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    bool located = false;
    unsigned long long cnt = 0;
    if (g < B.bases) {
        const SeedEnd e = seed_end_of(B, s_q, g);
        const uint32_t m = ms[g];
        // start[e + 1] > start[e]  <=>  ms[e + 1] <= ms[e]
        const bool flag = m >= min_len && (e.j + 1 == e.L || ms[g + 1] <= m);
        flags[g] = flag ? 1u : 0u;
        if (flag) {
            const uint2 r = rng[g];
            located = max_occ == 0 || r.y - r.x <= max_occ;
            cnt = located ? r.y - r.x : 0u;
        }
    } else if (g == B.bases) {
        flags[g] = 0;
    }
    const unsigned long long nl = (unsigned long long)__popcll(__ballot(located));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if (lane_id() == 0) {
        if (nl) atomicAdd(&ctl[SD_LOCATED], nl);
        if (cnt) atomicAdd(&ctl[SD_POSITIONS], cnt);
    }
}

// flagged ends write their seed at the scanned flag; psize (when positions are wanted): occurrences to locate per seed,
// psize[seeds] = 0
__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_compact(SeedBatch B, uint32_t max_occ, const uint32_t *__restrict__ ms,
                                                               const uint2 *__restrict__ rng, const uint32_t *__restrict__ flags,
                                                               const uint32_t *__restrict__ scanned,
                                                               kiss_hip_fmi_seed *__restrict__ seeds, uint64_t *__restrict__ psize)
{
    __shared__ uint64_t s_q[2];
    seed_block_reads(B, s_q);
    const uint64_t g = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    if (g == B.bases && psize) psize[scanned[g]] = 0;
    if (g >= B.bases || !flags[g]) return;
    const SeedEnd e = seed_end_of(B, s_q, g);
    const uint32_t m = ms[g], s = scanned[g];
    const uint2 r = rng[g];
    kiss_hip_fmi_seed out;
    out.start = e.j + 1 - m;
    out.len = m;
    out.sa_beg = r.x;
    out.sa_end = r.y;
    seeds[s] = out;
    if (psize) psize[s] = (max_occ == 0 || r.y - r.x <= max_occ) ? (uint64_t)(r.y - r.x) : 0ull;
}

// seed_index[v] = the scan value at the first end of virtual read v; seed_index[V] = the total
__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_index(SeedBatch B, const uint32_t *__restrict__ scanned,
                                                             uint64_t *__restrict__ seed_index)
{
    const uint64_t v = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x, V = B.Q << B.sh;
    if (v > V) return;
    uint64_t g = B.bases;
    if (v < V) {
        const uint64_t q = v >> B.sh, a = B.read_index[q];
        g = ((a - B.r0) << B.sh) + ((v & B.sh) ? B.read_index[q + 1] - a : 0ull);
    }
    seed_index[v] = scanned[g];
}

// one lane per position: its seed by binary search in pos_index (seeds over max_occ own empty segments), then the bounded
// walk to a sampled row.  A row that finds none is counted and gets position 0xFFFFFFFF.
__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_locate(FmiD f, uint32_t sa_intv, uint64_t sa_entries,
                                                              const kiss_hip_fmi_seed *__restrict__ seeds, uint64_t nseeds,
                                                              const uint64_t *__restrict__ pos_index, uint64_t total, int key_shift,
                                                              uint64_t *__restrict__ keys, unsigned long long *__restrict__ ctl)
{
    const uint64_t h = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    unsigned long long sum = 0;
    bool fail = false;
    if (h < total) {
        uint64_t lo = 0, hi = nseeds; // last seed with pos_index[seed] <= h
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pos_index[mid] <= h) lo = mid;
            else hi = mid;
        }
        const uint64_t row = (uint64_t)seeds[lo].sa_beg + (h - pos_index[lo]);
        uint32_t position;
        fail = !fm_locate_row(f, sa_intv, sa_entries, row, position);
        keys[h] = ((lo << 32) | position) << key_shift;
        if (!fail) sum = position;
    }
    const unsigned long long nf = (unsigned long long)__popcll(__ballot(fail));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if (lane_id() == 0) {
        if (sum) atomicAdd(&ctl[SD_CHECKSUM], sum);
        if (nf) atomicAdd(&ctl[SD_WALKFAIL], nf);
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_fm_seed_unpack(const uint64_t *__restrict__ keys, uint64_t total, int key_shift,
                                                              uint32_t *__restrict__ positions)
{
    const uint64_t i = (uint64_t)blockIdx.x * SD_THREADS + threadIdx.x;
    if (i < total) positions[i] = (uint32_t)(keys[i] >> key_shift);
}

int seed_steps(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
               uint32_t min_len, uint32_t max_len, uint32_t max_occ, int both_strands, uint32_t *ms, kiss_hip_fmi_seed *seeds,
               uint64_t *seed_index, uint64_t seed_capacity, uint32_t *positions, uint64_t *pos_index, uint64_t pos_capacity,
               kiss_hip_fmi_seed_report *rep, FmEvents &ev)
{
    const bool want = positions != nullptr;
    if (Q > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    const uint32_t sa_intv = fmi->sa_intv;
    FmiD f = fm_view_of(fmi);
    const uint64_t sa_entries = (f.N + sa_intv - 1) / sa_intv;
    DevBuf blocks, msbuf, rng, flags, scanned, psize;
    FmCtl<SD_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_SEED_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_fm_seed_check, dim3(fm_grid(Q, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, read_index, Q, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[SD_BAD]) return KISS_HIP_E_INVALID; // a read of length zero, or read_index decreases
    SeedBatch B;
    B.reads = reads;
    B.read_index = read_index;
    B.Q = Q;
    B.r0 = h[SD_R0];
    B.sh = both_strands ? 1u : 0u;
    B.bases = (uint64_t)(h[SD_RQ] - h[SD_R0]) << B.sh;
    const uint64_t bases = B.bases, V = Q << B.sh;
    if (rep) rep->bases = bases;
    // one call: fewer than 2^31 ends, and no more than the ctx scans (about 0.32 x its max_n)
    if (bases > 0x7FFFFFFFull || (bases + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;

    const uint64_t nblocks = f.N / 64 + 1;
    KTRY(blocks.take(ctx, FM_SLOT_BLOCKS, nblocks * 32));
    f.blk = (const uint4 *)blocks.p;
    if (!ms) {
        KTRY(msbuf.take(ctx, FM_SLOT_SEED_MS, (bases + 1) * 4));
        ms = (uint32_t *)msbuf.p;
    }
    KTRY(rng.take(ctx, FM_SLOT_SEED_RANGES, bases * 8));
    KTRY(flags.take(ctx, FM_SLOT_SEED_FLAGS, (bases + 1) * 4));
    KTRY(scanned.take(ctx, FM_SLOT_SEED_SCANNED, (bases + 1) * 4));
    ev.mark(0);
    KTRY(kiss_fm_make_blocks(ctx, f, nblocks, (uint4 *)blocks.p));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, bases);
        ev.mark(1);
        hipLaunchKernelGGL(k_fm_seed_ms, dim3(fm_grid(bases, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, f, B, max_len, ms, (uint2 *)rng.p,
                           d_ctl);
        KCHECK(hipGetLastError());
        ev.mark(2);
        hipLaunchKernelGGL(k_fm_seed_flag, dim3(fm_grid(bases + 1, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, B, min_len, max_occ,
                           (const uint32_t *)ms, (const uint2 *)rng.p, (uint32_t *)flags.p, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u32(ctx, (const uint32_t *)flags.p, (uint32_t *)scanned.p, bases + 1));
    uint32_t nseeds32 = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&nseeds32, (const uint32_t *)scanned.p + bases, 4, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    const uint64_t nseeds = nseeds32, total = h[SD_POSITIONS];
    if (rep) {
        rep->seeds = nseeds;
        rep->located_seeds = h[SD_LOCATED];
        rep->positions = total;
        rep->lf_pairs = h[SD_LF];
        rep->max_ms = (uint32_t)h[SD_MAXMS];
        rep->ms_search = ev.ms(1, 2);
    }
    // (the totals are in the report: the caller's second call)
    if (seed_capacity < nseeds || (want && pos_capacity < total)) return KISS_HIP_E_INVALID;
    if (want && total > ctx->m_cap) return KISS_HIP_E_UNSUPPORTED; // the sort runs in the ctx's LMS key arrays
    if (want) KTRY(psize.take(ctx, FM_SLOT_SEED_POS_SIZE, (nseeds + 1) * 8));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, bases);
        hipLaunchKernelGGL(k_fm_seed_compact, dim3(fm_grid(bases + 1, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, B, max_occ,
                           (const uint32_t *)ms, (const uint2 *)rng.p, (const uint32_t *)flags.p, (const uint32_t *)scanned.p, seeds,
                           (uint64_t *)psize.p);
        hipLaunchKernelGGL(k_fm_seed_index, dim3(fm_grid(V + 1, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, B, (const uint32_t *)scanned.p,
                           seed_index);
        KCHECK(hipGetLastError());
    }
    if (want) KTRY(kiss_scan_u64(ctx, (const uint64_t *)psize.p, pos_index, nseeds + 1));
    ev.mark(3);
    if (rep) rep->ms_compact = 0.f;
    int rc = KISS_HIP_OK;
    if (want && total) {
        const int key_shift = (32 - fm_bits(nseeds, 32, 0)) & ~7; // the sort takes whole bytes from the top of the key
        {
            KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
            hipLaunchKernelGGL(k_fm_seed_locate, dim3(fm_grid(total, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, f, sa_intv, sa_entries,
                               (const kiss_hip_fmi_seed *)seeds, nseeds, (const uint64_t *)pos_index, total, key_shift, ctx->keyA,
                               d_ctl);
            KCHECK(hipGetLastError());
            ev.mark(4);
        }
        RadixBufs rb = kiss_ctx_radix_bufs(ctx); // (a payload nobody reads)
        int res = 0;
        KTRY(kiss_radix_sort(ctx, rb, total, key_shift, 0, &res));
        {
            KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
            hipLaunchKernelGGL(k_fm_seed_unpack, dim3(fm_grid(total, SD_THREADS)), dim3(SD_THREADS), 0, ctx->stream, rb.key[res], total,
                               key_shift, positions);
            KCHECK(hipGetLastError());
        }
        ev.mark(5);
        KTRY(ctl.fetch());
        KTRY(kiss_radix_check(ctx)); // (synchronises)
        if (rep) {
            rep->walk_failures = h[SD_WALKFAIL];
            rep->checksum = h[SD_CHECKSUM];
            rep->ms_locate = ev.ms(3, 4);
            rep->ms_sort = ev.ms(4, 5);
        }
        if (h[SD_WALKFAIL]) rc = KISS_HIP_E_INVALID; // not an index of an exact suffix array: positions are not defined
    } else {
        KCHECK(hipStreamSynchronize(ctx->stream));
    }
    if (rep) rep->ms_compact = ev.ms(2, 3); // flags, scans, one look at the totals from the host, compaction
    return rc;
}

int seed_args_check(const kiss_hip_fmi_view_ex *fmi, bool host, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                    uint32_t min_len, const kiss_hip_fmi_seed *seeds, const uint64_t *seed_index, const uint32_t *positions,
                    const uint64_t *pos_index, uint64_t pos_capacity)
{
    if (!fmi) return KISS_HIP_E_INVALID;
    const kiss_hip_fmi_view &v = fmi->base;
    if (!fm_sa_intv_ok(v.sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    const bool any = positions || pos_index, all = positions && pos_index;
    if (min_len == 0 || v.n_sa == 0 || !v.bwt || !v.occ1 || !v.occ2 || !seed_index || (Q && (!reads || !read_index || !seeds)) ||
        any != all || (!any && pos_capacity))
        return KISS_HIP_E_INVALID;
    if ((all || host) && (!v.sa || (v.sa_intv != 1 && (!v.b || !v.b_occ)))) return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_seeds_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view_ex *fmi, const uint8_t *reads, const uint64_t *read_index,
                           uint64_t Q, uint32_t min_len, uint32_t max_len, uint32_t max_occ, int both_strands, uint32_t *ms,
                           kiss_hip_fmi_seed *seeds, uint64_t *seed_index, uint64_t seed_capacity, uint32_t *positions,
                           uint64_t *pos_index, uint64_t pos_capacity, kiss_hip_fmi_seed_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_fmi_seed_report{};
        report->Q = Q;
        report->V = both_strands ? 2 * Q : Q;
    }
    KTRY(seed_args_check(fmi, false, reads, read_index, Q, min_len, seeds, seed_index, positions, pos_index, pos_capacity));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) { // seed_index[0] = pos_index[0] = 0
        KTRY(kiss_zero_u32(ctx, seed_index, 2));
        if (pos_index) KTRY(kiss_zero_u32(ctx, pos_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    FmEvents ev(ctx, report != nullptr);
    const int rc = seed_steps(ctx, &fmi->base, reads, read_index, Q, min_len, max_len, max_occ, both_strands, ms, seeds, seed_index,
                              seed_capacity, positions, pos_index, pos_capacity, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_seeds_host(const kiss_hip_fmi_view_ex *fmi, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            uint32_t min_len, uint32_t max_len, uint32_t max_occ, int both_strands, uint32_t *ms,
                            kiss_hip_fmi_seed *seeds, uint64_t *seed_index, uint64_t seed_capacity, uint32_t *positions,
                            uint64_t *pos_index, uint64_t pos_capacity, kiss_hip_fmi_seed_report *report, int device)
{
    if (report) {
        *report = kiss_hip_fmi_seed_report{};
        report->Q = Q;
        report->V = both_strands ? 2 * Q : Q;
    }
    KTRY(seed_args_check(fmi, true, reads, read_index, Q, min_len, seeds, seed_index, positions, pos_index, pos_capacity));
    if (!fm_index_ascending(read_index, Q, true)) return KISS_HIP_E_INVALID;
    const kiss_hip_fmi_view &hv = fmi->base;
    const uint32_t sa_intv = hv.sa_intv;
    const bool all = positions != nullptr;
    kiss_hip_fmi_sizes_ex z;
    KTRY(kiss_hip_fmi_sizes_ex_for(hv.n_sa - 1, sa_intv, 0, &z));
    const uint64_t r0 = Q ? read_index[0] : 0, read_bytes = Q ? read_index[Q] - r0 : 0;
    const uint64_t V = both_strands ? 2 * Q : Q, bases = both_strands ? 2 * read_bytes : read_bytes;
    if (seed_capacity > bases) seed_capacity = bases; // (always enough)
    std::vector<uint64_t> ridx(Q + 1, 0); // (the reads are copied from read_index[0] on)
    if (Q)
        for (uint64_t q = 0; q <= Q; q++) ridx[q] = read_index[q] - r0;
    // (the ends of a call are scanned in the ctx's scratch, its positions sorted in the LMS arrays)
    return kiss_one_shot_own(device, fm_host_max_n(hv.n_sa, bases + 1, pos_capacity), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        kiss_hip_fmi_view_ex v = *fmi;
        v.base = fm_upload_index(st, hv, z.base);
        v.lookup = nullptr; // (the search does not use it)
        const uint8_t *dreads = st.up(reads ? reads + r0 : nullptr, read_bytes);
        const uint64_t *dridx = st.up(ridx.data(), (Q + 1) * 8);
        uint32_t *dms = st.room<uint32_t>(ms != nullptr, bases * 4);
        kiss_hip_fmi_seed *dseeds = st.room<kiss_hip_fmi_seed>(true, seed_capacity * 16);
        uint64_t *dsidx = st.room<uint64_t>(true, (V + 1) * 8);
        uint32_t *dpos = st.room<uint32_t>(all, pos_capacity * 4);
        uint64_t *dpidx = st.room<uint64_t>(all, (seed_capacity + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_fmi_seed_report r{};
        const int rc = kiss_hip_fmi_seeds_dev(ctx, &v, dreads, dridx, Q, min_len, max_len, max_occ, both_strands, dms, dseeds, dsidx,
                                              seed_capacity, dpos, dpidx, all ? pos_capacity : 0, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(seed_index, dsidx, (V + 1) * 8);
        st.down(seeds, dseeds, r.seeds * 16);
        if (ms) st.down(ms, dms, bases * 4);
        if (all) st.down(pos_index, dpidx, (r.seeds + 1) * 8);
        if (all) st.down(positions, dpos, r.positions * 4);
        return st.rc;
    });
}

} // extern "C"
