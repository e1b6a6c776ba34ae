// doubling.hip -- exact order by rank doubling, in two forms: over the suffix array after the induction (kiss_exact_refine)
// and over the LMS suffixes before it (kiss_lms_exact_refine, the form that runs; the other one is its fall-back and the
// finish of the general alphabet).  Both work on the tied-segment arrays of the LMS sort (lms_sort.hip) and open and close
// a round with the flag + compaction of flag_compact.hip; what the two rounds share is in the helpers in front of
// kiss_exact_refine.
#include "flag_compact.hpp"
#include <cstdio>
#include <ctime>
#include <utility>
#include <vector>

using namespace kiss_fc;

// =============================================================================================================
// Exact order by prefix doubling (the KISS2 / PREFIX_DOUBLING path, reference kiss2_core.hpp:728-797: sort,
// re-rank, compact, double).  The reference doubles over an encoded LMS string; here the doubling runs over
// the full suffix array, which 288 GB of HBM affords and which needs no sampled-rank bookkeeping:
//   1. the k-ordered pipeline has produced SA ordered by the first h0 bases (ties in arbitrary order);
//   2. group heads: SA[i] starts a group unless it shares h0 bases with SA[i-1]          (k_group_heads)
//   3. ISA[SA[i]] = i, then for tied suffixes the slot of their group head                 (k_isa_init/update)
//   4. rounds h = h0, 2*h0, ...: every tied suffix p fetches ISA[p + h], groups are radix sorted on
//      (group, rank), split where neighbours differ; singletons retire to SA, the rest get new ranks.
// Only the *result* (the unique suffix array) is comparable with the reference; the number of rounds is
// O(log(longest repeat / h0)) instead of the MSD path's O(longest repeat / 32).
// =============================================================================================================
namespace {

constexpr uint32_t SMALL_SEG = 64; // groups of up to this many members sort themselves inside a wave's reach

// cw (optional): the context words the induction left parallel to SA.  Only their taint bit is looked at: a suffix that
// does not descend from an LMS suffix the bounded-depth sort may have misplaced is where it belongs and starts a group of
// its own -- no text is read for it (at chm13 size 94 % of the 3.1 G entries; this kernel was 69 ms of random reads).
__global__ __launch_bounds__(LS_THREADS) void k_group_heads(const uint64_t *__restrict__ pk, uint64_t n,
                                                           const uint32_t *__restrict__ SA, uint64_t count, uint32_t h0,
                                                           const uint32_t *__restrict__ cw, uint8_t *__restrict__ heads,
                                                           uint32_t lo) // first entry that can be tied (SA: 1, SA[0] = n)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    const bool valid = i < count;
    const uint64_t p = valid ? SA[i] : 0;
    const bool tainted = valid && i >= lo && (!cw || (cw[i] & KISS_CTX_TAINT) != 0); // SA[0] = n has no context word
    const bool pfull = tainted && p + h0 <= n;
    const uint64_t kp = pfull ? kiss_key32(pk, p) : 0ull; // h0 >= 32
    // predecessor's first word: from the neighbouring lane, lane 0 loads it
    uint64_t q = __shfl_up(p, 1, 64);
    uint64_t kq = __shfl_up(kp, 1, 64);
    bool qfull = __shfl_up((int)pfull, 1, 64) != 0;
    if (lane_id() == 0 && pfull && i > lo) {
        q = SA[i - 1];
        qfull = q + h0 <= n && (!cw || (cw[i - 1] & KISS_CTX_TAINT) != 0);
        kq = qfull ? kiss_key32(pk, q) : 0ull;
    } else if (lane_id() == 0) {
        qfull = false;
    }
    if (!valid) return;
    uint8_t head = 1;
    if (i > 0 && pfull && qfull && kp == kq) {
        head = 0;
        uint32_t d = 32;
        // 128 bases per step while that much is left (five independent word loads per suffix and step: tainted
        // neighbours mostly ARE tied, so the walk usually runs the whole h0 bases)
        for (; d + 128 <= h0 && !head; d += 128) {
            uint64_t a[4], b[4];
            keys128(pk, p + d, a);
            keys128(pk, q + d, b);
            if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3]) head = 1;
        }
        if (d < h0 && !head && h0 >= 160) { // the rest as ONE step that ends at h0 (it overlaps what has been compared)
            uint64_t a[4], b[4];
            keys128(pk, p + h0 - 128, a);
            keys128(pk, q + h0 - 128, b);
            if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3]) head = 1;
            d = h0;
        }
        for (; d < h0 && !head; d += 32) {
            uint64_t a = kiss_key32(pk, p + d), b = kiss_key32(pk, q + d);
            if (h0 - d < 32) {
                const uint64_t mask = ~0ull << (64 - 2 * (h0 - d));
                a &= mask;
                b &= mask;
            }
            if (a != b) head = 1;
        }
    }
    heads[i] = head;
}

// ---- group heads in two steps (the form used when the context words with their taint bits are at hand) ---------------
// Only 5 % of the suffix-array entries of a genome are tainted; walked inside the one-lane-per-entry kernel above they
// leave 61 of 64 lanes of nearly every wave waiting for three dependent random reads (29 ms at chm13 size, all latency).
// Step 1 streams SA and the context words once: heads[i] = 1 for every entry that can not be tied with its
// predecessor, and the indexes of the candidates (both tainted, both with h0 bases left) are appended to a list, one
// atomic per workgroup -- spread over GH_REGIONS counters, each with its own slice of the list: three million adds to ONE
// address take 36 ms, which is more than the kernel they were meant to speed up.  Step 2 compares the candidates' h0
// bases with every lane busy.
constexpr int GH_THREADS = 1024;
constexpr int GH_ITEMS = 4;
constexpr int GH_REGIONS = 256;
__global__ __launch_bounds__(GH_THREADS) void k_heads_candidates(const uint32_t *__restrict__ SA, uint64_t count, uint64_t n,
                                                                uint32_t h0, const uint32_t *__restrict__ cw,
                                                                uint8_t *__restrict__ heads, uint32_t *__restrict__ list,
                                                                uint64_t region_cap, uint32_t *__restrict__ ncand,
                                                                uint32_t lo) // first entry that can be tied (SA: 1)
{
    __shared__ uint32_t wcount[GH_THREADS / 64];
    __shared__ uint32_t s_base;
    const uint32_t region = blockIdx.x % GH_REGIONS;
    const uint64_t i0 = ((uint64_t)blockIdx.x * GH_THREADS + threadIdx.x) * GH_ITEMS;
    uint32_t cm = 0; // bit e: entry i0 + e is a candidate
    if (i0 + GH_ITEMS <= count) { // four context words per load, four flag bytes per store
        const uint4 c4 = *reinterpret_cast<const uint4 *>(cw + i0);
        const uint32_t prev = i0 > 0 ? cw[i0 - 1] : 0u;
        const uint32_t t = (c4.x >> 31) | ((c4.y >> 31) << 1) | ((c4.z >> 31) << 2) | ((c4.w >> 31) << 3);
        cm = t & ((t << 1) | (prev >> 31)) & 0xFu;
#pragma unroll
        for (int e = 0; e < GH_ITEMS; e++)
            if (i0 + (uint64_t)e <= lo) cm &= ~(1u << e);
        if (cm) {
#pragma unroll
            for (int e = 0; e < GH_ITEMS; e++)
                if ((cm >> e) & 1u) {
                    const uint64_t p = SA[i0 + e], q = SA[i0 + e - 1];
                    if (!(p + h0 <= n && q + h0 <= n)) cm &= ~(1u << e);
                }
        }
        *reinterpret_cast<uint32_t *>(heads + i0) = 0x01010101u; // candidates that turn out tied are reset by k_heads_compare
    } else {
        for (int e = 0; e < GH_ITEMS; e++) {
            const uint64_t i = i0 + (uint64_t)e;
            if (i >= count) break;
            if (i > lo && (cw[i] & KISS_CTX_TAINT) && (cw[i - 1] & KISS_CTX_TAINT)) {
                const uint64_t p = SA[i], q = SA[i - 1];
                if (p + h0 <= n && q + h0 <= n) cm |= 1u << e;
            }
            heads[i] = 1;
        }
    }
    const uint32_t c = (uint32_t)__popc(cm);
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if ((int)lane_id() >= d) inc += o;
    }
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 63) wcount[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < GH_THREADS / 64; w++) {
            const uint32_t cc = wcount[w];
            wcount[w] = t;
            t += cc;
        }
        s_base = t ? atomicAdd(&ncand[region], t) : 0u;
    }
    __syncthreads();
    if (cm) {
        uint64_t at = (uint64_t)s_base + wcount[wave] + (inc - c);
#pragma unroll
        for (int e = 0; e < GH_ITEMS; e++)
            if ((cm >> e) & 1u) {
                if (at < region_cap) list[(uint64_t)region * region_cap + at] = (uint32_t)(i0 + e); // (an overflow shows in the counter)
                at++;
            }
    }
}

__global__ __launch_bounds__(LS_THREADS) void k_heads_compare(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ SA,
                                                             const uint32_t *__restrict__ list, uint64_t region_cap,
                                                             const uint32_t *__restrict__ ncand, uint32_t h0,
                                                             uint8_t *__restrict__ heads)
{
    const uint64_t j = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x; // blockIdx.y = region
    if (j >= ncand[blockIdx.y]) return;
    const uint32_t i = list[(uint64_t)blockIdx.y * region_cap + j];
    const uint64_t p = SA[i], q = SA[i - 1];
    bool differ = false;
    uint32_t d = 0;
    for (; d + 128 <= h0 && !differ; d += 128) {
        uint64_t a[4], b[4];
        keys128(pk, p + d, a);
        keys128(pk, q + d, b);
        differ = a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3];
    }
    for (; d < h0 && !differ; d += 32) {
        uint64_t a = kiss_key32(pk, p + d), b = kiss_key32(pk, q + d);
        if (h0 - d < 32) {
            const uint64_t mask = ~0ull << (64 - 2 * (h0 - d));
            a &= mask;
            b &= mask;
        }
        differ = a != b;
    }
    if (!differ) heads[i] = 0;
}

// debug: number of tainted context words
__global__ __launch_bounds__(LS_THREADS) void k_count_taint(const uint32_t *__restrict__ cw, uint64_t count,
                                                           unsigned long long *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    const uint64_t m = __ballot(i > 0 && i < count && (cw[i] & KISS_CTX_TAINT));
    if (lane_id() == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(LS_THREADS) void k_isa_init(const uint32_t *__restrict__ SA, uint64_t count,
                                                        uint32_t *__restrict__ isa)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i < count) isa[SA[i]] = (uint32_t)i;
}

// rank of a tied suffix = slot of the first member of its group
// (also reports the longest group: *maxlen, zeroed by the caller; segstart[nseg] = count)
__global__ __launch_bounds__(LS_THREADS) void k_isa_update(const uint32_t *__restrict__ pos,
                                                          const uint32_t *__restrict__ slot,
                                                          const uint32_t *__restrict__ seg,
                                                          const uint32_t *__restrict__ segstart, uint64_t count,
                                                          uint32_t *__restrict__ isa, uint32_t *__restrict__ maxlen,
                                                          int shift) // isa is indexed by position >> shift
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    uint32_t len = 0;
    if (i < count) {
        const uint32_t sg = seg[i];
        const uint32_t a = segstart[sg];
        isa[pos[i] >> shift] = slot[a];
        if ((uint32_t)i == a) len = segstart[sg + 1] - a;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(len, d, 64);
        len = o > len ? o : len;
    }
    if (lane_id() == 0 && len > 64) atomicMax(maxlen, len); // only groups past the in-wave sort size matter
}

// groups of <= 64 members: every member ranks itself inside its group on (key, index) and moves there;
// the group ids stay where they are (all members of a group carry the same one)
__global__ __launch_bounds__(LS_THREADS) void k_group_sort_small(const uint64_t *__restrict__ key,
                                                                const uint32_t *__restrict__ pos,
                                                                const uint32_t *__restrict__ seg,
                                                                const uint32_t *__restrict__ segstart, uint64_t count,
                                                                uint64_t *__restrict__ okey, uint32_t *__restrict__ opos,
                                                                uint64_t *__restrict__ big)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t sg = seg[i];
    const uint32_t a = segstart[sg], b = segstart[sg + 1];
    if (big) { // longer groups exist: flag their members for the radix path, (1 << 32) | starts-a-group
        const bool isbig = b - a > SMALL_SEG;
        big[i] = isbig ? ((1ull << 32) | (uint64_t)((uint32_t)i == a ? 1u : 0u)) : 0ull;
        if (isbig) return;
    }
    const uint64_t ki = key[i];
    uint32_t r = 0;
    for (uint32_t j = a; j < b; j++) {
        const uint64_t kj = key[j];
        r += (kj < ki || (kj == ki && j < (uint32_t)i)) ? 1u : 0u;
    }
    okey[a + r] = ki;
    opos[a + r] = pos[i];
}

__global__ __launch_bounds__(LS_THREADS) void k_gather_ranks(const uint32_t *__restrict__ isa,
                                                            const uint32_t *__restrict__ pos, uint64_t count, uint64_t h,
                                                            uint64_t n, uint64_t *__restrict__ key)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    uint64_t q = (uint64_t)pos[i] + h;
    if (q > n) q = n; // cannot happen for a tied suffix (it shares h bases with another one); isa[n] = 0
    key[i] = (uint64_t)isa[q] << 32;
}

} // namespace

// ---- what the two forms share --------------------------------------------------------------------------------------------
namespace {

// the tied suffixes of a round -- positions, slots (where they go in the list), group ids, group starts (+ end entry)
struct TiedSet {
    uint32_t *P, *S, *G, *SS;
    FcOut out() const { return FcOut{P, S, G, SS}; }
};
// ... and the arrays the next round's go to.  (Taken from the ctx after make_room_for_tied: a regrowth moves the arrays.)
struct TiedBufs {
    TiedSet cur, next;
    explicit TiedBufs(kiss_hip_ctx *ctx)
        : cur{ctx->posA, ctx->slotA, ctx->segA, ctx->segstartA}, next{ctx->posB, ctx->slotB, ctx->segB, ctx->segstartB}
    {
    }
    void swap() { std::swap(cur, next); }
};

// the list a form refines and the rank array it keeps
struct Doubling {
    uint32_t *list;        // the suffix array, or the merged LMS list: a suffix that retires is written to its slot
    uint64_t len;
    const uint8_t *heads;  // one byte per list entry, 0 = tied with its predecessor
    uint32_t *rank;        // rank[position >> rank_shift] = slot; a tied suffix carries the slot of its group's first member
    int rank_shift;
    uint32_t *cfix;        // optional: context words parallel to the list, rewritten for the suffixes that retire
    bool grow_lms;         // the LMS-sized work arrays are dead and may be regrown with the tied-segment arrays
    uint64_t *d_total;
    uint32_t *d_maxlen;    // longest group past SMALL_SEG, as k_isa_update leaves it
    unsigned sync_points;  // hooks build (KISS_HIP_LX_SYNC_POINTS): bit i set = the host waits for the stream at point i of a
                           // round: 0 groups sorted, 2 / 3 / 4 inside sort_big_members, 5 before the closing compaction
};

void sync_point(kiss_hip_ctx *ctx, const Doubling &d, unsigned i)
{
    if ((d.sync_points >> i) & 1u) (void)hipStreamSynchronize(ctx->stream);
}

// Tie flags by comparison: heads[i] = 0 where list[i] and list[i - 1] are both tainted (cw) and equal on their first h0
// bases.  Candidates first, compared densely afterwards; the candidate list lives in posA (dead here).  More candidates than
// it holds (texts that are one repeat), or no context words (cw == null: compare every neighbour pair): the one-kernel form
// does the whole job.  lo: the first entry that can be tied (the suffix array: 1, SA[0] = n; an LMS list: 0).
int heads_by_compare(kiss_hip_ctx *ctx, const uint32_t *list, uint64_t len, uint64_t n, uint32_t h0, const uint32_t *cw,
                     uint8_t *heads, uint32_t lo)
{
    const unsigned T = LS_THREADS;
    if (cw) {
        uint32_t *d_nc = ctx->rx_ghist; // GH_REGIONS counters (digit-histogram scratch of the radix sort, 3072 words, dead here)
        const uint64_t region_cap = ctx->m_cap / GH_REGIONS;
        KTRY(kiss_zero_u32(ctx, d_nc, GH_REGIONS));
        hipLaunchKernelGGL(k_heads_candidates, dim3((unsigned)div_up(len, GH_THREADS * GH_ITEMS)), dim3(GH_THREADS), 0, ctx->stream,
                           list, len, n, h0, cw, heads, ctx->posA, region_cap, d_nc, lo);
        uint32_t h_nc[GH_REGIONS];
        KCHECK(hipMemcpyAsync(h_nc, d_nc, sizeof h_nc, hipMemcpyDeviceToHost, ctx->stream));
        KCHECK(hipStreamSynchronize(ctx->stream));
        uint32_t mx = 0;
        for (uint32_t v : h_nc) mx = v > mx ? v : mx;
        if (mx <= region_cap) {
            if (mx)
                hipLaunchKernelGGL(k_heads_compare, dim3((unsigned)div_up((uint64_t)mx, T), GH_REGIONS), dim3(T), 0, ctx->stream,
                                   ctx->pk, list, ctx->posA, region_cap, d_nc, h0, heads);
            return KISS_HIP_OK;
        }
    }
    hipLaunchKernelGGL(k_group_heads, dim3((unsigned)div_up(len, T)), dim3(T), 0, ctx->stream, ctx->pk, n, list, len, h0, cw, heads, lo);
    return KISS_HIP_OK;
}

FcJob heads_job(const Doubling &d)
{
    FcJob job;
    job.src = FC_HEADS;
    job.key = reinterpret_cast<const uint64_t *>(d.heads);
    job.pos = d.list;
    job.count = d.len;
    return job;
}

// how many list entries are tied, in how many groups
int count_tied(kiss_hip_ctx *ctx, const Doubling &d, uint64_t *count, uint64_t *nseg)
{
    uint64_t tot;
    KTRY(fc_count(ctx, heads_job(d), d.d_total));
    KTRY(read_u64(ctx, d.d_total, &tot));
    *count = tot >> 32;
    *nseg = tot & 0xFFFFFFFFull;
    return KISS_HIP_OK;
}

// ranks of the tied suffixes of `t`: the slot of their group's first member
int rerank(kiss_hip_ctx *ctx, const Doubling &d, const TiedSet &t, uint64_t count, uint64_t nseg)
{
    KTimer timer(ctx, KISS_HIP_K_ISA, count);
    set_u32(ctx, t.SS + nseg, (uint32_t)count, d.d_maxlen);
    hipLaunchKernelGGL(k_isa_update, dim3((unsigned)div_up(count, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, t.P, t.S, t.G, t.SS,
                       count, d.rank, d.d_maxlen, d.rank_shift);
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}

// Behind count_tied: the tied-segment arrays regrown if they hold fewer than the `count` tied entries (their contents are
// dead), and the tile offsets counted again, which were in them
int make_room_for_tied(kiss_hip_ctx *ctx, const Doubling &d, uint64_t count)
{
    const bool grow_lms = d.grow_lms && count > ctx->m_cap; // (both sets of arrays in one go; keeps CTX, pk)
    if (!grow_lms && count <= ctx->t_cap) return KISS_HIP_OK;
    const uint64_t want = count + count / 64 + 1024;
    if (grow_lms) KTRY(kiss_lms_reserve(ctx, want, want));
    if (count > ctx->t_cap) KTRY(kiss_tied_reserve(ctx, want));
    return fc_count(ctx, heads_job(d), d.d_total);
}

// Opens the rounds: the `count` tied entries in `nseg` groups go to the tied-segment arrays and get their ranks
int compact_tied_from_heads(kiss_hip_ctx *ctx, const Doubling &d, uint64_t count, uint64_t nseg, const TiedSet &to)
{
    KTRY(fc_compact(ctx, heads_job(d), to.out()));
    return rerank(ctx, d, to, count, nseg);
}

// Groups of <= SMALL_SEG have sorted themselves into bkeyB / bposB and flagged the members of longer ones (ctx->flags[i] =
// (1 << 32) | starts-a-group): those members are pulled out, radix sorted on (group, rank) and put back --
// sorted keys in bkeyB, positions in bposB, group ids unchanged.  pbuf: two position buffers for the sort.
int sort_long_groups(kiss_hip_ctx *ctx, const Doubling &d, const uint32_t *P, uint64_t count, uint32_t *pbuf0, uint32_t *pbuf1)
{
    uint64_t *F1 = ctx->flags, *F2 = ctx->flags + ctx->t_cap;
    uint64_t bt;
    KTRY(flags_total(ctx, F1, F2, count, d.d_total, &bt));
    BigSort b;
    b.key = ctx->bkeyA;
    b.pos = P;
    b.count = count;
    b.flags = F1;
    b.ex = F2;
    b.nbig = bt >> 32;
    b.ngroups = bt & 0xFFFFFFFFull;
    b.key_lo_bit = 32;
    b.kbuf[0] = ctx->keyA;
    b.kbuf[1] = ctx->keyB;
    b.pbuf[0] = pbuf0;
    b.pbuf[1] = pbuf1;
    b.sbuf[0] = ctx->bsegA;
    b.sbuf[1] = ctx->bsegB;
    b.bidx = ctx->bposA;
    b.okey = ctx->bkeyB;
    b.opos = ctx->bposB;
    b.sync_points = d.sync_points;
    if (!b.nbig) return KISS_HIP_OK; // (the LMS form: the long groups are all stuck ones, which are not sorted on keys)
    ctx->stats.big_item_rounds += b.nbig;
    return sort_big_members(ctx, b);
}

// Closes a round: the groups are sorted on their keys (bkeyB, positions in bposB).  Split where (key, group) changes:
// singletons retire into the list and the rank array, the rest are compacted into the other buffer set (slots stay in
// index order), which becomes the current one, and get their new ranks.  d_abort (optional): a device word that, if set,
// ends the doubling as soon as the totals are read -- *why gets it, and the round is left as it is.
int finish_round(kiss_hip_ctx *ctx, const Doubling &d, TiedBufs &bufs, uint64_t *count, uint64_t *nseg,
                 const uint32_t *d_abort = nullptr, uint32_t *why = nullptr)
{
    FcJob job;
    job.src = FC_KEY_SEG;
    job.key = ctx->bkeyB;
    job.seg = bufs.cur.G;
    job.pos = ctx->bposB;
    job.slot = bufs.cur.S;
    job.count = *count;
    job.cmp_shift = 32;
    job.out = d.list;
    job.isa = d.rank;
    job.isa_shift = d.rank_shift;
    job.cfix = d.cfix; // (the list entry a suffix replaces was another suffix's: it takes the context word of its own position along)
    ctx->stats.doubling_rounds++;
    ctx->stats.sort_item_rounds += *count;
    KTRY(fc_count(ctx, job, d.d_total));
    sync_point(ctx, d, 5);
    KTRY(fc_compact(ctx, job, bufs.next.out())); // (queued before the host waits for the totals)
    uint64_t tot;
    KTRY(read_u64(ctx, d.d_total, &tot));
    if (d_abort) {
        KTRY(kiss_readback(ctx, d_abort, 1));
        if ((*why = ctx->h_pinned[0])) return KISS_HIP_OK;
    }
    bufs.swap();
    *count = tot >> 32;
    *nseg = tot & 0xFFFFFFFFull;
    return *count ? rerank(ctx, d, bufs.cur, *count, *nseg) : KISS_HIP_OK;
}

// the byte per suffix-array entry kiss_exact_refine flags ties in, kept by the ctx between calls (sized for max_n)
int refine_heads_buffer(kiss_hip_ctx *ctx, uint8_t **heads)
{
    if (!ctx->refine_heads) {
        const uint64_t cap = ctx->max_n + 2;
        hipError_t e = hipMalloc((void **)&ctx->refine_heads, cap);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ctx->refine_heads = nullptr;
            ctx->last_hip_error = (int)e;
            return KISS_HIP_E_NOMEM;
        }
        ctx->ws_bytes += cap;
    }
    *heads = ctx->refine_heads;
    return KISS_HIP_OK;
}

// KISS_HIP_DEBUG: how many suffix-array entries carry a taint bit
int report_taint(kiss_hip_ctx *ctx, uint64_t total)
{
    unsigned long long *dc = (unsigned long long *)(ctx->d_small + 44), hc = 0;
    KTRY(kiss_zero_u32(ctx, dc, 2));
    hipLaunchKernelGGL(k_count_taint, dim3((unsigned)div_up(total, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, ctx->CTX, total, dc);
    KCHECK(hipMemcpyAsync(&hc, dc, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[kiss_hip] refine: %llu of %llu suffix-array entries are tainted\n", hc, (unsigned long long)total);
    return KISS_HIP_OK;
}

// the rounds of kiss_exact_refine: h = h0, 2 h0, ... until nothing is tied
int doubling_rounds_sa(kiss_hip_ctx *ctx, const Doubling &d, TiedBufs &bufs, uint64_t n, uint32_t h0, uint64_t count, uint64_t nseg)
{
    const bool dbg = ctx->opts.debug;
    for (uint64_t h = h0; count > 0; h *= 2) {
        if (h > 2 * n + 64) return KINTERNAL();
        const unsigned grid = (unsigned)div_up(count, LS_THREADS);
        {
            KTimer t(ctx, KISS_HIP_K_KEYGATHER, count);
            hipLaunchKernelGGL(k_gather_ranks, dim3(grid), dim3(LS_THREADS), 0, ctx->stream, d.rank, bufs.cur.P, count, h, n, ctx->bkeyA);
        }
        uint64_t ml;
        KTRY(read_u64(ctx, d.d_maxlen, &ml)); // longest group (0: none longer than 64)
        const uint32_t maxlen = (uint32_t)ml;
        {
            KTimer t(ctx, KISS_HIP_K_SEGRANK, count);
            hipLaunchKernelGGL(k_group_sort_small, dim3(grid), dim3(LS_THREADS), 0, ctx->stream, ctx->bkeyA, bufs.cur.P, bufs.cur.G,
                               bufs.cur.SS, count, ctx->bkeyB, ctx->bposB, maxlen > SMALL_SEG ? ctx->flags : nullptr);
        }
        if (maxlen > SMALL_SEG) KTRY(sort_long_groups(ctx, d, bufs.cur.P, count, ctx->lmsP, ctx->lmsC));
        const uint64_t before = count;
        KTRY(finish_round(ctx, d, bufs, &count, &nseg));
        if (dbg)
            fprintf(stderr, "[kiss_hip] refine h=%llu: (host clock %.3f s) items %llu (longest group %s%u) -> %llu in %llu groups\n",
                    (unsigned long long)h, (double)clock() / CLOCKS_PER_SEC, (unsigned long long)before, maxlen ? "" : "<= ",
                    maxlen ? maxlen : 64u, (unsigned long long)count, (unsigned long long)nseg);
    }
    return KISS_HIP_OK;
}

// tie flags, the tied entries compacted and ranked, the rounds
int exact_refine_steps(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, uint32_t *d_SA, uint8_t *heads, bool heads_given)
{
    const uint64_t total = n + 1;
    const bool dbg = ctx->opts.debug;
    if (!heads_given) {
        KTimer t(ctx, KISS_HIP_K_GROUP_HEADS, total);
        if (dbg && ctx->ctx_words_valid) KTRY(report_taint(ctx, total));
        // the context words are still in CTX (it becomes the inverse suffix array only after this step)
        // (hooks build, KISS_HIP_NO_TAINT: compare every neighbour pair)
        const uint32_t *cw = (!ctx->opts.no_taint && ctx->ctx_words_valid) ? ctx->CTX : (const uint32_t *)nullptr;
        KTRY(heads_by_compare(ctx, d_SA, total, n, h0, cw, heads, 1u));
    }
    Doubling d;
    d.list = d_SA;
    d.len = total;
    d.heads = heads;
    d.rank = ctx->CTX; // the induction's context words are dead by now: (n + 2) u32
    d.rank_shift = 0;
    d.cfix = nullptr;
    d.grow_lms = true;
    d.d_total = (uint64_t *)(ctx->d_small + 2);
    d.d_maxlen = ctx->d_small + 8;
    d.sync_points = 0;
    uint64_t count, nseg;
    KTRY(count_tied(ctx, d, &count, &nseg));
    ctx->stats.refine_items = count;
    if (dbg)
        fprintf(stderr, "[kiss_hip] refine: %llu of %llu suffixes tied at depth %u in %llu groups\n", (unsigned long long)count,
                (unsigned long long)total, h0, (unsigned long long)nseg);
    if (count == 0) return KISS_HIP_OK;
    ctx->ctx_words_valid = false; // CTX becomes the inverse suffix array from here on
    // the inverse suffix array is only needed when something is tied
    if (ctx->opts.isa_direct) { // (hooks build: the plain random scatter)
        KTimer t(ctx, KISS_HIP_K_ISA, total);
        hipLaunchKernelGGL(k_isa_init, dim3((unsigned)div_up(total, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, d_SA, total, d.rank);
    } else
        KTRY(kiss_isa_build(ctx, d_SA, total, d.rank));
    KTRY(make_room_for_tied(ctx, d, count));
    TiedBufs bufs(ctx);
    KTRY(compact_tied_from_heads(ctx, d, count, nseg, bufs.cur));
    return doubling_rounds_sa(ctx, d, bufs, n, h0, count, nseg);
}

} // namespace

int kiss_exact_refine(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, uint32_t *d_SA, uint8_t *heads_in)
{
    // heads_in == nullptr: DNA, SA ordered by h0 >= 32 bases, ties found by comparing the packed text;
    // heads_in != nullptr: the caller knows the groups already (general alphabet: equal 7-character keys)
    if ((!heads_in && h0 < 32) || h0 == 0 || n < h0) return KINTERNAL();
    ctx->stats.refine_form = 2;
    KTRY(kiss_need_ctx_words(ctx));
    uint8_t *heads = heads_in;
    if (!heads) KTRY(refine_heads_buffer(ctx, &heads));
    int rc = exact_refine_steps(ctx, n, h0, d_SA, heads, heads_in != nullptr);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc == KISS_HIP_OK && e != hipSuccess) {
        ctx->last_hip_error = (int)e;
        rc = KISS_HIP_E_HIP;
    }
    return rc;
}

// =====================================================================================================================
// Exact order at the LMS level (round 3): the doubling runs BEFORE the induction, over the LMS suffixes alone.
//
// The reference's KISS2 does the same thing in its own way (`kiss2_core.hpp:835-886`: exact order of the LMS suffixes by
// prefix doubling over an encoded LMS string, then ONE induction).  Here the h0-ordered merged LMS list L (ctx->lmsP, all
// m LMS suffixes, ties in position order, the tied ones tainted) is refined in place:
//   * rank[p >> 1] = slot of p in L (LMS positions are never neighbours, so p >> 1 is collision-free; tied suffixes carry the
//     slot of their group's first member) -- a third of the entries of a full inverse suffix array, and the m-entry list is
//     what the tie detection, the compaction and the rounds stream instead of the n + 1 entries of SA;
//   * a round: all groups share >= D bases.  The members of a group share the LMS positions inside their common window
//     too, so a group picks the last position x = p + d, d < D, that the window alone proves to be an LMS position
//     (k_lms_stride: a type needs a differing base to its right, inside the window), and its members sort on
//     rank[(p + d) >> 1]: equal keys = equal through d + D bases.  The next round's D is D + the smallest stride.
//   * a group whose window ends in >= D/2 bases without such a position (a long run of one base, mostly) is "stuck": its
//     members (<= LX_STUCK_MAX) are ordered by comparing the text directly, which is final.
// Anything unexpected -- a stuck group of more members, comparisons that run past LX_STUCK_STEPS steps for one member,
// a rank that was never written -- aborts: the list is merged again as it was and kiss_exact_refine finishes the job on
// the suffix array as before (texts like A^1000 C repeated: their LMS suffixes are further apart than any window).
namespace {

constexpr uint32_t LX_STUCK_STEPS = 1u << 18; // all comparisons of one member of a stuck group together, <= 128 bases per step
constexpr uint32_t LX_STUCK_MAX = 8192;       // members of a stuck group (each is compared with all the others)
enum { LX_MAXLEN = 0, LX_MIN_D = 1, LX_ABORT = 2, LX_STUCK = 3 };

__global__ void k_lx_ctl_init(uint32_t *__restrict__ ctl)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ctl[LX_MIN_D] = 0xFFFFFFFFu;
        ctl[LX_ABORT] = 0;
        ctl[LX_STUCK] = 0;
    }
}

// suffix pi < suffix pj, both known to be equal on their first d bases (pi + d, pj + d <= n); the suffix that runs
// off the text first is the smaller one (the sentinel)
__device__ __forceinline__ bool exact_less(const uint64_t *__restrict__ pk, uint64_t n, uint64_t pi, uint64_t pj, uint64_t d,
                                           uint32_t &steps_left, bool *gave_up)
{
    for (; steps_left; steps_left--) {
        const uint64_t qi = pi + d, qj = pj + d;
        const uint64_t ri = n - qi, rj = n - qj; // bases left
        if (ri >= 160 && rj >= 160) {
            const uint32_t si = 2u * (uint32_t)(qi & 31u), sj = 2u * (uint32_t)(qj & 31u);
            uint64_t a[5], b[5];
            kiss_words5(pk, qi >> 5, a); // (aligned loads: kiss_internal.hpp)
            kiss_words5(pk, qj >> 5, b);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint64_t ki = (a[t] << si) | ((a[t + 1] >> 1) >> (63u - si));
                const uint64_t kj = (b[t] << sj) | ((b[t + 1] >> 1) >> (63u - sj));
                if (ki != kj) return ki < kj;
            }
            d += 128;
            continue;
        }
        uint64_t len = ri < rj ? ri : rj;
        if (len > 32) len = 32;
        uint64_t ki = kiss_key32(pk, qi), kj = kiss_key32(pk, qj);
        if (len < 32) {
            const uint64_t mask = len ? ~0ull << (64 - 2 * len) : 0ull;
            ki &= mask;
            kj &= mask;
        }
        if (ki != kj) return ki < kj;
        if (len < 32) return ri < rj; // one of them ends here
        d += 32;
    }
    *gave_up = true;
    return false;
}

// One thread per group: the stride d (0 = stuck).  Scans the window [p0, p0 + D) of the group's first member from its
// right end, at most scan_cap bases: position y + 1 is an LMS position if base(y) > base(y + 1) and y + 1 is S-type, and
// a type is only known once a differing base has been seen to the right.
__global__ __launch_bounds__(LS_THREADS) void k_lms_stride(const uint64_t *__restrict__ pk, uint64_t n,
                                                          const uint32_t *__restrict__ pos,
                                                          const uint32_t *__restrict__ segstart, uint64_t nseg, uint64_t D,
                                                          uint64_t scan_cap, uint32_t *__restrict__ dG,
                                                          uint32_t *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    uint32_t d = 0;
    const bool valid = g < nseg;
    if (valid) {
        const uint64_t p0 = pos[segstart[g]];
        if (p0 + D <= n) {
            uint64_t e = p0 + D; // bases [ylo, e) are still to be looked at
            const uint64_t ylo = (D - 1 > scan_cap) ? (e - 1 - scan_cap) : p0;
            int t = 0; // type of the base right of the current one: 0 unknown, 1 S, 2 L
            uint32_t cn = 0;
            bool first = true;
            while (e > ylo && d == 0) {
                const uint64_t s = (e - ylo > 32) ? e - 32 : ylo;
                const uint64_t w = kiss_key32(pk, s);
                int j = (int)(e - s) - 1;
                if (first) {
                    cn = (uint32_t)(w >> (62 - 2 * j)) & 3u;
                    j--;
                    first = false;
                }
                for (; j >= 0; j--) {
                    const uint32_t c = (uint32_t)(w >> (62 - 2 * j)) & 3u;
                    if (c > cn) {
                        if (t == 1) {
                            d = (uint32_t)(s + (uint64_t)j + 1 - p0);
                            break;
                        }
                        t = 2;
                    } else if (c < cn) {
                        t = 1;
                    }
                    cn = c;
                }
                e = s;
            }
        } else {
            atomicOr(&ctl[LX_ABORT], 8u); // a tied suffix without D bases: cannot be
        }
        dG[g] = d;
    }
    // smallest stride of the round (one atomic per wave, and only while it still lowers the minimum)
    uint32_t md = (valid && d) ? d : 0xFFFFFFFFu;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        const uint32_t o = __shfl_xor(md, x, 64);
        md = o < md ? o : md;
    }
    const uint64_t stuck = __ballot(valid && d == 0);
    if (lane_id() == 0) {
        if (md != 0xFFFFFFFFu && md < __hip_atomic_load(&ctl[LX_MIN_D], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(&ctl[LX_MIN_D], md);
        if (stuck) atomicAdd(&ctl[LX_STUCK], (uint32_t)__popcll(stuck));
    }
}

__global__ __launch_bounds__(LS_THREADS) void k_gather_ranks_lms(const uint32_t *__restrict__ rank,
                                                                const uint32_t *__restrict__ pos,
                                                                const uint32_t *__restrict__ seg,
                                                                const uint32_t *__restrict__ dG, uint64_t count, uint64_t n,
                                                                uint64_t *__restrict__ key, uint32_t *__restrict__ ctl)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t d = dG[seg[i]];
    uint64_t k = 0;
    if (d) {
        const uint64_t q = (uint64_t)pos[i] + d;
        const uint32_t r = q < n ? rank[q >> 1] : 0xFFFFFFFFu;
        if (r == 0xFFFFFFFFu) atomicOr(&ctl[LX_ABORT], 1u); // not an LMS position after all: cannot be
        k = (uint64_t)r << 32;
    }
    key[i] = k;
}

// k_group_sort_small for the LMS rounds: a stuck group orders itself by comparing the text from base D on
__global__ __launch_bounds__(LS_THREADS) void k_group_sort_small_lms(const uint64_t *__restrict__ pk, uint64_t n,
                                                                    const uint64_t *__restrict__ key,
                                                                    const uint32_t *__restrict__ pos,
                                                                    const uint32_t *__restrict__ seg,
                                                                    const uint32_t *__restrict__ segstart,
                                                                    const uint32_t *__restrict__ dG, uint64_t count,
                                                                    uint64_t D, uint64_t *__restrict__ okey,
                                                                    uint32_t *__restrict__ opos, uint64_t *__restrict__ big,
                                                                    uint32_t *__restrict__ ctl)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t sg = seg[i];
    const uint32_t a = segstart[sg], b = segstart[sg + 1];
    const bool stuck = dG[sg] == 0;
    const bool isbig = !stuck && b - a > SMALL_SEG; // (a stuck group is not sorted on keys, whatever its size)
    if (big) big[i] = isbig ? ((1ull << 32) | (uint64_t)((uint32_t)i == a ? 1u : 0u)) : 0ull;
    if (isbig) return;
    if (stuck && b - a > LX_STUCK_MAX) { // left where it is (the abort undoes the round anyway)
        if ((uint32_t)i == a) atomicOr(&ctl[LX_ABORT], 2u);
        okey[i] = 0;
        opos[i] = pos[i];
        return;
    }
    uint32_t r = 0;
    uint64_t ko;
    if (!stuck) {
        const uint64_t ki = key[i];
        for (uint32_t j = a; j < b; j++) {
            const uint64_t kj = key[j];
            r += (kj < ki || (kj == ki && j < (uint32_t)i)) ? 1u : 0u;
        }
        ko = ki;
    } else {
        const uint64_t pi = pos[i];
        bool gave_up = false;
        uint32_t steps_left = LX_STUCK_STEPS;
        for (uint32_t j = a; j < b; j++)
            if (j != (uint32_t)i) r += exact_less(pk, n, pos[j], pi, D, steps_left, &gave_up) ? 1u : 0u;
        if (gave_up) atomicOr(&ctl[LX_ABORT], 4u);
        ko = (uint64_t)r << 32; // all different: every member retires
    }
    okey[a + r] = ko;
    opos[a + r] = pos[i];
}

} // namespace

namespace {

// KISS_HIP_DEBUG: every pair the sort's tie flags (a) call tied must be tied by comparison (b) too
int cross_check_tie_flags(kiss_hip_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, const uint32_t *L, const uint32_t *C,
                          uint64_t m, uint32_t h0)
{
    std::vector<uint8_t> a(m), b(m);
    KCHECK(hipMemcpyAsync(a.data(), d_a, m, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipMemcpyAsync(b.data(), d_b, m, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    uint64_t tied_sort = 0, tied_cmp = 0, bad = 0;
    for (uint64_t i = 0; i < m; i++) {
        tied_sort += a[i] == 0;
        tied_cmp += b[i] == 0;
        bad += (a[i] == 0 && b[i] != 0);
    }
    fprintf(stderr, "[kiss_hip] lms refine: tie flags from the sort: %llu entries tied with their predecessor; by comparison "
                    "of %u bases: %llu; tied for the sort but not by comparison: %llu\n",
            (unsigned long long)tied_sort, h0, (unsigned long long)tied_cmp, (unsigned long long)bad);
    if (!bad) return KISS_HIP_OK;
    std::vector<uint32_t> hl(m), hcw(m);
    (void)hipMemcpy(hl.data(), L, m * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hcw.data(), C, m * 4, hipMemcpyDeviceToHost);
    int shown = 0;
    for (uint64_t i = 0; i < m && shown < 6; i++)
        if (a[i] == 0 && b[i] != 0) {
            shown++;
            fprintf(stderr, "[kiss_hip]   entry %llu of %llu (m_far %llu, near %u): position %u (taint %u), predecessor %u "
                            "(taint %u); flags around it, sort: %u %u %u  comparison: %u %u %u\n",
                    (unsigned long long)i, (unsigned long long)m, (unsigned long long)ctx->m_far, ctx->rm_E, hl[i],
                    hcw[i] >> 31, i ? hl[i - 1] : 0u, i ? hcw[i - 1] >> 31 : 0u, i ? a[i - 1] : 9u, a[i],
                    i + 1 < m ? a[i + 1] : 9u, i ? b[i - 1] : 9u, b[i], i + 1 < m ? b[i + 1] : 9u);
        }
    return KINTERNAL();
}

// The rounds of kiss_lms_exact_refine: D = h0, then D + the round's smallest stride, until nothing is tied or something
// unexpected shows (*why != 0: the caller gives up).  Against the suffix-array form: a stride per group in front of the rank
// gather, stuck groups ordered by comparison inside the group sort, and the control words read back twice a round.
int doubling_rounds_lms(kiss_hip_ctx *ctx, const Doubling &d, TiedBufs &bufs, uint64_t n, uint32_t h0, uint64_t count, uint64_t nseg,
                        uint32_t *ctl, uint32_t *bigpos0, uint32_t *bigpos1, uint32_t *why)
{
    const bool dbg = ctx->opts.debug;
    uint32_t *dG = ctx->bslot; // the stride of every group
    uint64_t D = h0;
    for (int rounds = 1; count > 0; rounds++) {
        if (rounds > 64 || D + 1 > n) {
            *why = 16;
            return KISS_HIP_OK;
        }
        const unsigned grid = (unsigned)div_up(count, LS_THREADS);
        {
            KTimer t(ctx, KISS_HIP_K_KEYGATHER, count);
            hipLaunchKernelGGL(k_lx_ctl_init, dim3(1), dim3(64), 0, ctx->stream, ctl);
            hipLaunchKernelGGL(k_lms_stride, dim3((unsigned)div_up(nseg, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, n,
                               bufs.cur.P, bufs.cur.SS, nseg, D, D / 2, dG, ctl);
            hipLaunchKernelGGL(k_gather_ranks_lms, dim3(grid), dim3(LS_THREADS), 0, ctx->stream, d.rank, bufs.cur.P, bufs.cur.G, dG,
                               count, n, ctx->bkeyA, ctl);
        }
        KTRY(kiss_readback(ctx, ctl, 4));
        const uint32_t maxlen = ctx->h_pinned[LX_MAXLEN], min_d = ctx->h_pinned[LX_MIN_D], nstuck = ctx->h_pinned[LX_STUCK];
        if ((*why = ctx->h_pinned[LX_ABORT])) return KISS_HIP_OK;
        {
            KTimer t(ctx, KISS_HIP_K_SEGRANK, count);
            hipLaunchKernelGGL(k_group_sort_small_lms, dim3(grid), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, n, ctx->bkeyA, bufs.cur.P,
                               bufs.cur.G, bufs.cur.SS, dG, count, D, ctx->bkeyB, ctx->bposB,
                               maxlen > SMALL_SEG ? ctx->flags : nullptr, ctl);
        }
        sync_point(ctx, d, 0);
        if (maxlen > SMALL_SEG) KTRY(sort_long_groups(ctx, d, bufs.cur.P, count, bigpos0, bigpos1));
        const uint64_t before = count, groups = nseg;
        KTRY(finish_round(ctx, d, bufs, &count, &nseg, ctl + LX_ABORT, why)); // (the abort word: what the sort kernel had to say)
        if (*why) return KISS_HIP_OK;
        if (dbg)
            fprintf(stderr, "[kiss_hip] lms refine D=%llu: items %llu in %llu groups (%u stuck, longest %s%u, stride >= %u) -> %llu\n",
                    (unsigned long long)D, (unsigned long long)before, (unsigned long long)groups, nstuck, maxlen ? "" : "<= ",
                    maxlen ? maxlen : 64u, min_d, (unsigned long long)count);
        if (min_d != 0xFFFFFFFFu) D += min_d;
    }
    return KISS_HIP_OK;
}

// tie flags (if the sort left none), the tied entries compacted and ranked, the rounds
int lms_refine_steps(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, uint32_t *scratch, uint8_t *heads, bool sort_flags, uint32_t *why)
{
    const uint64_t m = ctx->m;
    const bool dbg = ctx->opts.debug;
    uint32_t *L = ctx->lmsP, *C = ctx->lmsC;
    uint32_t *ctl = ctx->d_small + 8;
    if (!sort_flags || dbg) {
        // tie flags by comparison: both neighbours tainted and equal on their first h0 bases (the form without the sort's
        // flags -- KISS_HIP_LMS_HEADS_BY_COMPARE=1 --; with KISS_HIP_DEBUG also run beside them as a cross-check)
        uint8_t *hc = sort_flags ? heads + ((m + 64) & ~15ull) : heads;
        KTimer t(ctx, KISS_HIP_K_GROUP_HEADS, m);
        KTRY(heads_by_compare(ctx, L, m, n, h0, C, hc, 0u));
        if (sort_flags) KTRY(cross_check_tie_flags(ctx, heads, hc, L, C, m, h0));
    }
    Doubling d;
    d.list = L;
    d.len = m;
    d.heads = heads;
    d.rank = ctx->CTX; // (n >> 1) + 1 words of it
    d.rank_shift = 1;
    d.cfix = C;
    d.grow_lms = false; // (the list lives in them)
    d.d_total = (uint64_t *)(ctx->d_small + 2);
    d.d_maxlen = ctl + LX_MAXLEN;
    d.sync_points = ctx->opts.lx_sync_points;
    uint64_t count, nseg;
    KTRY(count_tied(ctx, d, &count, &nseg));
    ctx->stats.refine_items = count;
    if (dbg)
        fprintf(stderr, "[kiss_hip] lms refine: %llu of %llu LMS suffixes tied at depth %u in %llu groups\n",
                (unsigned long long)count, (unsigned long long)m, h0, (unsigned long long)nseg);
    if (count == 0) return KISS_HIP_OK; // nothing is tied: the list is exact as it stands
    KTRY(make_room_for_tied(ctx, d, count));
    // ranks (entries without an LMS position read as 0xFFFFFFFF).  The partition's pairs are in the suffix array buffer,
    // which is dead again once the rank array stands: the rounds sort their long groups' positions there
    uint64_t *pairs1 = reinterpret_cast<uint64_t *>(((uintptr_t)scratch + 7) & ~(uintptr_t)7);
    KTRY(kiss_rank_build_lms(ctx, L, ctx->lms_pos_complete ? ctx->lms_pos : (const uint32_t *)nullptr, m, n, d.rank, pairs1, ctx->keyA,
                             reinterpret_cast<uint32_t *>(ctx->keyB), 2 * ctx->m_cap));
    TiedBufs bufs(ctx);
    KTRY(compact_tied_from_heads(ctx, d, count, nseg, bufs.cur));
    return doubling_rounds_lms(ctx, d, bufs, n, h0, count, nseg, ctl, scratch, scratch + m, why);
}

} // namespace

int kiss_lms_exact_refine(kiss_hip_ctx *ctx, uint64_t n, uint32_t h0, uint32_t *scratch, bool *resolved)
{
    *resolved = false;
    if (h0 < 32 || n < h0 || !scratch) return KINTERNAL();
    const uint64_t m = ctx->m;
    ctx->hmerged = nullptr;
    if (m < 2) {
        KTRY(kiss_merge_lms(ctx));
        *resolved = true;
        return KISS_HIP_OK;
    }
    KTRY(kiss_need_ctx_words(ctx));
    ctx->ctx_words_valid = false;
    // CTX (n + 2 words, not in use before the induction): the rank array, then one tie flag byte per list entry
    // (and, at its far end, ctx->hfar: the tie flags the LMS sort wrote for the far list, api.hip)
    const uint64_t r_words = (n >> 1) + 1;
    uint8_t *heads = reinterpret_cast<uint8_t *>(ctx->CTX + ((r_words + 3) & ~3ull));
    if (((r_words + 3) & ~3ull) + (m + 16) / 4 + 1 > ctx->max_n + 2) return KINTERNAL();
    // the merged list; with the sort's own tie flags (ctx->hfar) the flags of the merged list come out of the same pass
    const bool sort_flags = ctx->hfar != nullptr && ctx->h_depth == h0;
    ctx->hmerged = sort_flags ? heads : nullptr;
    ctx->lms_merged = false;
    {
        const int mrc = kiss_merge_lms(ctx);
        ctx->hmerged = nullptr;
        if (mrc) return mrc;
    }
    // the partition's pairs need 2 m words of the (n + 1)-word scratch, 8-byte aligned: a text with n/2 LMS suffixes in a
    // buffer that starts on an odd word has one word too few -- the suffix-array form takes that call
    if (((uintptr_t)scratch & 7) && 2 * m + 2 > n + 1) {
        ctx->lms_merged = false;
        return kiss_merge_lms(ctx);
    }
    uint32_t why = 0; // reason bits of an abort: a stuck group too large, a walk too long, a rank never written, too many rounds
    const uint64_t rounds_before = ctx->stats.doubling_rounds, item_rounds_before = ctx->stats.sort_item_rounds;
    int rc = lms_refine_steps(ctx, n, h0, scratch, heads, sort_flags, &why);
    if (rc == KISS_HIP_OK && hipGetLastError() != hipSuccess) rc = KISS_HIP_E_HIP;
    if (rc) return rc;
    if (why) { // the list as the bounded phase left it: kiss_exact_refine takes over after the induction
        if (ctx->opts.debug) fprintf(stderr, "[kiss_hip] lms refine: gave up (reason bits %u), the suffix-array form takes over\n", why);
        ctx->stats.doubling_rounds = (uint32_t)rounds_before;
        ctx->stats.sort_item_rounds = item_rounds_before;
        ctx->lms_merged = false;
        ctx->hmerged = nullptr;
        return kiss_merge_lms(ctx);
    }
    *resolved = true;
    return KISS_HIP_OK;
}
