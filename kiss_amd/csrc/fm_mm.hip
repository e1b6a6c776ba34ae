// fm_mm.hip -- FM-index: batched search with up to KISS_HIP_FMI_MAX_MISMATCHES substitutions (kiss_hip_fmi_query_mm_*).
//
// The reference has no such function; ground truth is the text itself (Hamming distance, tests/fm_mm_model.py).
//
//   search  : backward search that branches.  At most e positions deviate, so the tree is walked without a general stack:
//             level d = "d mismatches so far" holds ONE walking frame (beg, end, position) and the up to three children
//             its parent has just spawned (the other three bases at the parent's position).  A frame walks the pattern
//             exactly from the right; while d < e every step also evaluates the three other bases ON THE SAME ONE OR TWO
//             RANK BLOCKS (the block loads are the cost of a step, the four counts are arithmetic) and, if any child is
//             non-empty, the frame is parked and the lane descends.  A frame dies when its range is empty and emits a
//             leaf (q, beg, end, d) when it has consumed position 0.  Different strings of one length own disjoint SA
//             ranges: the leaves of a pattern need no de-duplication.
//   shape   : two tiers.  ONE LANE PER PATTERN first: all lanes of a wave run ONE loop whatever their level (the levels
//             live in shared memory, indexed by d), so lanes at different depths do not serialise; only the LENGTH of the
//             walks differs between the lanes of a wave -- by orders of magnitude at e >= 2, and the kernel runs as long as
//             its longest lane.  So a lane that has evaluated more than MM_HEAVY_PAIRS[e] pairs gives its pattern up, and
//             ONE WAVE PER PATTERN searches those again from the start: frame 0 walked once by the whole wave (uniform
//             addresses), 64 positions at a time into shared memory, the (position, base) starts of frame 1 dealt to the
//             lanes from a shared counter, rightmost positions first (there the ranges are still wide and the subtrees
//             big); deeper frames run inside the lane.  A wave for EVERY pattern of a large batch was measured and
//             dropped: a wave that serves one pattern has one chain of dependent loads in flight while frame 0 walks and
//             mostly still-born tasks afterwards, a wave of 64 patterns has 64.  A SMALL batch (<= MM_WAVE_ONLY_Q patterns)
//             is the other way round -- too few lanes to fill the device, and the longest lane is the whole kernel --, so
//             it goes to the waves directly (DESIGN.md 4.6 has the numbers; both single-tier forms can be forced in the
//             hooks build, KissOpts::fm_mm_wave / fm_mm_budget, as the A-Bs).
//   locate  : leaf sizes -> exclusive scan; one lane per hit row finds its leaf by binary search, walks LF to a sampled
//             row (at most SA_INTV - 1 steps, never past the primary row: the walk is bounded whatever arrays it is
//             handed) and writes the sort key (q << 32 | position) and the mismatch count.
//   order   : the library's stable radix sort on that key, payload = mismatch count: ascending position inside a pattern.
//             It runs in the ctx's LMS key / position arrays, which bound the hits of one call.
// counts[q][j] never needs the locate: it is the sum of the leaf sizes of class j, kept in registers by the search.
#include "fm_internal.hpp"

namespace {

constexpr int MM_LANE_THREADS = 256; // one lane per pattern
constexpr int MM_WAVE_THREADS = 64;  // one wave (= one workgroup: __syncthreads() is a wave barrier) per pattern
constexpr int MM_CHUNK = 64;         // frame-0 positions walked per round of the wave form
constexpr int MM_LOC_THREADS = 256;

// control block of a call (u64 words)
enum { MM_NLEAVES = 0 /* leaf slots handed out */, MM_HITS0 = 1 /* .. 4 */, MM_LF = 5, MM_WALKFAIL = 6, MM_CHECKSUM = 7,
       MM_RANGES = 8 /* leaves written */, MM_CTL_WORDS = 10 };

// Leaves go to one global list.  A wave takes MM_LEAF_CHUNK slots of it at a time with ONE atomic and fills them from its
// ballots; what it leaves unused is written as empty leaves (beg == end: no rows, the locate's search skips them).  One
// atomic per wave and leaf ballot on the single counter was a third of the e = 0 kernel (15 600 waves, one address).
// A call that wants no positions passes no list (leaves == nullptr): the leaves are counted and nothing is reserved.
struct MmLeafOut {
    uint4 *leaves;
    uint64_t cap;
    unsigned long long *ctl;
    uint32_t chunk;              // slots taken at a time: 64 with a pattern per lane, 8 with one per wave (at least the ballot's)
    unsigned long long base = 0; // of this wave's chunk (uniform)
    uint32_t size = 0, used = 0; // its slots, and how many of them are taken (uniform); size <= 64
    uint32_t written = 0;        // this lane's leaves
};
__device__ __forceinline__ void mm_leaf_pad(MmLeafOut &o)
{
    const uint32_t l = lane_id();
    if (l < o.size - o.used) {
        const uint64_t slot = o.base + o.used + l;
        if (slot < o.cap) o.leaves[slot] = make_uint4(0u, 0u, 0u, 0u);
    }
    o.used = o.size;
}
// called by every lane of the wave (a ballot inside)
__device__ __forceinline__ void mm_leaf_emit(MmLeafOut &o, bool leaf, uint32_t q, uint32_t beg, uint32_t end, uint32_t d)
{
    if (!o.leaves) { // counts only
        o.written += leaf ? 1u : 0u;
        return;
    }
    const uint64_t lm = __ballot(leaf);
    if (!lm) return;
    const uint32_t cnt = (uint32_t)__popcll(lm);
    if (o.used + cnt > o.size) {
        mm_leaf_pad(o);
        o.size = cnt > o.chunk ? cnt : o.chunk;
        unsigned long long b = 0;
        if (lane_id() == 0) b = atomicAdd(&o.ctl[MM_NLEAVES], (unsigned long long)o.size);
        o.base = __shfl(b, 0, 64);
        o.used = 0;
    }
    if (leaf) {
        const uint64_t slot = o.base + o.used + (uint32_t)__popcll(lm & lanemask_lt());
        if (slot < o.cap) o.leaves[slot] = make_uint4(q, beg, end, d);
        o.written++;
    }
    o.used += cnt;
}

// Per-lane state of the levels, in shared memory as [word][lane] (a lane only ever touches its own column, consecutive
// lanes hit consecutive banks).  Level l = 1 .. E: pend[l][k] = child k the frame of level l - 1 spawned, (0, 0) = none /
// taken.  Level l = 0 .. E - 1: the parked frame (beg, end, next position); (0, 0) = it died at the step that spawned.
// The children of level l start at the position the parked frame of level l - 1 continues at.
template <int E> struct MmWords { static constexpr int value = E ? 9 * E : 1; };
#define MM_PEND(l, k, w) st[((l) - 1) * 6 + (k) * 2 + (w)][tid]
#define MM_SAVE(l, w) st[6 * E + (l) * 3 + (w)][tid]

// E: the mismatch bound (0..3).  WAVE = false: one lane per pattern, every pattern of the batch; a lane that has evaluated
// more than `budget` pairs gives its pattern up -- it flags it (hflag), appends it to the heavy list (heavy[0] = count,
// heavy[1 ..] = pattern numbers) and writes no counts; the leaves it has emitted carry MM_LEAF_LANE_PASS and are dropped by
// k_fm_mm_leaf_sizes.  WAVE = true: one wave per pattern, from the start -- the patterns of the heavy list (from_list; the
// number is only known on the device, so a fixed grid walks the list), or every pattern (the A-B of the hooks build).
constexpr uint32_t MM_LEAF_LANE_PASS = 0x100u;
template <int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? MM_WAVE_THREADS : MM_LANE_THREADS) void
k_fm_mm_search(FmiD f, const uint8_t *__restrict__ pat, uint32_t L, uint64_t Q, uint32_t *__restrict__ counts,
               uint64_t *__restrict__ qtot /* may be null */, uint4 *__restrict__ leaves, uint64_t leaf_cap,
               unsigned long long *__restrict__ ctl, unsigned long long budget, uint32_t *__restrict__ heavy_list,
               uint8_t *__restrict__ hflag, int from_list)
{
    constexpr int THREADS = WAVE ? MM_WAVE_THREADS : MM_LANE_THREADS;
    __shared__ uint32_t st[MmWords<E>::value][THREADS];
    __shared__ uint2 fr0[WAVE ? MM_CHUNK : 1];
    __shared__ uint32_t s_next;
    const uint32_t tid = threadIdx.x;
    const uint32_t N = (uint32_t)f.N;
    MmLeafOut out;
    out.leaves = leaves;
    out.cap = leaf_cap;
    out.ctl = ctl;
    out.chunk = WAVE ? 8u : 64u;
    unsigned long long lf = 0; // fm_lf2-equivalents (a (range, base) pair evaluated)
    const uint64_t npat = WAVE ? (from_list ? (uint64_t)heavy_list[0] : Q) : 1;
    for (uint64_t it = WAVE ? blockIdx.x : 0; it < npat; it += WAVE ? gridDim.x : 1) {
        const uint64_t q = WAVE ? (from_list ? (uint64_t)heavy_list[1 + it] : it) : (uint64_t)blockIdx.x * THREADS + tid;
        const bool live = q < Q;
        const uint8_t *p = pat + (live ? q : 0) * (uint64_t)L;
        uint32_t cls[4] = {0, 0, 0, 0}; // hits by number of mismatches (this lane's leaves)
        bool heavy = false;
        // frame 0 of the wave form (uniform over the wave)
        uint32_t fb = 0, fe = N;
        int hi = (int)L - 1;
        // the lane's walking frame
        int d = 0, pos = hi;
        uint32_t beg = 0, end = N, tk = 0;
        bool walking = !WAVE && live, done = !WAVE && !live;
        uint32_t ntasks = 0;

        for (;;) {
            if (WAVE) { // the next MM_CHUNK positions of frame 0, then their (position, base) tasks
                if (hi < 0 || fb >= fe) break;
                const int len = hi + 1 < MM_CHUNK ? hi + 1 : MM_CHUNK;
                uint32_t na = 0;
                for (int j = 0; j < len && fb < fe; j++) {
                    if (tid == 0) fr0[j] = make_uint2(fb, fe); // the range BEFORE position hi - j is consumed
                    na++;
                    uint64_t b64 = fb, e64 = fe;
                    fm_lf2(f, p[hi - j] & 3u, b64, e64);
                    fb = b64 < N ? (uint32_t)b64 : N;
                    fe = e64 < N ? (uint32_t)e64 : N;
                }
                if (tid == 0) {
                    lf += na;
                    s_next = 0;
                }
                ntasks = 3 * na;
                __syncthreads();
                d = 0;
                walking = false;
                done = false;
            }
            // ---- the walk: every lane of the wave runs this one loop, whatever its level ------------------------
            for (;;) {
                while (!walking && !done) {
                    if (d == 0) { // the root frame is finished: the next task of this pattern, or nothing
                        if (WAVE) {
                            const uint32_t t = atomicAdd(&s_next, 1u);
                            if (t >= ntasks) {
                                done = true;
                            } else {
                                const uint32_t j = t / 3u;
                                tk = t - 3u * j;
                                const uint2 r = fr0[j];
                                beg = r.x;
                                end = r.y;
                                pos = hi - (int)j;
                                walking = true;
                            }
                        } else {
                            done = true;
                        }
                    } else if (E) {
                        int k = -1;
#pragma unroll
                        for (int u = 2; u >= 0; u--)
                            if (MM_PEND(d, u, 0) != MM_PEND(d, u, 1)) k = u;
                        if (k >= 0) { // the next child of this level
                            beg = MM_PEND(d, k, 0);
                            end = MM_PEND(d, k, 1);
                            MM_PEND(d, k, 0) = 0;
                            MM_PEND(d, k, 1) = 0;
                            pos = (int)MM_SAVE(d - 1, 2);
                            walking = true;
                        } else { // back to the parked frame of the parent
                            d--;
                            beg = MM_SAVE(d, 0);
                            end = MM_SAVE(d, 1);
                            pos = (int)MM_SAVE(d, 2);
                            walking = beg != end;
                        }
                    }
                }
                // leaves: appended once per wave and iteration
                const bool leaf = walking && pos < 0;
                mm_leaf_emit(out, leaf, (uint32_t)q, beg, end, (uint32_t)d | (WAVE ? 0u : MM_LEAF_LANE_PASS));
                if (leaf) {
                    const uint32_t sz = end - beg;
                    cls[0] += d == 0 ? sz : 0u;
                    cls[1] += d == 1 ? sz : 0u;
                    cls[2] += d == 2 ? sz : 0u;
                    cls[3] += d == 3 ? sz : 0u;
                    walking = false;
                }
                if (__all(done)) break;
                if (walking) { // one step: position `pos` of the pattern, all bases wanted on the same one or two blocks
                    const uint32_t c0 = p[pos] & 3u;
                    const FmBlock bb = fm_block(f, beg >> 6);
                    const FmBlock be = (end >> 6) == (beg >> 6) ? bb : fm_block(f, end >> 6);
                    const bool root_task = WAVE && d == 0; // only base tk deviates here, and frame 0 itself is the wave's
                    bool spawned = false;
                    if (E && d < E) {
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) {
                            const uint32_t c = (c0 + 1u + k) & 3u;
                            uint32_t nb = 0, ne = 0;
                            if (!root_task || k == tk) {
                                nb = f.cnt[c] + fm_occ_in(f, bb, c, beg);
                                ne = f.cnt[c] + fm_occ_in(f, be, c, end);
                                nb = nb < N ? nb : N;
                                ne = ne < N ? ne : N;
                                lf++;
                            }
                            if (nb >= ne) nb = ne = 0;
                            MM_PEND(d + 1, k, 0) = nb;
                            MM_PEND(d + 1, k, 1) = ne;
                            spawned |= nb != ne;
                        }
                    }
                    bool alive = false;
                    if (!root_task) {
                        uint32_t nb = f.cnt[c0] + fm_occ_in(f, bb, c0, beg), ne = f.cnt[c0] + fm_occ_in(f, be, c0, end);
                        beg = nb < N ? nb : N;
                        end = ne < N ? ne : N;
                        alive = beg < end;
                        lf++;
                    }
                    pos--;
                    if (E && spawned) {
                        MM_SAVE(d, 0) = alive ? beg : 0u;
                        MM_SAVE(d, 1) = alive ? end : 0u;
                        MM_SAVE(d, 2) = (uint32_t)pos;
                        d++;
                        walking = false;
                    } else {
                        walking = alive;
                    }
                    if (!WAVE && lf > budget) { // a heavy pattern: a wave takes it over from the start (MM_HEAVY_*)
                        heavy = true;
                        walking = false;
                        done = true;
                    }
                }
            }
            if (!WAVE) break;
            __syncthreads(); // (fr0 and the counter of this round are dead)
            hi -= MM_CHUNK;
            const bool f0_leaf = hi < 0 && fb < fe; // frame 0 consumed the whole pattern: the exact occurrences
            mm_leaf_emit(out, f0_leaf && tid == 0, (uint32_t)q, fb, fe, 0u);
            if (f0_leaf && tid == 0) cls[0] += fe - fb;
        }
        // per-pattern counts and the totals of the call
        if (WAVE) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (int j = 0; j <= E; j++) cls[j] += __shfl_xor(cls[j], s, 64);
            }
            if (tid == 0) {
                unsigned long long tot = 0;
#pragma unroll
                for (int j = 0; j <= E; j++) {
                    counts[q * (E + 1) + j] = cls[j];
                    tot += cls[j];
                    if (cls[j]) atomicAdd(&ctl[MM_HITS0 + j], (unsigned long long)cls[j]);
                }
                if (qtot) qtot[q] = tot;
            }
            __syncthreads(); // (the shared state of this pattern is dead)
        } else {
            // heavy patterns: flagged, listed (one append per wave), and nothing of theirs counted here
            const uint64_t hm = __ballot(heavy);
            if (hm) {
                uint32_t hb = 0;
                if (lane_id() == 0) hb = atomicAdd(&heavy_list[0], (uint32_t)__popcll(hm));
                hb = __shfl(hb, 0, 64);
                if (heavy) {
                    heavy_list[1 + hb + (uint32_t)__popcll(hm & lanemask_lt())] = (uint32_t)q;
                    hflag[q] = 1;
                    cls[0] = cls[1] = cls[2] = cls[3] = 0;
                    out.written = 0;
                }
            }
            unsigned long long tot = 0;
            if (live && !heavy) {
#pragma unroll
                for (int j = 0; j <= E; j++) {
                    counts[q * (E + 1) + j] = cls[j];
                    tot += cls[j];
                }
                if (qtot) qtot[q] = tot;
            }
            unsigned long long w[4] = {cls[0], cls[1], cls[2], cls[3]};
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (int j = 0; j <= E; j++) w[j] += __shfl_xor(w[j], s, 64);
            }
            if (lane_id() == 0) {
#pragma unroll
                for (int j = 0; j <= E; j++)
                    if (w[j]) atomicAdd(&ctl[MM_HITS0 + j], w[j]);
            }
        }
    }
    mm_leaf_pad(out);
    unsigned long long nw = out.written;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        nw += __shfl_xor(nw, s, 64);
        lf += __shfl_xor(lf, s, 64);
    }
    if (lane_id() == 0) {
        if (nw) atomicAdd(&ctl[MM_RANGES], nw);
        if (lf) atomicAdd(&ctl[MM_LF], lf);
    }
}
#undef MM_PEND
#undef MM_SAVE

// (leaves a lane emitted before it gave its pattern up count no rows: the wave that took the pattern over emits them again)
__global__ __launch_bounds__(MM_LOC_THREADS) void k_fm_mm_leaf_sizes(const uint4 *__restrict__ leaves, uint64_t nleaves,
                                                                    const uint8_t *__restrict__ hflag,
                                                                    uint64_t *__restrict__ sizes)
{
    const uint64_t i = (uint64_t)blockIdx.x * MM_LOC_THREADS + threadIdx.x;
    if (i > nleaves) return;
    uint64_t s = 0;
    if (i < nleaves) {
        const uint4 lv = leaves[i];
        s = lv.z - lv.y;
        if (s && (lv.w & MM_LEAF_LANE_PASS) && hflag[lv.x]) s = 0;
    }
    sizes[i] = s; // [nleaves] = 0: the scan turns it into the total
}

// one lane per hit row: its leaf by binary search in the scanned sizes, then the bounded walk to a sampled row
// (fm_locate_row).  A row that finds no sampled row inside the bound (an index that was not built from an exact suffix
// array) is counted and gets position 0xFFFFFFFF.
__global__ __launch_bounds__(MM_LOC_THREADS) void k_fm_mm_locate(FmiD f, uint32_t sa_intv, uint64_t sa_entries,
                                                                const uint4 *__restrict__ leaves, uint64_t nleaves,
                                                                const uint64_t *__restrict__ leaf_index, uint64_t total,
                                                                int key_shift, uint64_t *__restrict__ keys,
                                                                uint32_t *__restrict__ vals,
                                                                unsigned long long *__restrict__ ctl)
{
    const uint64_t h = (uint64_t)blockIdx.x * MM_LOC_THREADS + threadIdx.x;
    unsigned long long sum = 0;
    bool fail = false;
    if (h < total) {
        uint64_t lo = 0, hi = nleaves; // last leaf with leaf_index[leaf] <= h
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (leaf_index[mid] <= h) lo = mid;
            else hi = mid;
        }
        const uint4 lv = leaves[lo];
        const uint64_t row = (uint64_t)lv.y + (h - leaf_index[lo]);
        uint32_t position;
        fail = !fm_locate_row(f, sa_intv, sa_entries, row, position);
        keys[h] = (((uint64_t)lv.x << 32) | position) << key_shift;
        vals[h] = lv.w & 0xFFu;
        if (!fail) sum = position;
    }
    const unsigned long long nf = (unsigned long long)__popcll(__ballot(fail));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if (lane_id() == 0) {
        if (sum) atomicAdd(&ctl[MM_CHECKSUM], sum);
        if (nf) atomicAdd(&ctl[MM_WALKFAIL], nf);
    }
}

__global__ __launch_bounds__(MM_LOC_THREADS) void k_fm_mm_unpack(const uint64_t *__restrict__ keys,
                                                                const uint32_t *__restrict__ vals, uint64_t total,
                                                                int key_shift, uint32_t *__restrict__ positions,
                                                                uint8_t *__restrict__ mismatches)
{
    const uint64_t i = (uint64_t)blockIdx.x * MM_LOC_THREADS + threadIdx.x;
    if (i >= total) return;
    positions[i] = (uint32_t)(keys[i] >> key_shift);
    mismatches[i] = (uint8_t)vals[i];
}

// A pattern whose lane has evaluated more (range, base) pairs than this is searched again by a wave of its own.  The lane
// kernel runs as long as its longest lane, and a lane spends some 0.7 us per pair (two dependent loads per step).  Measured
// on the dm-size text, 10^6 patterns of 32 bases (10^5 at e = 3), ms of the search (profiles/fm_mismatch_dm_size.json,
// DESIGN.md 4.6):
//   e = 1: lanes only 9.20, bound 256 22.9, bound 1024 8.20, bound 4096 9.20;
//   e = 2: lanes only 97.6, bound 2048 262, bound 8192 91.1, bound 32768 97.7;
//   e = 3: lanes only 121.7, bound 32768 328 (the mean pattern needs 38 600 pairs: most patterns are then searched twice),
//          bound 131072 121.9, bound 524288 121.9 -- no bound helps there, the batch is as long as its longest patterns.
//   A wave per pattern from the start: 22.4 / 138.2 / 164.8.
constexpr unsigned long long MM_HEAVY_PAIRS[4] = {~0ull, 1024, 8192, 131072};
constexpr unsigned MM_HEAVY_GRID = 4096; // waves that walk the heavy list
// A batch of at most this many patterns skips the lanes: the lane kernel cannot be shorter than its longest lane (17 ms at
// e = 2, 117 ms at e = 3 on the dm-size text, whatever the batch), the wave kernel's time is proportional to the batch
// (22 / 138 / 1650 us per 1000 patterns at e = 1 / 2 / 3).  The two meet at about 80 000 / 120 000 / 70 000 patterns.  It is what
// every part of a batch that is split by its number of hits runs.
constexpr uint64_t MM_WAVE_ONLY_Q = 65536;

template <bool WAVE>
void mm_launch_search(kiss_hip_ctx *ctx, uint32_t e, const FmiD &f, const uint8_t *pat, uint32_t L, uint64_t Q,
                      uint32_t *counts, uint64_t *qtot, uint4 *leaves, uint64_t leaf_cap, unsigned long long *ctl,
                      unsigned long long budget, uint32_t *heavy_list, uint8_t *hflag, int from_list)
{
    const unsigned grid = WAVE ? (unsigned)(from_list && Q > MM_HEAVY_GRID ? MM_HEAVY_GRID : Q) : (unsigned)div_up(Q, MM_LANE_THREADS);
    const dim3 block(WAVE ? MM_WAVE_THREADS : MM_LANE_THREADS);
#define MM_GO(E_)                                                                                                      \
    hipLaunchKernelGGL((k_fm_mm_search<E_, WAVE>), dim3(grid), block, 0, ctx->stream, f, pat, L, Q, counts, qtot, leaves, \
                       leaf_cap, ctl, budget, heavy_list, hflag, from_list)
    switch (e) {
    case 0: MM_GO(0); break;
    case 1: MM_GO(1); break;
    case 2: MM_GO(2); break;
    default: MM_GO(3); break;
    }
#undef MM_GO
}

int mm_query_steps(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                   uint32_t e, uint32_t *counts, uint32_t *positions, uint8_t *mismatches, uint64_t *index,
                   uint64_t capacity, kiss_hip_fmi_mm_report *rep, FmEvents &ev)
{
    const bool want = positions != nullptr;
    if (Q > 0x7FFFFFFFull || Q / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    kiss_opts_refresh(ctx);
    const uint32_t sa_intv = fmi->sa_intv;
    FmiD f = fm_view_of(fmi);
    const uint64_t sa_entries = (f.N + sa_intv - 1) / sa_intv;

    DevBuf blocks, leaves, qtot, lsize, lidx, heavy, hflag;
    FmCtl<MM_CTL_WORDS> ctl;
    const uint64_t nblocks = f.N / 64 + 1;
    KTRY(blocks.take(ctx, FM_SLOT_BLOCKS, nblocks * 32));
    f.blk = (const uint4 *)blocks.p;
    KTRY(ctl.take(ctx, FM_SLOT_MM_CTL));
    if (want) KTRY(qtot.take(ctx, FM_SLOT_MM_QTOT, (Q + 1) * 8));
    KTRY(heavy.take(ctx, FM_SLOT_MM_HEAVY, (Q + 2) * 4));
    KTRY(hflag.take(ctx, FM_SLOT_MM_HFLAG, (Q + 8) & ~3ull));
    ev.mark(0);
    KTRY(kiss_fm_make_blocks(ctx, f, nblocks, (uint4 *)blocks.p));
    // the leaf list (only for positions) is sized by what the pool holds (the previous batch of this ctx); a batch that
    // emits more says how many and is searched a second time, with headroom: the waves take their chunks of slots in an
    // order that differs from run to run, and so does the number of slots they leave unused
    // (hooks build: every pattern by a wave / a bound of the caller's for the lanes, the A-Bs of DESIGN.md 4.6)
    const bool lane_form = e == 0 || (!ctx->opts.fm_mm_wave && (Q > MM_WAVE_ONLY_Q || ctx->opts.fm_mm_budget));
    const unsigned long long budget = e == 0 ? ~0ull : ctx->opts.fm_mm_budget ? ctx->opts.fm_mm_budget : MM_HEAVY_PAIRS[e];
    unsigned long long *const h = ctl.h;
    uint64_t leaf_cap = 0;
    for (int attempt = 0;; attempt++) {
        if (want) {
            const uint64_t want_leaves = attempt ? h[MM_NLEAVES] + h[MM_NLEAVES] / 4 + 65536 : (e ? 8 * Q : 2 * Q) + 1024;
            const uint64_t held = ctx->fm_pool_cap[FM_SLOT_MM_LEAVES];
            KTRY(leaves.take(ctx, FM_SLOT_MM_LEAVES, held / 16 < want_leaves ? want_leaves * 16 : held));
            leaf_cap = ctx->fm_pool_cap[FM_SLOT_MM_LEAVES] / 16;
        }
        KTRY(ctl.zero());
        KTRY(kiss_zero_u32(ctx, heavy.p, 1));
        KTRY(kiss_zero_u32(ctx, hflag.p, (Q + 3) / 4));
        {
            KTimer t(ctx, KISS_HIP_K_FM_QUERY, Q);
            ev.mark(1);
            uint64_t *qt = want ? (uint64_t *)qtot.p : nullptr;
            if (lane_form) {
                mm_launch_search<false>(ctx, e, f, patterns, L, Q, counts, qt, (uint4 *)leaves.p, leaf_cap,
                                        ctl.d, budget, (uint32_t *)heavy.p, (uint8_t *)hflag.p, 0);
                if (e) // the patterns the lanes gave up, a wave each (none: the waves find an empty list)
                    mm_launch_search<true>(ctx, e, f, patterns, L, Q, counts, qt, (uint4 *)leaves.p, leaf_cap,
                                           ctl.d, 0, (uint32_t *)heavy.p, (uint8_t *)hflag.p, 1);
            } else {
                mm_launch_search<true>(ctx, e, f, patterns, L, Q, counts, qt, (uint4 *)leaves.p, leaf_cap,
                                       ctl.d, 0, (uint32_t *)heavy.p, (uint8_t *)hflag.p, 0);
            }
            ev.mark(2);
            KCHECK(hipGetLastError());
        }
        KTRY(ctl.fetch_sync());
        if (h[MM_NLEAVES] <= leaf_cap) break;
        if (attempt) return KINTERNAL();
    }
    const uint64_t nleaves = h[MM_NLEAVES];
    uint64_t total = 0;
    if (rep) {
        for (int j = 0; j < 4; j++) rep->hits[j] = h[MM_HITS0 + j];
        rep->ranges = h[MM_RANGES];
        rep->lf_pairs = h[MM_LF];
        rep->ms_search = ev.ms(1, 2);
    }
    for (int j = 0; j < 4; j++) total += h[MM_HITS0 + j];
    int rc = KISS_HIP_OK;
    if (want) {
        if (capacity < total) return KISS_HIP_E_INVALID; // (the total is in the report: the caller's second call)
        // the sort runs in the ctx's LMS key / position arrays
        if (total > ctx->m_cap || nleaves / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
        KTRY(kiss_zero_u32(ctx, (uint8_t *)qtot.p + Q * 8, 2));
        KTRY(kiss_scan_u64(ctx, (const uint64_t *)qtot.p, index, Q + 1));
        if (total) {
            KTRY(lsize.take(ctx, FM_SLOT_MM_LEAF_SIZE, (nleaves + 1) * 8));
            KTRY(lidx.take(ctx, FM_SLOT_MM_LEAF_INDEX, (nleaves + 1) * 8));
            const int key_shift = (32 - fm_bits(Q, 32, 0)) & ~7; // the sort takes whole bytes from the top of the key
            {
                KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
                ev.mark(3);
                hipLaunchKernelGGL(k_fm_mm_leaf_sizes, dim3((unsigned)div_up(nleaves + 1, MM_LOC_THREADS)), dim3(MM_LOC_THREADS), 0,
                                   ctx->stream, (const uint4 *)leaves.p, nleaves, (const uint8_t *)hflag.p, (uint64_t *)lsize.p);
                KCHECK(hipGetLastError());
                KTRY(kiss_scan_u64(ctx, (const uint64_t *)lsize.p, (uint64_t *)lidx.p, nleaves + 1));
                hipLaunchKernelGGL(k_fm_mm_locate, dim3((unsigned)div_up(total, MM_LOC_THREADS)), dim3(MM_LOC_THREADS), 0, ctx->stream,
                                   f, sa_intv, sa_entries, (const uint4 *)leaves.p, nleaves, (const uint64_t *)lidx.p, total,
                                   key_shift, ctx->keyA, ctx->posA, ctl.d);
                KCHECK(hipGetLastError());
                ev.mark(4);
            }
            RadixBufs rb = kiss_ctx_radix_bufs(ctx);
            int res = 0;
            KTRY(kiss_radix_sort(ctx, rb, total, key_shift, 0, &res));
            {
                KTimer t(ctx, KISS_HIP_K_FM_QUERY, total);
                hipLaunchKernelGGL(k_fm_mm_unpack, dim3((unsigned)div_up(total, MM_LOC_THREADS)), dim3(MM_LOC_THREADS), 0, ctx->stream,
                                   rb.key[res], rb.pos[res], total, key_shift, positions, mismatches);
                KCHECK(hipGetLastError());
            }
            ev.mark(5);
            KTRY(ctl.fetch());
            KTRY(kiss_radix_check(ctx)); // (synchronises)
            if (rep) {
                rep->walk_failures = h[MM_WALKFAIL];
                rep->checksum = h[MM_CHECKSUM];
                rep->ms_locate = ev.ms(3, 4);
                rep->ms_sort = ev.ms(4, 5);
            }
            if (h[MM_WALKFAIL]) rc = KISS_HIP_E_INVALID; // not an index of an exact suffix array: positions are not defined
        } else {
            KCHECK(hipStreamSynchronize(ctx->stream));
        }
    }
    return rc;
}

int fmi_query_mm(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                 uint32_t e, uint32_t *counts, uint32_t *positions, uint8_t *mismatches, uint64_t *index,
                 uint64_t capacity, kiss_hip_fmi_mm_report *rep, void *stream)
{
    KTRY(fm_enter(ctx, stream));
    if (Q == 0) return KISS_HIP_OK;
    FmEvents ev(ctx, rep != nullptr);
    const int rc = mm_query_steps(ctx, fmi, patterns, L, Q, e, counts, positions, mismatches, index, capacity, rep, ev);
    return fm_leave(ctx, ev, rc, rep ? &rep->ms_total : nullptr);
}

} // namespace

extern "C" {

int kiss_hip_fmi_query_mm_dev(kiss_hip_ctx *ctx, const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                              uint32_t max_mismatches, uint32_t *counts, uint32_t *positions, uint8_t *mismatches,
                              uint64_t *index, uint64_t capacity, kiss_hip_fmi_mm_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    if (report) {
        *report = kiss_hip_fmi_mm_report{};
        report->Q = Q;
        report->L = L;
        report->max_mismatches = max_mismatches;
    }
    if (!fmi) return KISS_HIP_E_INVALID;
    if (max_mismatches > KISS_HIP_FMI_MAX_MISMATCHES || !fm_sa_intv_ok(fmi->sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    const bool any = positions || mismatches || index, all = positions && mismatches && index;
    if (!ctx || L == 0 || fmi->n_sa == 0 || (Q && (!patterns || !counts)) || any != all || (!any && capacity) || !fmi->bwt ||
        !fmi->occ1 || !fmi->occ2)
        return KISS_HIP_E_INVALID;
    if (all && (!fmi->sa || (fmi->sa_intv != 1 && (!fmi->b || !fmi->b_occ)))) return KISS_HIP_E_INVALID;
    if (all && Q == 0) { // index[0] = 0
        KTRY(fm_enter(ctx, stream));
        KTRY(kiss_zero_u32(ctx, index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
    }
    return fmi_query_mm(ctx, fmi, patterns, L, Q, max_mismatches, counts, positions, mismatches, index, capacity, report, stream);
}

int kiss_hip_fmi_query_mm_host(const kiss_hip_fmi_view *fmi, const uint8_t *patterns, uint32_t L, uint64_t Q,
                               uint32_t max_mismatches, uint32_t *counts, uint32_t *positions, uint8_t *mismatches,
                               uint64_t *index, uint64_t capacity, kiss_hip_fmi_mm_report *report, int device)
{
    if (report) {
        *report = kiss_hip_fmi_mm_report{};
        report->Q = Q;
        report->L = L;
        report->max_mismatches = max_mismatches;
    }
    if (!fmi) return KISS_HIP_E_INVALID;
    const uint32_t sa_intv = fmi->sa_intv;
    if (max_mismatches > KISS_HIP_FMI_MAX_MISMATCHES || !fm_sa_intv_ok(sa_intv)) return KISS_HIP_E_UNSUPPORTED;
    const bool any = positions || mismatches || index, all = positions && mismatches && index;
    if (L == 0 || fmi->n_sa == 0 || (Q && (!patterns || !counts)) || any != all || (!any && capacity) || !fmi->bwt || !fmi->occ1 ||
        !fmi->occ2 || !fmi->sa || (sa_intv != 1 && (!fmi->b || !fmi->b_occ)))
        return KISS_HIP_E_INVALID;
    kiss_hip_fmi_sizes_ex z;
    KTRY(kiss_hip_fmi_sizes_ex_for(fmi->n_sa - 1, sa_intv, 0, &z));
    // (the hits of a call are sorted in the ctx's LMS arrays)
    return kiss_one_shot_own(device, fm_host_max_n(fmi->n_sa, Q, capacity), [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t cnt_bytes = Q * (max_mismatches + 1) * 4;
        FmStage st(ctx);
        const kiss_hip_fmi_view v = fm_upload_index(st, *fmi, z.base);
        const uint8_t *dpat = st.up(patterns, Q * L);
        uint32_t *dcnt = st.room<uint32_t>(true, cnt_bytes);
        uint32_t *dpos = st.room<uint32_t>(all, capacity * 4);
        uint8_t *dmm = st.room<uint8_t>(all, capacity);
        uint64_t *didx = st.room<uint64_t>(all, (Q + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_fmi_mm_report r{};
        const int rc = kiss_hip_fmi_query_mm_dev(ctx, &v, dpat, L, Q, max_mismatches, dcnt, dpos, dmm, didx, all ? capacity : 0, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        uint64_t total = 0;
        for (int j = 0; j < 4; j++) total += r.hits[j];
        st.down(counts, dcnt, cnt_bytes);
        if (all) st.down(index, didx, (Q + 1) * 8);
        if (all) st.down(positions, dpos, total * 4);
        if (all) st.down(mismatches, dmm, total);
        return st.rc;
    });
}

} // extern "C"
