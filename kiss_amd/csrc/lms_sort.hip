// lms_sort.hip -- k-ordered sort of the LMS suffixes (the "far" ones: p + D <= n).
//
// Contract (reference comparator, include/biovoltron/algo/sort/kiss1_core.hpp:94-135, applied after the
// stable 10-mer bucketing of :41-83): for two LMS suffixes that both have D = 125*(k/125+1) bases left
// the order is (first D bases, then text position).  k >= n means the exact suffix order (D unbounded;
// past-the-end bases read as 'A' exactly like the reference's zero padding, structs.hpp:94-96).
//
// GPU formulation: MSD refinement.
//   round 0 : stable LSD radix sort of all suffixes on their first 20 bases (5 passes of 8 bits);
//             suffixes that share those 20 bases form a segment, singletons retire to their final slot.
//             A segment of exactly two -- more than half of what is tied -- leaves the stream there and then as one
//             pair record, decided by one lane's walk to the full depth D (flag_compact.hip: k_fc0_onepass<true>; k_pair_finish).
//   round r : every still-tied suffix fetches its next 32 bases (one u64 key).
//             - a segment of <= SMALL_SEG suffixes is FINISHED on the spot: every suffix is ranked against the
//               others of its segment, first on the fetched key and, for pairs that tie on it, by walking both
//               suffixes to the full depth D (then position).  All of them retire.  (k_small_finish: one launch,
//               the keys stay in LDS, every tied pair is walked once.)
//             - larger segments are compacted and sorted on (segment id, key): from the second refinement round on
//               by a stable three-way split around the key of the segment's middle item (what is left then is
//               mostly long tandem arrays, whose members carry one key per round) followed by a radix sort of the
//               < and > groups only; in the first round by the radix sort directly.  Then they are split where
//               neighbours differ and go round again.
// Every step is stable and the initial order is ascending text position, which yields the reference's
// position tie-break (kiss1_core.hpp:131-133) once the depth D is exhausted.
// The flag + compaction steps that end every round are in flag_compact.hip; the exact-order finish by rank doubling, which
// takes over from this sort in exact order, is in doubling.hip.
#include "flag_compact.hpp"
#include <cstdio>
#include <vector>

using namespace kiss_fc;

namespace {

// the refinement rounds of the LMS sort: measured at chm13 size 8 / 16 / 24 / 64 / 256 -> 83.7 / 83.5 / 83.1 / 85.3 /
// 90.1 ms per sort (KISS_HIP_SMALL_SEG): the all-pairs finish is O(s^2) walks per segment, the pivot rounds are not
constexpr uint32_t LMS_SMALL_SEG = 24;
constexpr int ROUND0_BASES = 20;

// seg / segstart (optional): only members of segments of min_len .. max_len items get a key.  A segment of exactly two is
// compared once by k_seg_finish, walking both suffixes from the segment's depth on, and a segment that goes to a pivot
// round is keyed there against its reference string (k_pivot_lcp): for both the 32-base key would be one more random
// text read per member for nothing (pairs are more than half of what survives round 0 -- the two copies of a duplicated
// stretch --, the big segments most of the rest)
__global__ __launch_bounds__(LS_THREADS) void k_gather_keys(const uint64_t *__restrict__ pk, uint64_t n,
                                                           const uint32_t *__restrict__ pos, uint64_t count,
                                                           uint64_t depth_off, uint64_t mask,
                                                           uint64_t *__restrict__ key, const uint32_t *__restrict__ seg,
                                                           const uint32_t *__restrict__ segstart, uint32_t min_len,
                                                           uint32_t max_len)
{
    uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    if (seg) {
        const uint32_t sg = seg[i];
        const uint32_t len = segstart[sg + 1] - segstart[sg];
        if (len < min_len || len > max_len) return;
    }
    uint64_t q = (uint64_t)pos[i] + depth_off;
    uint64_t k = (q < n) ? kiss_key32(pk, q) : 0ull;
    key[i] = k & mask;
}

// true if suffix pi sorts before suffix pj, both already equal on [0, off + 32); bases from off + 32 on are
// compared up to depth (0 = unbounded), ties go to the smaller index (= smaller text position)
// *tied (optional) is set when the walk reached the depth without a difference: the order then is the tie rule's, and
// both suffixes are tainted for the exact-order finish (KISS_CTX_TAINT)
// (off + 32 = the first base not yet compared: callers that have compared the 32-base key of the round pass `off`,
//  the pair path of k_seg_finish, which has no key, passes off - 32 and lets the walk start at the segment's depth)
__device__ __forceinline__ bool deep_less(const uint64_t *__restrict__ pk, uint64_t n, uint64_t pi, uint64_t pj,
                                          uint64_t off, uint64_t depth, bool i_before_j, bool *tied = nullptr)
{
    uint64_t d = off + 32;
    for (;;) {
        if ((depth && d >= depth) || (pi + d >= n && pj + d >= n)) { // (both off the text: not for two LMS suffixes)
            if (tied) *tied = true;
            return i_before_j;
        }
        uint64_t qi = pi + d, qj = pj + d;
        if (qi + 96 < n && qj + 96 < n && (!depth || depth - d >= 128)) {
            // 128 bases per step: the ten word loads are independent, so one round trip to memory covers four
            // 32-base compares (the walk through a long repeat is a chain of dependent loads otherwise)
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
        if (depth >= 128 && pi + depth <= n && pj + depth <= n) {
            // fewer than 128 bases to go: ONE more step over the last 128 bases of the depth instead of up to four
            // dependent 32-base steps.  It overlaps bases already found equal, which changes nothing: the first
            // differing word still holds the first differing base.
            const uint64_t ri = pi + depth - 128, rj = pj + depth - 128;
            const uint32_t si = 2u * (uint32_t)(ri & 31u), sj = 2u * (uint32_t)(rj & 31u);
            uint64_t a[5], b[5];
            kiss_words5(pk, ri >> 5, a);
            kiss_words5(pk, rj >> 5, b);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint64_t ki = (a[t] << si) | ((a[t + 1] >> 1) >> (63u - si));
                const uint64_t kj = (b[t] << sj) | ((b[t + 1] >> 1) >> (63u - sj));
                if (ki != kj) return ki < kj;
            }
            if (tied) *tied = true;
            return i_before_j;
        }
        uint64_t ki = qi < n ? kiss_key32(pk, qi) : 0ull;
        uint64_t kj = qj < n ? kiss_key32(pk, qj) : 0ull;
        if (depth && depth - d < 32) {
            uint64_t mask = ~0ull << (64 - 2 * (depth - d));
            ki &= mask;
            kj &= mask;
        }
        if (ki != kj) return ki < kj;
        d += 32;
    }
}

// (k_seg_adjacent and k_seg_finish: the three-kernel form of the small-segment finish, behind k_gather_keys.  The sort
//  runs k_small_finish below instead; the hooks build keeps this form as its A-B arm, KISS_HIP_NO_SMALL_FUSED, and for
//  other thresholds than LMS_SMALL_SEG.)
// phase A for small segments of >= 3 members: is my successor in the segment not smaller than me?
// (a segment whose adjacent pairs are all in order is already sorted: the common case for periodic repeats,
//  where all-pairs ranking would walk s^2 pairs to the full depth)
__global__ __launch_bounds__(LS_THREADS) void k_seg_adjacent(const uint64_t *__restrict__ pk, uint64_t n,
                                                            const uint64_t *__restrict__ key,
                                                            const uint32_t *__restrict__ pos,
                                                            const uint32_t *__restrict__ seg,
                                                            const uint32_t *__restrict__ segstart, uint64_t count,
                                                            uint64_t off, uint64_t depth, uint32_t small_seg,
                                                            uint8_t *__restrict__ inorder)
{
    uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint32_t sg = seg[i];
    const uint32_t a = segstart[sg], b = segstart[sg + 1];
    const uint32_t len = b - a;
    if (len < 3 || len > small_seg) return;
    uint8_t ok = 1; // 0: my successor is smaller, 1: in order, 2: in order by the tie rule (equal through the depth)
    if ((uint32_t)i + 1 < b) {
        const uint64_t ki = key[i], kn = key[i + 1];
        if (kn != ki) ok = kn > ki;
        else {
            bool tied = false;
            ok = !deep_less(pk, n, pos[i + 1], pos[i], off, depth, false, &tied);
            if (tied) ok = 2;
        }
    }
    inorder[i] = ok;
}

// small segments: final rank of every member, written straight to its final slot;
// big segments: flagged for the radix path.  big[i] = 0: finished here, 1: member of a big segment, 3: its first member
// (one byte per item since round 4: k_bigb_count / k_bigb_compact below count and compact them tile by tile; the
//  8-byte flag words of rounds 1-3 went through a full scan, 5 GB of traffic for 35 M big-segment items)
__global__ __launch_bounds__(LS_THREADS) void k_seg_finish(const uint64_t *__restrict__ pk, uint64_t n,
                                                          const uint64_t *__restrict__ key,
                                                          const uint32_t *__restrict__ pos,
                                                          const uint32_t *__restrict__ slot,
                                                          const uint32_t *__restrict__ seg,
                                                          const uint32_t *__restrict__ segstart, uint64_t count,
                                                          uint64_t off, uint64_t depth, uint32_t small_seg,
                                                          const uint8_t *__restrict__ inorder,
                                                          uint32_t *__restrict__ out, uint8_t *__restrict__ big,
                                                          uint32_t *__restrict__ nbig,
                                                          const uint32_t *__restrict__ tctx, // first round only: the
                                                          uint32_t *__restrict__ octx,       // items' context words
                                                          uint8_t *__restrict__ hfar) // optional: 0 for an item that retires
                                                          // tied with the one before it in the final order (ctx->hfar)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    const bool valid = i < count;
    uint32_t a = 0, b = 0;
    if (valid) {
        const uint32_t sg = seg[i];
        a = segstart[sg];
        b = segstart[sg + 1];
    }
    const bool small = valid && (b - a <= small_seg);
    // a pair (by far the most common tied segment: two copies of a repeat) is compared once: its first member walks
    // the two suffixes, the second one -- the next lane -- takes the opposite rank
    const bool second_in_wave = small && (b - a == 2) && ((uint32_t)i == a + 1) && lane_id() > 0;
    uint32_t r = 0;
    uint64_t pi = 0;
    // taint (KISS_CTX_TAINT): this item is tied with another one through the full depth (a walk of deep_less, here or in
    // k_seg_adjacent, ended without a difference): its place among its mates is the tie rule's
    bool taint = false;
    bool tied_before = false; // tied with a mate that precedes it in the final order (position order among mates)
    if (small) {
        pi = pos[i];
        if (!second_in_wave && b - a == 2) {
            // a pair: no keys were gathered for it (k_gather_keys); one walk from the segment's depth decides
            const uint32_t j = (uint32_t)i == a ? a + 1 : a;
            r = deep_less(pk, n, pos[j], pi, off - 32, depth, j < (uint32_t)i, &taint) ? 1u : 0u;
        } else if (!second_in_wave) {
            const uint64_t ki = key[i];
            bool sorted = false;
            if (b - a >= 3) { // adjacent pairs all in order -> already sorted
                sorted = true;
                for (uint32_t j = a; j + 1 < b; j++) sorted = sorted && inorder[j];
            }
            if (sorted) {
                r = (uint32_t)i - a;
                tied_before = (uint32_t)i > a && inorder[i - 1] == 2;
                taint = tied_before || ((uint32_t)i + 1 < b && inorder[i] == 2);
            } else {
                for (uint32_t j = a; j < b; j++) {
                    if (j == (uint32_t)i) continue;
                    uint64_t kj = key[j];
                    bool jless;
                    if (kj != ki) jless = kj < ki;
                    else {
                        bool tj = false;
                        jless = deep_less(pk, n, pos[j], pi, off, depth, j < (uint32_t)i, &tj);
                        taint = taint || tj;
                        tied_before = tied_before || (tj && jless);
                    }
                    r += jless ? 1u : 0u;
                }
            }
        }
    }
    const uint32_t r_prev = __shfl_up(r, 1, 64);
    const bool t_prev = __shfl_up((int)taint, 1, 64) != 0;
    if (second_in_wave) {
        r = 1u - r_prev;
        taint = t_prev; // the pair's first member did the comparison
    }
    if (small && b - a == 2) tied_before = taint && r == 1;
    if (small) {
        const uint32_t dst = slot[a + r];
        out[dst] = (uint32_t)pi;
        if (hfar && tied_before) hfar[dst] = 0;
        // the context word a finished item brought along from round 0 (key payload) spares the placement step a
        // random text gather; items that stay tied past this round get theirs gathered there (and are tainted there)
        if (tctx) octx[dst] = tctx[i] | (taint ? KISS_CTX_TAINT : 0u);
        else if (taint) octx[dst] = KISS_CTX_TAINT; // no word yet (gathered at placement), but tainted
        big[i] = 0;
    } else if (valid) {
        big[i] = (uint32_t)i == a ? (uint8_t)3 : (uint8_t)1;
    }
    (void)nbig; // the number of big-segment items comes out of the flag scan (one address hit by every wave's
                // atomicAdd cost more than the rest of this kernel)
}

// ---- k_gather_keys (small segments) + k_seg_adjacent + k_seg_finish in one kernel -----------------------------------
// A workgroup owns SF_THREADS consecutive stream items and also loads the SF_HALO items on either side, so every segment of
// <= LMS_SMALL_SEG members that has a member in the block lies in LDS as a whole (a segment that crosses the block's edge
// is done by both blocks, each storing its own members).  Per window item LDS holds the position, the round's key (never
// written to memory), the segment bounds and what the walks found:
//     inorder[w]    the pair (w, w + 1), as k_seg_adjacent: 0 successor smaller, 1 in order, 2 in order by the tie rule
//     before[w]     bit d: w sorts before its mate w + d        tiedm[w]  bit d: ... and the two are tied through the depth
// The key-tied pairs are put on a list in LDS and the block's lanes walk them list entry by list entry -- every unordered
// pair ONCE (k_seg_finish walked it from both sides, and k_seg_adjacent a third time if it was adjacent) and without the
// idle lanes of one-lane-per-item: first the adjacent pairs; only a segment that these do not show to be in order lists
// its other tied pairs.  A rank then is a count over the mates' bits.  A segment of two (no key: it is walked from the
// segment's depth) is an adjacent pair like the others.  Every thread reaches every barrier.
constexpr int SF_THREADS = LS_THREADS;
constexpr int SF_HALO = (int)LMS_SMALL_SEG - 1;
constexpr int SF_WINDOW = SF_THREADS + 2 * SF_HALO;
constexpr int SF_PAIRS_CAP = SF_WINDOW * ((int)LMS_SMALL_SEG - 2); // an item lists its pairs with the mates >= 2 places on
static_assert(LMS_SMALL_SEG <= 32 && SF_WINDOW <= 512 && 2 * SF_HALO <= SF_THREADS, "bit masks per item, 9 + 5 bit list entries");

// the window items a lane loads: its own item of the block, and (the first 2 * SF_HALO lanes) one item of the halo
__device__ __forceinline__ int sf_window_item(int tid, int t)
{
    if (t == 0) return tid + SF_HALO;
    return tid < SF_HALO ? tid : (tid < 2 * SF_HALO ? tid + SF_THREADS : -1);
}

__global__ __launch_bounds__(SF_THREADS) void k_small_finish(const uint64_t *__restrict__ pk, uint64_t n,
                                                            const uint32_t *__restrict__ pos,
                                                            const uint32_t *__restrict__ slot,
                                                            const uint32_t *__restrict__ seg,
                                                            const uint32_t *__restrict__ segstart, uint32_t count,
                                                            uint64_t off, uint64_t depth, uint64_t mask,
                                                            uint32_t *__restrict__ out, uint8_t *__restrict__ big,
                                                            const uint32_t *__restrict__ tctx, // first round only: the
                                                            uint32_t *__restrict__ octx,       // items' context words
                                                            uint8_t *__restrict__ hfar)        // as k_seg_finish
{
    __shared__ uint64_t s_key[SF_WINDOW];
    __shared__ uint32_t s_pos[SF_WINDOW];
    __shared__ int32_t s_a[SF_WINDOW], s_b[SF_WINDOW]; // segment bounds as window indices; s_b = 0: not an item of a small
                                                       // segment that this block finishes
    __shared__ uint32_t s_before[SF_WINDOW], s_tiedm[SF_WINDOW];
    __shared__ uint8_t s_inorder[SF_WINDOW], s_unsorted[SF_WINDOW];
    __shared__ uint16_t s_adj[SF_WINDOW];     // list of adjacent pairs to walk: w
    __shared__ uint16_t s_far[SF_PAIRS_CAP];  // list of the other pairs to walk: w | d << 9
    __shared__ uint32_t s_nadj, s_nfar;

    const int tid = (int)threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * SF_THREADS - SF_HALO; // stream index of window item 0
    if (tid == 0) s_nadj = s_nfar = 0;
    // ---- the window: positions, segment bounds, keys
    uint32_t my_a = 0, my_len = 0; // of this lane's own item (window index tid + SF_HALO); my_len = 0: past the end
    // (the first 2 * SF_HALO lanes load a second item: both chains seg -> segstart -> key are issued together)
    bool valid[2];
    uint32_t sgv[2] = {0, 0}, pv[2] = {0, 0}, av[2] = {0, 0}, bv[2] = {0, 0};
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int w = sf_window_item(tid, t);
        const int64_t g = g0 + w;
        valid[t] = w >= 0 && g >= 0 && g < (int64_t)count;
        if (valid[t]) {
            sgv[t] = seg[g];
            pv[t] = pos[g];
        }
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
        if (valid[t]) {
            av[t] = segstart[sgv[t]];
            bv[t] = segstart[sgv[t] + 1];
        }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int w = sf_window_item(tid, t);
        if (w < 0) continue;
        const bool own = t == 0;
        int32_t wa = 0, wb = 0;
        uint32_t p = 0;
        uint64_t key = 0;
        if (valid[t]) {
            const uint32_t a = av[t], b = bv[t], len = b - a;
            if (own) {
                my_a = a;
                my_len = len;
            }
            // (a halo item counts only as a mate of an item of the block)
            if (len <= LMS_SMALL_SEG && (int64_t)b > g0 + SF_HALO && (int64_t)a < g0 + SF_HALO + SF_THREADS) {
                wa = (int32_t)((int64_t)a - g0);
                wb = (int32_t)((int64_t)b - g0);
                p = pv[t];
                if (len >= 3) { // as k_gather_keys
                    const uint64_t q = (uint64_t)p + off;
                    key = (q < n ? kiss_key32(pk, q) : 0ull) & mask;
                }
            }
        }
        s_a[w] = wa;
        s_b[w] = wb;
        s_pos[w] = p;
        s_key[w] = key;
        s_before[w] = 0;
        s_tiedm[w] = 0;
        s_inorder[w] = 1;
        s_unsorted[w] = 0;
    }
    __syncthreads();
    // ---- adjacent pairs: decided by the key, or listed for a walk
    for (int w = tid; w < SF_WINDOW; w += SF_THREADS) {
        if (w + 1 < s_b[w]) {
            const uint64_t ki = s_key[w], kn = s_key[w + 1];
            if (kn != ki) s_inorder[w] = kn > ki ? 1 : 0;
            else s_adj[atomicAdd(&s_nadj, 1u)] = (uint16_t)w;
        }
    }
    __syncthreads();
    const int nadj = (int)s_nadj;
    for (int e = tid; e < nadj; e += SF_THREADS) {
        const int w = s_adj[e];
        const bool pair = s_b[w] - s_a[w] == 2; // no key was compared: the walk starts at the segment's depth
        bool tied = false;
        const bool ok = !deep_less(pk, n, s_pos[w + 1], s_pos[w], pair ? off - 32 : off, depth, false, &tied);
        s_inorder[w] = tied ? 2 : (ok ? 1 : 0);
    }
    __syncthreads();
    // ---- a segment with an adjacent pair out of order: every pair of it counts.  Item w decides its pairs with the mates
    // behind it: by the key, from the adjacent walk, or it lists them for a walk
    for (int w = tid; w < SF_WINDOW; w += SF_THREADS) {
        const int wa = s_a[w], wb = s_b[w];
        bool sorted = true;
        for (int j = wa; j + 1 < wb; j++) sorted = sorted && s_inorder[j] != 0;
        if (sorted) continue;
        s_unsorted[w] = 1;
        const bool own = w >= SF_HALO && w < SF_HALO + SF_THREADS;
        const uint64_t ki = s_key[w];
        uint32_t before = 0, walk = 0;
        for (int j = w + 1; j < wb; j++) {
            const uint64_t kj = s_key[j];
            const uint32_t bit = 1u << (j - w);
            if (kj != ki) before |= ki < kj ? bit : 0u;
            else if (j == w + 1) before |= s_inorder[w] ? bit : 0u;
            else if (own || (j >= SF_HALO && j < SF_HALO + SF_THREADS)) walk |= bit; // (two halo items: nobody asks)
        }
        s_before[w] = before;
        if (s_inorder[w] == 2) s_tiedm[w] = 2u;
        if (walk) {
            uint32_t at = atomicAdd(&s_nfar, (uint32_t)__popc(walk));
            while (walk) {
                const int d = __ffs(walk) - 1;
                walk &= walk - 1;
                s_far[at++] = (uint16_t)(w | (d << 9));
            }
        }
    }
    __syncthreads();
    const int nfar = (int)s_nfar;
    for (int e = tid; e < nfar; e += SF_THREADS) {
        const int w = s_far[e] & 511, d = s_far[e] >> 9;
        bool tied = false;
        const bool first = deep_less(pk, n, s_pos[w], s_pos[w + d], off, depth, true, &tied);
        if (first) atomicOr(&s_before[w], 1u << d);
        if (tied) atomicOr(&s_tiedm[w], 1u << d);
    }
    __syncthreads();
    // ---- ranks and stores, one lane per item of the block
    const int w = tid + SF_HALO;
    const uint32_t i = (uint32_t)(g0 + w);
    if (my_len == 0) return; // past the end of the stream (after the last barrier)
    if (my_len > LMS_SMALL_SEG) {
        big[i] = i == my_a ? (uint8_t)3 : (uint8_t)1;
        return;
    }
    const int wa = s_a[w], wb = s_b[w];
    uint32_t r;
    bool taint, tied_before;
    if (!s_unsorted[w]) {
        r = (uint32_t)(w - wa);
        tied_before = w > wa && s_inorder[w - 1] == 2;
        taint = tied_before || (w + 1 < wb && s_inorder[w] == 2);
    } else {
        const uint32_t behind = (2u << (wb - 1 - w)) - 2u; // bits 1 .. wb - 1 - w: my mates behind me
        r = (uint32_t)__popc(~s_before[w] & behind);
        taint = s_tiedm[w] != 0;
        tied_before = false;
        for (int j = wa; j < w; j++) {
            r += (s_before[j] >> (w - j)) & 1u;
            tied_before = tied_before || ((s_tiedm[j] >> (w - j)) & 1u);
        }
        taint = taint || tied_before;
    }
    const uint32_t dst = slot[my_a + r];
    out[dst] = s_pos[w];
    if (hfar && tied_before) hfar[dst] = 0;
    if (tctx) octx[dst] = tctx[i] | (taint ? KISS_CTX_TAINT : 0u);
    else if (taint) octx[dst] = KISS_CTX_TAINT;
    big[i] = 0;
}

// the pairs that k_fc0_onepass took out of the survivor stream, one lane per record: what the pair path of k_seg_finish
// does, without the seg -> segstart -> pos[mate] -> slot chain.  The list still holds the two members in position order
// (out[slot] = p0, out[slot + 1] = p1) and octx their context words, so only what changes is stored: a pair that swaps,
// a taint bit.
__global__ __launch_bounds__(LS_THREADS) void k_pair_finish(const uint64_t *__restrict__ pk, uint64_t n,
                                                           const uint32_t *__restrict__ rpos0,
                                                           const uint32_t *__restrict__ rpos1,
                                                           const uint32_t *__restrict__ rslot, uint64_t npairs,
                                                           uint64_t off, uint64_t depth, uint32_t *__restrict__ out,
                                                           uint32_t *__restrict__ octx, uint8_t *__restrict__ hfar)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= npairs) return;
    const uint32_t p0 = rpos0[i], p1 = rpos1[i], s = rslot[i];
    bool taint = false;
    // the first member's walk in k_seg_finish: is the second member smaller?  (tied through the depth: no, position order)
    const bool swap = deep_less(pk, n, p1, p0, off - 32, depth, false, &taint);
    if (!swap && !taint) return;
    const uint32_t c0 = octx[s], c1 = octx[s + 1];
    const uint32_t t = taint ? KISS_CTX_TAINT : 0u;
    if (swap) {
        out[s] = p1;
        out[s + 1] = p0;
    }
    octx[s] = (swap ? c1 : c0) | t;
    octx[s + 1] = (swap ? c0 : c1) | t;
    if (hfar && taint) hfar[s + 1] = 0; // the member in the second slot is tied with the one before it
}

// ---- big segments: three-way split around a pivot key before any radix pass ---------------------------------
// The members of a long tandem array stay tied round after round: most of a big segment carries ONE key (the
// unmutated continuation of the repeat) and only the items whose 32-base window holds a mutation differ.  Sorting
// such a segment on (segment, key) costs 8 + 3 radix passes over all of it.  Instead: pivot = the key of the
// segment's middle item; a stable segmented partition into < pivot | == pivot | > pivot (one scan, one scatter);
// only the < and > groups -- now segments of their own -- go through the radix sort.  The result is the same
// (segment, key) order.  cls[i] = [key < pivot] | [key == pivot] << 32.
__device__ __forceinline__ uint32_t pivot_class(const uint64_t *__restrict__ bkey, uint32_t a, uint32_t b, uint64_t k)
{
    const uint64_t pv = bkey[(a + b) >> 1];
    return k < pv ? 0u : (k == pv ? 1u : 2u);
}

__global__ __launch_bounds__(LS_THREADS) void k_pivot_class(const uint64_t *__restrict__ bkey,
                                                           const uint32_t *__restrict__ bseg,
                                                           const uint32_t *__restrict__ bsegstart, uint64_t nbig,
                                                           uint64_t *__restrict__ cls)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= nbig) return;
    const uint32_t sid = bseg[i];
    const uint32_t c = pivot_class(bkey, bsegstart[sid], bsegstart[sid + 1], bkey[i]);
    cls[i] = c == 0 ? 1ull : (c == 1 ? (1ull << 32) : 0ull);
}

// ex = exclusive scan of cls, tot[0] = its grand total.  Items move inside their segment; ne[d] flags the members of
// the < and > groups at their new place: (1 << 32) | starts-a-group.
__global__ __launch_bounds__(LS_THREADS) void k_pivot_scatter(const uint64_t *__restrict__ bkey,
                                                             const uint32_t *__restrict__ bpos,
                                                             const uint32_t *__restrict__ bseg,
                                                             const uint32_t *__restrict__ bsegstart, uint64_t nbig,
                                                             const uint64_t *__restrict__ cls,
                                                             const uint64_t *__restrict__ ex,
                                                             const uint64_t *__restrict__ tot,
                                                             uint64_t *__restrict__ okey, uint32_t *__restrict__ opos,
                                                             uint64_t *__restrict__ ne)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= nbig) return;
    const uint32_t sid = bseg[i];
    const uint32_t a = bsegstart[sid], b = bsegstart[sid + 1];
    const uint64_t ea = ex[a], eb = (uint64_t)b < nbig ? ex[b] : tot[0], ei = ex[i], ci = cls[i];
    const uint32_t t0 = (uint32_t)eb - (uint32_t)ea, t1 = (uint32_t)(eb >> 32) - (uint32_t)(ea >> 32);
    const uint32_t lt_before = (uint32_t)ei - (uint32_t)ea, eq_before = (uint32_t)(ei >> 32) - (uint32_t)(ea >> 32);
    const uint32_t c = (uint32_t)ci ? 0u : ((ci >> 32) ? 1u : 2u);
    uint32_t d;
    if (c == 0) d = a + lt_before;
    else if (c == 1) d = a + t0 + eq_before;
    else d = a + t0 + t1 + ((uint32_t)i - a - lt_before - eq_before);
    okey[d] = bkey[i];
    opos[d] = bpos[i];
    uint64_t f = 0;
    if (c == 0) f = (1ull << 32) | (uint64_t)(d == a ? 1u : 0u);
    else if (c == 2) f = (1ull << 32) | (uint64_t)(d == a + t0 + t1 ? 1u : 0u);
    ne[d] = f;
}

// ---- pivot rounds: the members of a big segment against one reference string, to the full depth -------------------------------------
// What is still tied in big segments after two rounds is long tandem arrays (and the odd high-copy repeat).  Their
// members stay tied round after round -- eleven more 32-base rounds of ~40 launches and an 8 + 2-pass radix sort each at
// D = 375 -- although one comparison says almost everything: every member is compared with ONE reference string (the
// segment's consensus, see k_pivot_lcp) from the current depth to the full depth D, giving
//     side = member < reference | equal through D | member > reference,   d = first differing base,   c = the member's base there.
// Two members on the < side order by (d ascending, c); on the > side by (d descending, c); members equal through D
// are final in their present (= text position) order.  One stable radix sort on (segment, side, d', c) -- 13 bits + the
// segment id at k = 256 -- replaces the rounds.  Members with the same (side, d, c) are tied through off + d + 1 bases:
// they form a new, much smaller segment that goes round again from the SAME depth `off` (so all survivors still share
// one depth; the few bases they walk twice cost less than a per-segment depth would).  Progress: if every member of a
// segment fell into the same (side, d, c) class, the three members the reference is made of would all carry base c at
// d, and so would the reference -- so a segment always splits into at least two classes or retires as a whole.
// Bounded depth only: in exact order (D unbounded) "equal through D" does not exist, the 32-base rounds run instead.

__device__ __forceinline__ uint64_t maj3(uint64_t a, uint64_t b, uint64_t c) { return (a & b) | (a & c) | (b & c); }

// Key of a member: up to `slots` deviations from the reference, most significant first, then a "complete" bit:
//     [side:2 | d':dbits | c:2] x slots ... [complete:1]          in the TOP bits of a 64-bit word
// side 0: the member's base is smaller than the reference's at d (d' = d: the earlier the deviation, the smaller the
// member), side 2: larger (d' = rem - 1 - d: the earlier, the larger), side 1: no further deviation through the depth
// (terminator; the walk is complete and the key says everything the comparator can see).  Members that are equal up to
// and including a deviation keep following the same argument from the next base on, so the slots compare
// lexicographically.  After a substitution a tandem array is back in phase with its consensus, so the next slot holds
// the member's next mutation: one round looks `slots` mutations deep.
__global__ __launch_bounds__(LS_THREADS) void k_pivot_lcp(const uint64_t *__restrict__ pk,
                                                         const uint32_t *__restrict__ bpos,
                                                         const uint32_t *__restrict__ bseg,
                                                         const uint32_t *__restrict__ bsegstart, uint64_t nbig,
                                                         uint64_t off, uint64_t depth, int dbits, int slots,
                                                         uint64_t *__restrict__ keyout, int frac_den, int with_ctx)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= nbig) return;
    const uint32_t sid = bseg[i];
    const uint32_t a = bsegstart[sid], b = bsegstart[sid + 1], len = b - a;
    // The reference the members are compared with may be ANY fixed string (the order argument only needs it to be the
    // same for the whole segment).  A real member carries its own mutations, and everything that follows the consensus
    // up to that member's first mutation would land in one class.  The bitwise majority of three members is the
    // consensus wherever at most one of them is mutated: members of a tandem array then deviate from the reference at
    // their OWN mutations.
    const uint64_t p = (uint64_t)bpos[i] + off;
    // Which three: the quarters of the segment in one round, 2/7 4/7 5/7 in the next, 3/11 5/11 8/11 in the third, and
    // round again -- arrays of equal length (telomeres) put the quarters of a segment exactly at array ends, where
    // members stop following the consensus; the next round then picks elsewhere.
    const uint64_t f1 = frac_den == 4 ? 1 : (frac_den == 7 ? 2 : 3), f2 = frac_den == 4 ? 2 : (frac_den == 7 ? 4 : 5),
                   f3 = frac_den == 4 ? 3 : (frac_den == 7 ? 5 : 8);
    const uint64_t q1 = (uint64_t)bpos[a + (uint32_t)(((uint64_t)len * f1) / (uint64_t)frac_den)] + off,
                   q2 = (uint64_t)bpos[a + (uint32_t)(((uint64_t)len * f2) / (uint64_t)frac_den)] + off,
                   q3 = (uint64_t)bpos[a + (uint32_t)(((uint64_t)len * f3) / (uint64_t)frac_den)] + off;
    const uint64_t rem = depth - off; // all of them are far suffixes: position + rem lies inside the text
    const int slotbits = dbits + 4;
    uint64_t key = 0;
    int used = 0;
    bool complete = false;
    auto take = [&](uint64_t kx, uint64_t kr, uint64_t base0) { // deviations inside one 32-base word, in text order
        uint64_t diff = kx ^ kr;
        diff = (diff | (diff >> 1)) & 0x5555555555555555ull; // one flag per base (its low bit)
        while (diff && used < slots) {
            const uint32_t lz = (uint32_t)__clzll((long long)diff) >> 1; // base index inside the word
            const uint32_t sh = 62u - 2u * lz;
            const uint64_t cx = (kx >> sh) & 3ull, cr = (kr >> sh) & 3ull;
            const uint64_t d = base0 + lz;
            const uint64_t side = cx < cr ? 0ull : 2ull;
            const uint64_t dk = side == 0 ? d : rem - 1 - d;
            key = (key << slotbits) | (side << (dbits + 2)) | (dk << 2) | cx;
            used++;
            diff &= ~(1ull << sh);
        }
    };
    uint64_t done = 0;
    while (done < rem && used < slots) {
        if (rem - done >= 128) { // four words per step: the loads of one step are independent (one round trip to memory)
            uint64_t kx[4], k1[4], k2[4], k3[4];
            keys128(pk, p + done, kx);
            keys128(pk, q1 + done, k1);
            keys128(pk, q2 + done, k2);
            keys128(pk, q3 + done, k3);
#pragma unroll
            for (int t = 0; t < 4; t++) take(kx[t], maj3(k1[t], k2[t], k3[t]), done + 32u * (uint32_t)t);
            done += 128;
            continue;
        }
        uint64_t ki = kiss_key32(pk, p + done);
        uint64_t kr = maj3(kiss_key32(pk, q1 + done), kiss_key32(pk, q2 + done), kiss_key32(pk, q3 + done));
        if (rem - done < 32) {
            const uint64_t mask = ~0ull << (64 - 2 * (rem - done));
            ki &= mask;
            kr &= mask;
        }
        take(ki, kr, done);
        done += 32;
    }
    if (used < slots) { // the walk reached the depth: terminator slot, the key is complete
        key = (key << slotbits) | (1ull << (dbits + 2));
        used++;
        complete = true;
    }
    key <<= (uint64_t)slotbits * (uint64_t)(slots - used); // unused slots: zeros (only behind a terminator)
    key = (key << 1) | (complete ? 1ull : 0ull);
    // The low 24 bits of the word are not sorted on (with_ctx: the key ends at bit 24 or above) and carry the member's
    // short context word, like the low bits of a round-0 key: a member that retires in this round gets its word without
    // the random text gather of the induction (the bases in front of the member sit in the sector this walk has read)
    keyout[i] = (key << (64 - (slots * slotbits + 1))) | (with_ctx ? (uint64_t)kiss_load_ctx_n(pk, bpos[i], KISS_KEY_CTX_BASES) : 0ull);
}

// boundaries of the new segments in the sorted list: one byte per item, 1 = (segment, key) differs from the predecessor's,
// or the item's key is complete (it says everything the comparator sees: the item is final where the stable sort left it;
// it and its successor both start a "segment", which makes it a singleton for the compaction)
__global__ __launch_bounds__(LS_THREADS) void k_pivot_heads(const uint64_t *__restrict__ key,
                                                           const uint32_t *__restrict__ seg, uint64_t nbig,
                                                           int complete_bit, uint8_t *__restrict__ heads,
                                                           uint64_t cmp_mask) // the key bits (a payload may sit below them)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= nbig) return;
    const uint64_t k = key[i] & cmp_mask;
    const bool complete = ((k >> complete_bit) & 1ull) != 0;
    const bool same_prev = i > 0 && seg[i] == seg[i - 1] && (key[i - 1] & cmp_mask) == k;
    uint8_t h = 1;
    if (same_prev && !complete) h = 0;
    // bit 1: a complete key shared with a neighbour = equal through the full depth: final here by the tie rule (taint)
    if (complete && (same_prev || (i + 1 < nbig && seg[i + 1] == seg[i] && (key[i + 1] & cmp_mask) == k))) h |= 2;
    if (complete && same_prev) h |= 4; // bit 2: ... and that neighbour is the predecessor (ctx->hfar)
    heads[i] = h;
}

// kiss_load_ctx_n gathers context words of two lengths: KISS_KEY_CTX_BASES for the pivot key above, KISS_CTX_BASES where an
// item retires (k_fc_compact, flag_compact.hip).  In a unit that passes it ONE length the optimiser folds that length into the
// helper before it inlines it, and k_pivot_lcp comes out with 88 registers instead of the 78 it had, and was measured with,
// while both callers were one unit.  This kernel is never launched; it is the second caller, and keeps k_pivot_lcp's code
// what it was.  (tools/kernel_diff.py shows the difference when it goes.)
__global__ void k_ctx_lengths_anchor(const uint64_t *pk, uint32_t *out)
{
    out[threadIdx.x] = kiss_load_ctx(pk, out[threadIdx.x + 64]);
}

// ---- the driver: stages over one state --------------------------------------------------------------------------------

// Every work array of the ctx that the sort uses under another name, with the time each name is live.  Built before round 0
// and again whenever the tied-segment arrays have been regrown (flags, bslot, segB and segstartB move then).
struct LmsViews {
    // keyA: the pair records of round 0 (three columns of rcol words: a pair is two items, so count / 2 records at most fit
    // its 2 count words) from the one-pass compaction until k_pair_finish has read them; then K1, the keys of a round
    uint32_t *rpos0, *rpos1, *rslot;
    uint64_t rcol;
    uint64_t *K1;
    // keyB: round 0's sorted keys until its compaction; then the second key buffer of the pivot and class-split sorts
    uint64_t *key2;
    // flags, 2 t_cap words.  F1: tile counts and their scan, the class words of a split.  F2: scans of per-item words; from
    // the small-segment step to the big-segment compaction of a round its bytes are `inorder` and, behind them, `bigb`
    // (round_of).  The last nbig words: NE, the flags of the < and > members of a class split (class_split_flags).
    uint64_t *F1, *F2;
    // segB (second segment column of the doubling forms): the head bytes of a pivot round, the second segment column of a
    // class split's sort.  segstartB: the start of every big segment in the compact arrays (+ end entry)
    uint8_t *pivot_heads;
    uint32_t *seg2, *bss;
    // lmsP / lmsC (the merged list: written by the placement step, after the sort): positions of a class split's sort
    uint32_t *sortpos[2];
    // bslot: the tied items' context words from round 0's compaction to the small-segment step of the first refinement
    // round; from that round's big-segment compaction on the slots of the big-segment items
    uint32_t *tctx, *bslot;
    // d_small + 2: the totals a count leaves (two words; four after the one-pass round 0); + 8: the word the end-entry
    // kernel zeroes (k_seg_finish's unused counter); + 24: the grand total of a split's class counts
    uint64_t *d_total, *d_ptot;
    uint32_t *d_nbig;
};

LmsViews views_of(kiss_hip_ctx *ctx)
{
    LmsViews v;
    v.rcol = (ctx->m_far / 2 + 4) & ~3ull;
    v.rpos0 = reinterpret_cast<uint32_t *>(ctx->keyA);
    v.rpos1 = v.rpos0 + v.rcol;
    v.rslot = v.rpos1 + v.rcol;
    v.K1 = ctx->keyA;
    v.key2 = ctx->keyB;
    v.F1 = ctx->flags;
    v.F2 = ctx->flags + ctx->t_cap;
    v.pivot_heads = reinterpret_cast<uint8_t *>(ctx->segB);
    v.seg2 = ctx->segB;
    v.bss = ctx->segstartB;
    v.sortpos[0] = ctx->lmsP;
    v.sortpos[1] = ctx->lmsC;
    v.tctx = v.bslot = ctx->bslot;
    v.d_total = reinterpret_cast<uint64_t *>(ctx->d_small + 2);
    v.d_nbig = ctx->d_small + 8;
    v.d_ptot = reinterpret_cast<uint64_t *>(ctx->d_small + 24);
    return v;
}

struct LmsSort {
    kiss_hip_ctx *ctx;
    uint64_t n, depth;
    // the options, resolved
    bool dbg;
    bool pivot_on;     // (hooks build: off = 32-base rounds only)
    bool pivot_r1;     // from the first refinement round on; off keeps that one in the 32-base form (hooks build)
    int pivot_slots;   // deviations recorded per member and round: 3 (the hooks build can sweep 1 .. 8)
    bool no_pair_keys;
    uint32_t small_seg;
    bool small_fused;  // k_small_finish is compiled for LMS_SMALL_SEG (its halo and its bit masks)
    LmsViews v;
    // the survivors: positions, slots, segment ids, segment starts; how many in how many segments; tied through `off` bases
    uint32_t *Pc, *Sc, *Gc, *SSc;
    uint64_t count, nseg;
    uint64_t off = ROUND0_BASES;
    uint64_t npairs = 0;       // pairs that left round 0 as records
    bool have_tctx = false;    // v.tctx holds the survivors' context words ...
    bool first_refine = true;  // ... which are only good for the first pass over them
    unsigned pivot_rounds_done = 0;

    FcOut survivors() const { return FcOut{Pc, Sc, Gc, SSc}; }
    void take_tied_arrays() // (at the start, and after kiss_tied_reserve)
    {
        Sc = ctx->slotA;
        Gc = ctx->segA;
        SSc = ctx->segstartA;
        v = views_of(ctx);
    }
    void set_survivors(uint64_t tot)
    {
        count = tot >> 32;
        nseg = tot & 0xFFFFFFFFull;
    }
};

// what a refinement round works out from the depth before it starts
struct Round {
    uint64_t mask;  // of the bases of the round's key that count
    int key_lo_bit;
    bool last_round, pivot_ahead;
    unsigned grid;
    uint8_t *inorder, *bigb; // bytes of F2, see LmsViews
};

Round round_of(const LmsSort &s)
{
    Round r;
    uint64_t rem = s.depth ? s.depth - s.off : 32;
    if (rem > 32) rem = 32;
    r.last_round = s.depth ? (s.off + 32 >= s.depth) : false;
    r.mask = rem >= 32 ? ~0ull : (~0ull << (64 - 2 * rem));
    r.key_lo_bit = (int)(64 - 2 * rem);
    r.grid = (unsigned)div_up(s.count, LS_THREADS);
    // big segments need the round's key only where they are radix sorted on it (no pivot round ahead)
    r.pivot_ahead = s.depth && (s.off > ROUND0_BASES || s.pivot_r1) && s.pivot_on;
    r.inorder = reinterpret_cast<uint8_t *>(s.v.F2);
    r.bigb = r.inorder + ((s.count + 15) & ~15ull);
    return r;
}

// the tied-segment arrays hold fewer than the `surv` tied suffixes of round 0: regrow them (empty so far)
int regrow_tied(LmsSort &s, uint64_t surv)
{
    KTRY(kiss_tied_reserve(s.ctx, surv + surv / 8 + 1024));
    s.take_tied_arrays();
    return KISS_HIP_OK;
}

// ---- round 0: radix sort on the first 20 bases, then flag + compact in one pass over the sorted keys (tied pairs leave as
// records) or, for short lists and in the hooks build, as count / scan / compact
int round0(LmsSort &s)
{
    kiss_hip_ctx *ctx = s.ctx;
    const uint64_t count = ctx->m_far;
    RadixBufs rb;
    rb.first_pos = ctx->lms_pos; // the ascending list stays intact: the first pass reads it, nothing writes it
    rb.key[0] = ctx->keyA;
    rb.key[1] = ctx->keyB;
    rb.pos[0] = ctx->posA;
    // five passes: the result lands in buffer 1.  The sorted positions ARE the k-ordered list for every suffix that round 0
    // makes unique, so the last pass writes them where they belong and the compaction below has nothing to copy.
    static_assert(KISS_R0_PASSES % 2 == 1, "round-0 result must land in buffer 1");
    rb.pos[1] = ctx->lms_sorted_far;
    rb.seg[0] = rb.seg[1] = nullptr;
    // depth >= 125 whenever bounded, so the first 20 bases always count in full
    const int r0_shift = 64 - 2 * ROUND0_BASES;
    static_assert(64 - 2 * ROUND0_BASES == KISS_R0_SHIFT && (2 * ROUND0_BASES + 7) / 8 == KISS_R0_PASSES, "classify.hip counts these digits");
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, count, r0_shift, 0, &res));
    ctx->stats.lms_rounds++;
    ctx->stats.sort_item_rounds += count;
    s.Pc = rb.pos[res ^ 1]; // receives the survivors' positions
    uint64_t tot;
    // (the result of the five passes is in buffer 1 = the output list itself, so there are no positions to copy)
    const bool onepass = !ctx->opts.no_fc0_onepass && fc0_onepass_fits(ctx, count) && rb.pos[res] == ctx->lms_sorted_far;
    // the records go to keyA: the fifth pass must have left its result in keyB
    const bool pair_records = onepass && !ctx->opts.no_pair_records && rb.key[res] == ctx->keyB;
    if (onepass) {
        for (int attempt = 0;; attempt++) {
            const Fc0Job job{rb.key[res], rb.pos[res], count, r0_shift, ctx->lms_ctx_far, s.v.tctx,
                             pair_records ? s.v.rpos0 : (uint32_t *)nullptr, (uint32_t)s.v.rcol};
            KTRY(fc0_onepass(ctx, job, s.survivors(), s.v.d_total, &tot, &s.npairs));
            if ((tot >> 32) <= ctx->t_cap) break;
            if (attempt) return KINTERNAL();
            KTRY(regrow_tied(s, tot >> 32)); // (the survivors' stores beyond the arrays were dropped): once more
        }
        s.have_tctx = true;
    } else {
        FcJob job;
        job.key = rb.key[res];
        job.pos = rb.pos[res];
        job.count = count;
        job.cmp_shift = r0_shift;
        job.out = ctx->lms_sorted_far;
        job.octx = ctx->lms_ctx_far;
        KTRY(fc_count(ctx, job, s.v.d_total));
        KTRY(read_u64(ctx, s.v.d_total, &tot));
        if ((tot >> 32) > ctx->t_cap) {
            KTRY(regrow_tied(s, tot >> 32));
            KTRY(fc_count(ctx, job, s.v.d_total));
        }
        job.nctx = s.v.tctx;
        KTRY(fc_compact(ctx, job, s.survivors(), &s.have_tctx));
    }
    s.set_survivors(tot);
    if (s.dbg)
        fprintf(stderr, "[kiss_hip] round 0: items %llu -> survivors %llu in %llu segments\n", (unsigned long long)count,
                (unsigned long long)s.count, (unsigned long long)s.nseg);
    return KISS_HIP_OK;
}

// ---- the pairs that round 0 took out of the stream (after its retry: the list and the context words this patches are
// written by the pass itself)
int finish_pair_records(LmsSort &s)
{
    kiss_hip_ctx *ctx = s.ctx;
    if (s.npairs > ctx->m_far / 2) return KINTERNAL();
    {
        KTimer t(ctx, KISS_HIP_K_SEGRANK, 2 * s.npairs);
        hipLaunchKernelGGL(k_pair_finish, dim3((unsigned)div_up(s.npairs, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, s.n,
                           s.v.rpos0, s.v.rpos1, s.v.rslot, s.npairs, (uint64_t)ROUND0_BASES, s.depth, ctx->lms_sorted_far,
                           ctx->lms_ctx_far, ctx->hfar);
        KCHECK(hipGetLastError());
    }
    ctx->stats.pair_records = (uint32_t)s.npairs;
    // the pairs are the first refinement round's items like the survivors: the counts keep their meaning
    ctx->stats.sort_item_rounds += 2 * s.npairs;
    if (s.count == 0) ctx->stats.lms_rounds++; // (nothing but pairs was tied: no round runs)
    return KISS_HIP_OK;
}

// ---- the round's keys, for the segments that are ranked or sorted on them from memory
int gather_keys(LmsSort &s, const Round &r)
{
    kiss_hip_ctx *ctx = s.ctx;
    // k_small_finish gathers the keys of the small segments itself and keeps them in LDS; the big segments are radix sorted
    // on theirs (k_bigb_compact reads them from K1) unless a pivot round keys them against its reference string
    if (s.small_fused && r.pivot_ahead) return KISS_HIP_OK;
    const uint32_t *seg = s.Gc;
    uint32_t min_len = s.small_seg + 1u, max_len = 0xFFFFFFFFu;
    if (!s.small_fused) { // the three-kernel form ranks the small segments of >= 3 on keys from memory
        seg = s.no_pair_keys ? s.Gc : (const uint32_t *)nullptr;
        min_len = 3u;
        max_len = r.pivot_ahead ? s.small_seg : 0xFFFFFFFFu;
    }
    KTimer t(ctx, KISS_HIP_K_KEYGATHER, s.count);
    set_u32(ctx, s.SSc + s.nseg, (uint32_t)s.count); // (segstart's end entry is needed by the length test: set it first)
    hipLaunchKernelGGL(k_gather_keys, dim3(r.grid), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, s.n, s.Pc, s.count, s.off, r.mask,
                       s.v.K1, seg, s.SSc, min_len, max_len);
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}

// ---- segments of up to small_seg members retire; the members of the others are flagged in r.bigb
int finish_small_segments(LmsSort &s, const Round &r)
{
    kiss_hip_ctx *ctx = s.ctx;
    {
        KTimer t(ctx, KISS_HIP_K_SEGRANK, s.count);
        set_u32(ctx, s.SSc + s.nseg, (uint32_t)s.count, s.v.d_nbig);
        const uint32_t *tctx = (s.have_tctx && s.first_refine) ? s.v.tctx : (const uint32_t *)nullptr;
        if (s.small_fused) {
            hipLaunchKernelGGL(k_small_finish, dim3(r.grid), dim3(SF_THREADS), 0, ctx->stream, ctx->pk, s.n, s.Pc, s.Sc, s.Gc, s.SSc,
                               (uint32_t)s.count, s.off, s.depth, r.mask, ctx->lms_sorted_far, r.bigb, tctx, ctx->lms_ctx_far,
                               ctx->hfar);
        } else { // the three-kernel form (hooks build: KISS_HIP_NO_SMALL_FUSED, or another KISS_HIP_SMALL_SEG)
            hipLaunchKernelGGL(k_seg_adjacent, dim3(r.grid), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, s.n, s.v.K1, s.Pc, s.Gc,
                               s.SSc, s.count, s.off, s.depth, s.small_seg, r.inorder);
            hipLaunchKernelGGL(k_seg_finish, dim3(r.grid), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, s.n, s.v.K1, s.Pc, s.Sc, s.Gc,
                               s.SSc, s.count, s.off, s.depth, s.small_seg, r.inorder, ctx->lms_sorted_far, r.bigb, s.v.d_nbig,
                               tctx, ctx->lms_ctx_far, ctx->hfar);
        }
        KCHECK(hipGetLastError());
    }
    ctx->stats.lms_rounds++;
    ctx->stats.sort_item_rounds += s.count;
    return KISS_HIP_OK;
}

// ---- big segments -> the compact arrays bkeyA / bposA / bsegA / bslot, segment starts in bss
int compact_big_segments(LmsSort &s, const Round &r, uint64_t nbig, uint64_t nbigseg)
{
    kiss_hip_ctx *ctx = s.ctx;
    const BigbOut to{ctx->bkeyA, ctx->bposA, ctx->bsegA, s.v.bslot, s.v.bss};
    return bigb_compact(ctx, r.bigb, r.pivot_ahead ? (const uint64_t *)nullptr : s.v.K1, s.Pc, s.Sc, s.count, to, nbig, nbigseg);
}

#ifdef KISS_HIP_HOOKS
// debugging aid (KISS_HIP_DUMP_PIVOT): the inputs and keys of a pivot round, one file per round
int dump_pivot_round(LmsSort &s, const char *dump, uint64_t nbig, uint64_t nbigseg, int dbits, int slots)
{
    kiss_hip_ctx *ctx = s.ctx;
    std::vector<uint32_t> hp(nbig), hs(nbig), hss(nbigseg + 1);
    std::vector<uint64_t> hk(nbig);
    KCHECK(hipStreamSynchronize(ctx->stream));
    KCHECK(hipMemcpy(hp.data(), ctx->bposA, nbig * 4, hipMemcpyDeviceToHost));
    KCHECK(hipMemcpy(hs.data(), ctx->bsegA, nbig * 4, hipMemcpyDeviceToHost));
    KCHECK(hipMemcpy(hss.data(), s.v.bss, (nbigseg + 1) * 4, hipMemcpyDeviceToHost));
    KCHECK(hipMemcpy(hk.data(), ctx->bkeyB, nbig * 8, hipMemcpyDeviceToHost));
    char name[512];
    snprintf(name, sizeof name, "%s.%u", dump, ctx->stats.lms_rounds);
    if (FILE *f = fopen(name, "wb")) {
        const uint64_t hdr[6] = {nbig, nbigseg, s.off, s.depth, (uint64_t)dbits, (uint64_t)slots};
        fwrite(hdr, 8, 6, f);
        fwrite(hp.data(), 4, nbig, f);
        fwrite(hs.data(), 4, nbig, f);
        fwrite(hss.data(), 4, nbigseg + 1, f);
        fwrite(hk.data(), 8, nbig, f);
        fclose(f);
    }
    return KISS_HIP_OK;
}
#endif

// ---- a pivot round (bounded depth): see k_pivot_lcp.  Its survivors are tied through off + d + 1 > off bases: the next
// round starts from the same depth
int pivot_round(LmsSort &s, uint64_t nbig, uint64_t nbigseg)
{
    kiss_hip_ctx *ctx = s.ctx;
    static const int pivot_den[3] = {4, 7, 11};
    const unsigned bgrid = (unsigned)div_up(nbig, LS_THREADS);
    const int dbits = bits_for(s.depth - s.off); // d < depth - off
    int slots = 63 / (dbits + 4);                // deviations per key: [side 2 | d | base 2] each + 1 bit
    if (slots > s.pivot_slots) slots = s.pivot_slots;
    const int kbits = slots * (dbits + 4) + 1;
    const int key_lo = 64 - 8 * ((kbits + 7) / 8);
    // room for the members' context words below the sorted bits (k = 256: 40 key bits, 24 bits free)
    const bool with_ctx = key_lo >= 24 && !ctx->opts.no_pivot_ctx;
    {
        KTimer t(ctx, KISS_HIP_K_SEGRANK, nbig);
        hipLaunchKernelGGL(k_pivot_lcp, dim3(bgrid), dim3(LS_THREADS), 0, ctx->stream, ctx->pk, ctx->bposA, ctx->bsegA, s.v.bss, nbig,
                           s.off, s.depth, dbits, slots, ctx->bkeyB, pivot_den[s.pivot_rounds_done % 3], with_ctx ? 1 : 0);
        s.pivot_rounds_done++;
        KCHECK(hipGetLastError());
    }
#ifdef KISS_HIP_HOOKS
    if (ctx->opts.dump_pivot[0]) KTRY(dump_pivot_round(s, ctx->opts.dump_pivot, nbig, nbigseg, dbits, slots));
#endif
    RadixBufs pb;
    pb.key[0] = ctx->bkeyB;
    pb.key[1] = s.v.key2;
    pb.pos[0] = ctx->bposA;
    pb.pos[1] = ctx->bposB;
    pb.seg[0] = ctx->bsegA;
    pb.seg[1] = ctx->bsegB;
    int pres = 0;
    const int sbits = bits_for(nbigseg);
    KTRY(kiss_radix_sort(ctx, pb, nbig, key_lo, sbits, &pres));
    // a single segment has no segment digits: the sort then leaves the segment column alone (all the same id)
    const uint32_t *sseg = sbits ? pb.seg[pres] : ctx->bsegA;
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, nbig);
        hipLaunchKernelGGL(k_pivot_heads, dim3(bgrid), dim3(LS_THREADS), 0, ctx->stream, pb.key[pres], sseg, nbig, 64 - kbits,
                           s.v.pivot_heads, ~0ull << (64 - kbits));
        KCHECK(hipGetLastError());
    }
    FcJob job;
    job.src = FC_HEADS;
    job.key = reinterpret_cast<const uint64_t *>(s.v.pivot_heads);
    job.pos = pb.pos[pres];
    job.slot = s.v.bslot;
    job.count = nbig;
    job.out = ctx->lms_sorted_far;
    job.tmark = ctx->lms_ctx_far;
    job.payload = with_ctx ? pb.key[pres] : (const uint64_t *)nullptr;
    uint64_t tot;
    KTRY(fc_count(ctx, job, s.v.d_total));
    KTRY(read_u64(ctx, s.v.d_total, &tot));
    KTRY(fc_compact(ctx, job, s.survivors()));
    ctx->stats.big_item_rounds += nbig;
    s.set_survivors(tot);
    if (s.dbg)
        fprintf(stderr, "[kiss_hip]   pivot round: %llu big-segment items in %llu segments -> %llu still tied in %llu "
                        "segments (same depth)\n", (unsigned long long)nbig, (unsigned long long)nbigseg,
                (unsigned long long)s.count, (unsigned long long)s.nseg);
    return KISS_HIP_OK;
}

// the big-segment items of a 32-base round in (segment, key) order
struct SortedBig {
    const uint64_t *key;
    const uint32_t *pos, *seg;
};

// NE of a round, or null: no room for it (it would overlap the scan words: the tied-segment arrays are nearly full), or the
// first refinement round, which still holds the diverged copies of interspersed repeats (78 % of the items differ from
// their pivot at chm13 size): the split only pays from the second round on, when what is left is the long tandem arrays
uint64_t *class_split_flags(const LmsSort &s, uint64_t nbig)
{
    if (2 * nbig > s.ctx->t_cap || s.off == ROUND0_BASES) return nullptr;
    return s.ctx->flags + 2 * s.ctx->t_cap - nbig;
}

// ---- a 32-base round with class split: three-way split of every big segment around the key of its middle item, then the
// < and > groups alone are radix sorted on (group, key)
int class_split_round(LmsSort &s, const Round &r, uint64_t *NE, uint64_t nbig, uint64_t nbigseg, SortedBig *sorted)
{
    kiss_hip_ctx *ctx = s.ctx;
    const unsigned bgrid = (unsigned)div_up(nbig, LS_THREADS);
    uint64_t *const F1 = s.v.F1, *const F2 = s.v.F2;
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, nbig);
        hipLaunchKernelGGL(k_pivot_class, dim3(bgrid), dim3(LS_THREADS), 0, ctx->stream, ctx->bkeyA, ctx->bsegA, s.v.bss, nbig, F1);
        KCHECK(hipGetLastError());
    }
    KTRY(flags_total(ctx, F1, F2, nbig, s.v.d_ptot)); // (segment ends at nbig; read by the scatter, not by the host)
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, nbig);
        hipLaunchKernelGGL(k_pivot_scatter, dim3(bgrid), dim3(LS_THREADS), 0, ctx->stream, ctx->bkeyA, ctx->bposA, ctx->bsegA, s.v.bss,
                           nbig, F1, F2, s.v.d_ptot, ctx->bkeyB, ctx->bposB, NE);
        KCHECK(hipGetLastError());
    }
    uint64_t *const H1 = NE, *const H2 = F1; // the class words are dead now
    uint64_t nt;
    KTRY(flags_total(ctx, H1, H2, nbig, s.v.d_total, &nt));
    const uint64_t nne = nt >> 32, ngroups = nt & 0xFFFFFFFFull;
    if (s.dbg)
        fprintf(stderr, "[kiss_hip]   big segments %llu: %llu of %llu items differ from their pivot key (%llu groups)\n",
                (unsigned long long)nbigseg, (unsigned long long)nne, (unsigned long long)nbig, (unsigned long long)ngroups);
    if (nne) {
        BigSort b;
        b.key = ctx->bkeyB;
        b.pos = ctx->bposB;
        b.count = nbig;
        b.flags = H1;
        b.ex = H2;
        b.nbig = nne;
        b.ngroups = ngroups;
        b.key_lo_bit = r.key_lo_bit;
        b.kbuf[0] = s.v.key2;
        b.kbuf[1] = ctx->bkeyA; // free since the partition
        b.pbuf[0] = s.v.sortpos[0];
        b.pbuf[1] = s.v.sortpos[1];
        b.sbuf[0] = ctx->bsegB;
        b.sbuf[1] = s.v.seg2;
        b.bidx = ctx->bposA;    // (as bkeyA)
        b.okey = ctx->bkeyB;
        b.opos = ctx->bposB;
        KTRY(sort_big_members(ctx, b));
    }
    ctx->stats.big_item_rounds += nne;
    *sorted = SortedBig{ctx->bkeyB, ctx->bposB, ctx->bsegA};
    return KISS_HIP_OK;
}

// ---- a 32-base round by plain radix sort on (segment, key): the first refinement round, or no room for the split's flags
int radix_round(LmsSort &s, const Round &r, uint64_t nbig, uint64_t nbigseg, SortedBig *sorted)
{
    kiss_hip_ctx *ctx = s.ctx;
    RadixBufs bb;
    bb.key[0] = ctx->bkeyA;
    bb.key[1] = ctx->bkeyB;
    bb.pos[0] = ctx->bposA;
    bb.pos[1] = ctx->bposB;
    bb.seg[0] = ctx->bsegA;
    bb.seg[1] = ctx->bsegB;
    int bres = 0;
    KTRY(kiss_radix_sort(ctx, bb, nbig, r.key_lo_bit, bits_for(nbigseg), &bres));
    ctx->stats.big_item_rounds += nbig;
    // one segment: no segment digits, the column did not move
    *sorted = SortedBig{bb.key[bres], bb.pos[bres], bits_for(nbigseg) ? bb.seg[bres] : ctx->bsegA};
    return KISS_HIP_OK;
}

// ---- the closing compaction of a 32-base round: split where neighbours differ, singletons retire, the rest go round again
int closing_compaction(LmsSort &s, const Round &r, const SortedBig &sorted, uint64_t nbig)
{
    kiss_hip_ctx *ctx = s.ctx;
    FcJob job;
    job.src = FC_KEY_SEG;
    job.key = sorted.key;
    job.seg = sorted.seg;
    job.pos = sorted.pos;
    job.slot = s.v.bslot;
    job.count = nbig;
    job.last_round = (int)r.last_round;
    job.out = ctx->lms_sorted_far;
    job.tmark = ctx->lms_ctx_far;
    uint64_t tot;
    KTRY(fc_count(ctx, job, s.v.d_total));
    KTRY(fc_compact(ctx, job, s.survivors())); // (queued before the host waits for the total)
    KTRY(read_u64(ctx, s.v.d_total, &tot));
    s.set_survivors(tot);
    return KISS_HIP_OK;
}

// KISS_HIP_DEBUG: device time from its construction to ms()
struct DbgSpan {
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DbgSpan(kiss_hip_ctx *ctx, bool on) : stream(ctx->stream)
    {
        if (!on) return;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, stream);
    }
    float ms()
    {
        float v = 0;
        (void)hipEventRecord(e1, stream);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&v, e0, e1);
        return v;
    }
    ~DbgSpan()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

} // namespace

int kiss_lms_sort(kiss_hip_ctx *ctx, uint64_t n, uint32_t k, uint64_t depth)
{
    (void)k;
    const uint64_t m_far = ctx->m_far;
    ctx->stats.lms_rounds = 0;
    ctx->stats.sort_item_rounds = 0;
    ctx->stats.pair_records = 0;
    if (m_far == 0) return KISS_HIP_OK;
    if (m_far == 1) {
        KCHECK(hipMemcpyAsync(ctx->lms_sorted_far, ctx->lms_pos, sizeof(uint32_t), hipMemcpyDeviceToDevice,
                              ctx->stream));
        KTRY(kiss_zero_u32(ctx, ctx->lms_ctx_far, 1));
        return KISS_HIP_OK;
    }
    LmsSort s;
    s.ctx = ctx;
    s.n = n;
    s.depth = depth;
    s.dbg = ctx->opts.debug;
    s.pivot_on = !ctx->opts.no_pivot_rounds;
    s.pivot_r1 = !ctx->opts.pivot_from_round2;
    s.pivot_slots = ctx->opts.pivot_slots >= 1 && ctx->opts.pivot_slots <= 8 ? ctx->opts.pivot_slots : 3;
    s.no_pair_keys = !ctx->opts.pair_keys;
    s.small_seg = ctx->opts.small_seg >= 2 && ctx->opts.small_seg <= 4096 ? ctx->opts.small_seg : LMS_SMALL_SEG;
    s.small_fused = !ctx->opts.no_small_fused && s.small_seg == LMS_SMALL_SEG;
    s.take_tied_arrays();

    KTRY(round0(s));
    if (s.npairs) KTRY(finish_pair_records(s));

    // refinement rounds: what is tied through `off` bases goes round until nothing is
    for (;; s.first_refine = false) {
        if (s.count == 0) break;
        if (depth && s.off >= depth) return KINTERNAL(); // the last round retires everything
        const Round r = round_of(s);
        KTRY(gather_keys(s, r));
        uint64_t bt;
        {
            DbgSpan span(ctx, s.dbg);
            KTRY(finish_small_segments(s, r));
            KTRY(bigb_count(ctx, r.bigb, s.count, s.v.d_total, &bt));
            if (s.dbg) fprintf(stderr, "[kiss_hip]   seg_finish + flag scan %.3f ms\n", span.ms());
        }
        const uint64_t nbig = bt >> 32, nbigseg = bt & 0xFFFFFFFFull;
        if (s.dbg)
            fprintf(stderr, "[kiss_hip] round off=%llu: items %llu in %llu segments, big-segment items %llu\n",
                    (unsigned long long)s.off, (unsigned long long)s.count, (unsigned long long)s.nseg, (unsigned long long)nbig);
        if (nbig == 0) break;
        KTRY(compact_big_segments(s, r, nbig, nbigseg));
        if (r.pivot_ahead) {
            KTRY(pivot_round(s, nbig, nbigseg));
            continue;
        }
        SortedBig sorted;
        if (uint64_t *NE = class_split_flags(s, nbig)) KTRY(class_split_round(s, r, NE, nbig, nbigseg, &sorted));
        else KTRY(radix_round(s, r, nbig, nbigseg, &sorted));
        KTRY(closing_compaction(s, r, sorted, nbig));
        s.off += 32;
        if (!depth && s.off > n + 64 && s.count > 0) return KINTERNAL(); // exact mode must have terminated
        // exact order, repeats longer than this: 32 bases per round is the wrong tool, the caller switches to
        // rank doubling (same result)
        if (!depth && s.off >= KISS_EXACT_MSD_MAX_DEPTH && s.count > 0) return KISS_INTERNAL_TOO_DEEP;
    }
    return KISS_HIP_OK;
}
