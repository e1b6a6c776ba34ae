// flag_compact.hip -- flag + compaction of sorted lists (flag_compact.hpp): the step that ends round 0 and every refinement
// round of the LMS sort (lms_sort.hip) and every round of the rank doubling (doubling.hip).  The kernel families differ in
// where the flags come from and how wide the accesses are:
//   k_fc_*      keys (and segment ids) or head bytes, one item per lane and load: any combination of outputs
//   k_fc0_*     round 0, keys only, slot = index: 16-byte accesses; k_fc0_onepass does count + scan + compact in one pass
//   k_fch_*     head bytes over a whole suffix array or LMS list, survivors only
//   k_bigb_*    the byte flags a refinement round leaves for the members of big segments
// All of them count per tile of FC_TILE items, scan over the tiles and compact with the tile's offset.
#include "flag_compact.hpp"
#include <cstdio>
#include <cstring>

using namespace kiss_fc;

namespace {

// ---- fused flag + compaction over 2048-item tiles (no per-item flag / scan arrays) ------------------------
// pass 1: per-tile (survivors << 32 | surviving heads); pass 2 (after an exclusive scan over tiles): the same
// flags again, wave-ballot prefix inside the tile, survivors compacted, singletons retired.
constexpr int FC_THREADS = 256;
constexpr int FC_ITEMS = 8;
constexpr int FC_ITEMS_DEFAULT = FC_ITEMS;
constexpr int FC_TILE = FC_THREADS * FC_ITEMS;

template <int SRC>
__device__ __forceinline__ void fc_flags(const uint64_t *__restrict__ key, const uint32_t *__restrict__ seg, uint64_t i,
                                         uint64_t count, int cmp_shift, int last_round, bool &surv, bool &shead,
                                         bool *tie = nullptr, // *tie: the item shares everything compared with a neighbour
                                         bool *tie_prev = nullptr) // ... with its predecessor
{
    surv = shead = false;
    if (tie) *tie = false;
    if (tie_prev) *tie_prev = false;
    if (i >= count) return;
    bool head, nhead;
    if constexpr (SRC == FC_HEADS) {
        const uint8_t *hb = reinterpret_cast<const uint8_t *>(key);
        head = (i == 0) || hb[i] != 0;
        nhead = (i + 1 == count) || hb[i + 1] != 0;
        if (tie) *tie = (hb[i] & 2) != 0; // the producer of the head bytes says so (k_pivot_heads)
        if (tie_prev) *tie_prev = (hb[i] & 4) != 0;
    } else {
        constexpr bool HAS_SEG = SRC == FC_KEY_SEG;
        uint64_t k = key[i] >> cmp_shift;
        uint32_t s = HAS_SEG ? seg[i] : 0u;
        head = (i == 0) || (key[i - 1] >> cmp_shift) != k || (HAS_SEG && seg[i - 1] != s);
        nhead = (i + 1 == count) || (key[i + 1] >> cmp_shift) != k || (HAS_SEG && seg[i + 1] != s);
    }
    surv = !(head && nhead) && !last_round;
    shead = surv && head;
    if constexpr (SRC != FC_HEADS) {
        if (tie) *tie = !(head && nhead);
        if (tie_prev) *tie_prev = !head;
    }
}

template <int SRC>
__global__ __launch_bounds__(FC_THREADS) void k_fc_count(const uint64_t *__restrict__ key,
                                                        const uint32_t *__restrict__ seg, uint64_t count,
                                                        int cmp_shift, int last_round, uint64_t *__restrict__ tcnt)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * FC_TILE + (uint64_t)wave * (FC_ITEMS * 64) + lane_id();
    uint32_t ns = 0, nh = 0;
#pragma unroll
    for (int j = 0; j < FC_ITEMS; j++) {
        bool sv, sh;
        fc_flags<SRC>(key, seg, base + (uint64_t)j * 64, count, cmp_shift, last_round, sv, sh);
        ns += (uint32_t)__popcll(__ballot(sv));
        nh += (uint32_t)__popcll(__ballot(sh));
    }
    if (lane_id() == 0) {
        ws[wave][0] = ns;
        ws[wave][1] = nh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int w = 0; w < FC_THREADS / 64; w++) {
            a += ws[w][0];
            b += ws[w][1];
        }
        tcnt[blockIdx.x] = (a << 32) | b;
    }
}

// out: retired items land in out[slot] (nullptr: they already are where they belong);
// isa (optional): inverse array, isa[position] = slot for every retired item;
// octx (optional, round 0 only): context word per slot from the key payload, 0 for slots still tied
template <int SRC, bool HAS_SLOT>
__global__ __launch_bounds__(FC_THREADS) void k_fc_compact(const uint64_t *__restrict__ key,
                                                          const uint32_t *__restrict__ seg,
                                                          const uint32_t *__restrict__ pos,
                                                          const uint32_t *__restrict__ slot, uint64_t count,
                                                          int cmp_shift, int last_round,
                                                          const uint64_t *__restrict__ tex, // exclusive scan of tcnt
                                                          uint32_t *__restrict__ npos, uint32_t *__restrict__ nslot,
                                                          uint32_t *__restrict__ nseg, uint32_t *__restrict__ nsegstart,
                                                          uint32_t *__restrict__ out, uint32_t *__restrict__ isa,
                                                          uint32_t *__restrict__ octx,
                                                          uint32_t *__restrict__ tmark, // taint marks of retiring items
                                                          const uint64_t *__restrict__ payload, // optional, with tmark: words
                                                          // whose low KISS_KEY_CTX bits are the items' context words
                                                          int isa_shift, // isa is indexed by position >> isa_shift
                                                          const uint64_t *__restrict__ pk_fix, // optional, with cfix: the
                                                          uint32_t *__restrict__ cfix, // context word of a retiring item's own
                                                          // position is gathered from the packed text into cfix[slot]
                                                          uint8_t *__restrict__ hmark) // optional: hmark[slot] = 0 for an item
                                                          // that retires tied with its predecessor (ctx->hfar)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * FC_TILE + (uint64_t)wave * (FC_ITEMS * 64) + lane_id();
    uint32_t rs[FC_ITEMS], rh[FC_ITEMS]; // rank among survivors / surviving heads inside the wave (inclusive for heads)
    uint32_t fl = 0;                      // bit 2j = survivor, bit 2j+1 = surviving head
    uint32_t tl = 0;                      // bit j = retires while tied with a neighbour (last round / complete pivot key)
    uint32_t tp = 0;                      // bit j = ... and that neighbour is its predecessor
    uint32_t ns = 0, nh = 0;
#pragma unroll
    for (int j = 0; j < FC_ITEMS; j++) {
        bool sv, sh, ti, tpv;
        fc_flags<SRC>(key, seg, base + (uint64_t)j * 64, count, cmp_shift, last_round, sv, sh, &ti, &tpv);
        tl |= (ti && !sv ? 1u : 0u) << j;
        tp |= (ti && tpv && !sv ? 1u : 0u) << j;
        const uint64_t ms = __ballot(sv), mh = __ballot(sh);
        rs[j] = ns + (uint32_t)__popcll(ms & lanemask_lt());
        rh[j] = nh + (uint32_t)__popcll(mh & lanemask_lt()) + (sh ? 1u : 0u);
        ns += (uint32_t)__popcll(ms);
        nh += (uint32_t)__popcll(mh);
        fl |= (sv ? 1u : 0u) << (2 * j) | (sh ? 2u : 0u) << (2 * j);
    }
    if (lane_id() == 0) {
        ws[wave][0] = ns;
        ws[wave][1] = nh;
    }
    __syncthreads();
    const uint64_t te = tex[blockIdx.x];
    uint32_t bs = (uint32_t)(te >> 32), bh = (uint32_t)(te & 0xFFFFFFFFull);
    for (int w = 0; w < wave; w++) {
        bs += ws[w][0];
        bh += ws[w][1];
    }
#pragma unroll
    for (int j = 0; j < FC_ITEMS; j++) {
        const uint64_t i = base + (uint64_t)j * 64;
        if (i >= count) continue;
        const uint32_t p = pos[i];
        const uint32_t sl = HAS_SLOT ? slot[i] : (uint32_t)i;
        if ((fl >> (2 * j)) & 1u) {
            const uint32_t ni = bs + rs[j];
            const uint32_t sid = bh + rh[j] - 1u; // heads up to and including this item's own segment head
            npos[ni] = p;
            nslot[ni] = sl;
            nseg[ni] = sid;
            if ((fl >> (2 * j)) & 2u) nsegstart[sid] = ni;
            if (octx) octx[sl] = 0; // tied so far: its context word is gathered at placement
        } else {
            if (out) out[sl] = p;
            if (tmark && payload) // the word came along with the sort key (k_pivot_lcp)
                tmark[sl] = (uint32_t)(payload[i] & KISS_KEY_CTX_MASK) | (((tl >> j) & 1u) ? KISS_CTX_TAINT : 0u);
            else if (tmark && ((tl >> j) & 1u)) tmark[sl] = KISS_CTX_TAINT; // no context word yet: gathered at placement
            if (isa) isa[p >> isa_shift] = sl;
            if (cfix) cfix[sl] = kiss_load_ctx(pk_fix, p);
            if (hmark && ((tp >> j) & 1u)) hmark[sl] = 0;
            if constexpr (SRC != FC_HEADS) {
                if (octx) octx[sl] = (uint32_t)(key[i] & KISS_KEY_CTX_MASK); // round 0: payload of the classification key
            }
        }
    }
}

// ---- round 0 (keys only, slot = index): the same flag + compaction with 16-byte accesses ----------------------
// A thread owns FC_ITEMS consecutive items (two keys per load, four positions per load); survivor ranks come from a
// wave prefix of the per-thread counts.  Every slot gets its position (a tied suffix's slot is rewritten when it
// retires later) and its context word (0 while tied), so the stores are plain 16-byte streams.
template <int FC_ITEMS = FC_ITEMS_DEFAULT>
__device__ __forceinline__ void fc0_load(const uint64_t *__restrict__ key, uint64_t i0, uint64_t count, int cmp_shift,
                                         uint64_t k[FC_ITEMS + 2], uint32_t &valid, uint32_t *low = nullptr)
{
    // k[0] = key before my first item, k[1..FC_ITEMS] = my items, k[FC_ITEMS + 1] = key after; all >> cmp_shift
    valid = i0 >= count ? 0u : (count - i0 >= FC_ITEMS ? (uint32_t)FC_ITEMS : (uint32_t)(count - i0));
    if (valid == FC_ITEMS) {
#pragma unroll
        for (int q = 0; q < FC_ITEMS / 2; q++) {
            const ulonglong2 kk = *reinterpret_cast<const ulonglong2 *>(key + i0 + 2 * q);
            k[1 + 2 * q] = kk.x >> cmp_shift;
            k[2 + 2 * q] = kk.y >> cmp_shift;
            if (low) { // the payload bits below the compared ones
                low[2 * q] = (uint32_t)(kk.x & KISS_KEY_CTX_MASK);
                low[2 * q + 1] = (uint32_t)(kk.y & KISS_KEY_CTX_MASK);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < FC_ITEMS; e++) {
            const uint64_t kk = (uint32_t)e < valid ? key[i0 + e] : 0ull;
            k[1 + e] = kk >> cmp_shift;
            if (low) low[e] = (uint32_t)(kk & KISS_KEY_CTX_MASK);
        }
    }
    k[0] = (valid && i0 > 0) ? (key[i0 - 1] >> cmp_shift) : 0ull;
    k[FC_ITEMS + 1] = (valid && i0 + FC_ITEMS < count) ? (key[i0 + FC_ITEMS] >> cmp_shift) : 0ull;
}

template <int FC_ITEMS = FC_ITEMS_DEFAULT>
__device__ __forceinline__ void fc0_flags(const uint64_t k[FC_ITEMS + 2], uint64_t i0, uint64_t count, uint32_t valid,
                                          uint32_t &survmask, uint32_t &headmask)
{
    survmask = headmask = 0;
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        if ((uint32_t)e < valid) {
            const uint64_t i = i0 + (uint64_t)e;
            const bool head = i == 0 || k[e] != k[e + 1];
            const bool nhead = i + 1 == count || k[e + 2] != k[e + 1];
            const bool surv = !(head && nhead);
            survmask |= (surv ? 1u : 0u) << e;
            headmask |= ((surv && head) ? 1u : 0u) << e;
        }
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_fc0_count(const uint64_t *__restrict__ key, uint64_t count, int cmp_shift,
                                                         uint64_t *__restrict__ tcnt)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint64_t k[FC_ITEMS + 2];
    uint32_t valid, sm, hm;
    fc0_load(key, i0, count, cmp_shift, k, valid);
    fc0_flags(k, i0, count, valid, sm, hm);
    uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ns += __shfl_xor(ns, d, 64);
        nh += __shfl_xor(nh, d, 64);
    }
    if (lane_id() == 0) {
        ws[threadIdx.x >> 6][0] = ns;
        ws[threadIdx.x >> 6][1] = nh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int w = 0; w < FC_THREADS / 64; w++) {
            a += ws[w][0];
            b += ws[w][1];
        }
        tcnt[blockIdx.x] = (a << 32) | b;
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_fc0_compact(const uint64_t *__restrict__ key,
                                                           const uint32_t *__restrict__ pos, uint64_t count,
                                                           int cmp_shift, const uint64_t *__restrict__ tex,
                                                           uint32_t *__restrict__ npos, uint32_t *__restrict__ nslot,
                                                           uint32_t *__restrict__ nseg, uint32_t *__restrict__ nsegstart,
                                                           uint32_t *__restrict__ out, uint32_t *__restrict__ octx,
                                                           uint32_t *__restrict__ nctx)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint64_t k[FC_ITEMS + 2];
    uint32_t valid, sm, hm;
    uint32_t p[FC_ITEMS], cw[FC_ITEMS];
    fc0_load(key, i0, count, cmp_shift, k, valid, cw);
    fc0_flags(k, i0, count, valid, sm, hm);
    const uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
    uint32_t is = ns, ih = nh; // inclusive wave prefixes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t os = __shfl_up(is, d, 64), oh = __shfl_up(ih, d, 64);
        if ((int)lane_id() >= d) {
            is += os;
            ih += oh;
        }
    }
    if (lane_id() == 63) {
        ws[wave][0] = is;
        ws[wave][1] = ih;
    }
    __syncthreads();
    const uint64_t te = tex[blockIdx.x];
    uint32_t bs = (uint32_t)(te >> 32) + (is - ns), bh = (uint32_t)(te & 0xFFFFFFFFull) + (ih - nh);
    for (int w = 0; w < wave; w++) {
        bs += ws[w][0];
        bh += ws[w][1];
    }
    if (valid == 0) return;
    // cw = payload of my keys: the low KISS_KEY_CTX bits (cmp_shift >= 24 in round 0), kept from the one key load
    if (valid == FC_ITEMS) {
#pragma unroll
        for (int q = 0; q < FC_ITEMS / 4; q++) {
            const uint4 t = *reinterpret_cast<const uint4 *>(pos + i0 + 4 * q);
            p[4 * q] = t.x;
            p[4 * q + 1] = t.y;
            p[4 * q + 2] = t.z;
            p[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < FC_ITEMS; e++) p[e] = (uint32_t)e < valid ? pos[i0 + e] : 0u;
    }
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        if ((sm >> e) & 1u) {
            const uint32_t ni = bs++;
            if ((hm >> e) & 1u) bh++;
            const uint32_t sid = bh - 1u; // heads up to and including this item's own segment head
            npos[ni] = p[e];
            nslot[ni] = (uint32_t)(i0 + e);
            nseg[ni] = sid;
            if ((hm >> e) & 1u) nsegstart[sid] = ni;
            if (nctx) nctx[ni] = cw[e]; // travels with the tied item through the first refinement round (k_seg_finish)
            cw[e] = 0;                  // tied so far: written when the item is finished, else gathered at placement
        }
    }
    // out == nullptr: the positions already are where they belong (the last radix pass wrote them into the output list)
    if (valid == FC_ITEMS) {
#pragma unroll
        for (int q = 0; q < FC_ITEMS / 4; q++) {
            if (out) *reinterpret_cast<uint4 *>(out + i0 + 4 * q) = make_uint4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
            *reinterpret_cast<uint4 *>(octx + i0 + 4 * q) = make_uint4(cw[4 * q], cw[4 * q + 1], cw[4 * q + 2], cw[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < FC_ITEMS; e++)
            if ((uint32_t)e < valid) {
                if (out) out[i0 + e] = p[e];
                octx[i0 + e] = cw[e];
            }
    }
}

// ---- round 0 in ONE pass over the sorted keys ---------------------------------------------------------------------
// k_fc0_count + scan + k_fc0_compact read the 7 GB of sorted keys twice.  Here a tile of FC1_TILE items flags its items,
// publishes its (survivors, segment heads) pair, finds the sum over all earlier tiles by a decoupled look-back and
// compacts -- the keys are read once.  One 64-bit descriptor per tile: [status:2 | survivors:31 | heads:31] (status 1 =
// this tile's counts, 2 = counts of this and all earlier tiles); wave 0 inspects 64 predecessors per round trip.  Tiles
// are numbered by an atomic ticket, so every predecessor of a running tile is running or done, and the wait is bounded
// like the radix look-back (radix.hip) -- an error flag instead of a hung GPU.  The host learns the totals only
// afterwards, so stores beyond `cap` (the tied-segment arrays) are dropped; the caller regrows and runs the pass again.
// Layout (round 4): STRIPED.  A lane takes two neighbouring items per 16-byte key load and the 64 lanes of a wave take
// 128 neighbouring items per load instruction (1 KiB, every byte of every line used); a wave owns FC1_ITEMS / 2 such
// chunks.  The blocked form of round 3 (a thread owned 8 neighbouring items = 64 bytes, so ONE load instruction of a wave
// touched 64 different lines and used 16 bytes of each; the 16 waves' 64 KiB of lines did not fit the 32 KiB L1) spent
// its time re-fetching lines from L2: 7.4 ms for 17 GB, and 10.4 / 15.3 ms with 16 / 32 items per thread.  Flags come
// from one lane shift of the keys per chunk, ranks from ballots; a wave's stores of one chunk go to consecutive
// survivor slots.  The survivor order (rank = tied items in front, in list order) is the same as before.
#ifndef KISS_FC1_THREADS
#define KISS_FC1_THREADS 1024
#endif
#ifndef KISS_FC1_ITEMS
#define KISS_FC1_ITEMS 8
#endif
#ifndef KISS_FC1_MIN_WAVES
#define KISS_FC1_MIN_WAVES 1
#endif
#ifndef KISS_FC1_STORE_UNROLL
#define KISS_FC1_STORE_UNROLL 4 // (= all chunks; 1 saves 12 registers and buys no second workgroup per CU)
#endif
constexpr int FC1_THREADS = KISS_FC1_THREADS;
constexpr int FC1_ITEMS = KISS_FC1_ITEMS;
constexpr int FC1_CHUNKS = FC1_ITEMS / 2;         // chunks of 128 items per wave
constexpr int FC1_WAVE_ITEMS = 64 * FC1_ITEMS;    // 512
constexpr int FC1_TILE = FC1_THREADS * FC1_ITEMS; // 8192
constexpr uint32_t FC1_SPIN_LIMIT = 1u << 22;
static_assert(FC1_ITEMS % 2 == 0 && FC1_ITEMS <= 16, "two items per lane and chunk; four flag bits per chunk in one word");

#ifdef FC_PROF
// -DFC_PROF (tools/build_prof.sh): wall-clock ticks between the phase boundaries of a tile, summed over all tiles by thread 0
__device__ unsigned long long fc_prof[12];
#define FC_MARK(i)                                                                                                     \
    do {                                                                                                               \
        if (threadIdx.x == 0) {                                                                                        \
            const unsigned long long now_ = wall_clock64();                                                            \
            atomicAdd(&fc_prof[i], now_ - t_prev_);                                                                    \
            t_prev_ = now_;                                                                                            \
        }                                                                                                              \
    } while (0)
#else
#define FC_MARK(i)
#endif
__device__ __forceinline__ uint64_t lane_value_u64(uint64_t v, int src_lane) // (the same lane in all callers)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src_lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src_lane);
    return ((uint64_t)hi << 32) | lo;
}

// PAIRS: a tied segment of exactly two items (head at i, none at i + 1, head at i + 2 or the end of the list) does not
// survive.  The lane that holds its first member writes ONE record -- (position of the first member, position of the
// second, list index of the first = its slot; the second's slot is the next one), three columns of rcol words in rec --
// at index (pairs in front of it), and k_pair_finish decides the pair with one lane and no index chasing.  Both members
// keep their context words in octx instead of the zero of a tied item, so a record needs none.
// A third running count goes through the look-back in a second descriptor word per tile, [status:2 | pairs:62], next to
// the first (desc[2 t], desc[2 t + 1]); the two are written one after the other, so a reader that finds them in different
// states reads them again.  The second member is the lane's own second item, the first item of the lane above or (lane 63)
// the first item of the next chunk; a pair whose first member is the LAST item of a wave's 512-item stretch would need
// the key two items past the stretch: it stays in the survivor stream, where k_seg_finish decides it as before.
template <bool PAIRS>
__global__ __launch_bounds__(FC1_THREADS, KISS_FC1_MIN_WAVES) void k_fc0_onepass(const uint64_t *__restrict__ key,
                                                            const uint32_t *__restrict__ pos, uint64_t count,
                                                            int cmp_shift, uint64_t tiles, uint64_t *__restrict__ desc,
                                                            uint32_t *__restrict__ ticket, uint32_t *__restrict__ err,
                                                            uint32_t *__restrict__ npos, uint32_t *__restrict__ nslot,
                                                            uint32_t *__restrict__ nseg, uint32_t *__restrict__ nsegstart,
                                                            uint32_t *__restrict__ octx, uint32_t *__restrict__ nctx,
                                                            uint64_t cap, uint64_t *__restrict__ total,
                                                            uint32_t *__restrict__ rec, uint32_t rcol)
{
    constexpr int DS = PAIRS ? 2 : 1; // descriptor words per tile
    __shared__ uint32_t ws[FC1_THREADS / 64][3];
    __shared__ uint32_t s_tile;
    __shared__ uint32_t s_excl[3];
#ifdef FC_PROF
    unsigned long long t_prev_ = wall_clock64();
#endif
    if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    FC_MARK(0); // ticket + barrier
    const uint64_t tile = s_tile;
    if (tile >= tiles) return;
    const int wave = threadIdx.x >> 6;
    const uint32_t lane = lane_id();
    const uint64_t wbase = tile * FC1_TILE + (uint64_t)wave * FC1_WAVE_ITEMS; // first item of my wave
    const bool full = wbase + FC1_WAVE_ITEMS <= count;                        // (wave-uniform)
    uint64_t k0[FC1_CHUNKS], k1[FC1_CHUNKS]; // compared bits of my two items of chunk j
    uint32_t c0[FC1_CHUNKS], c1[FC1_CHUNKS]; // their payload: the low KISS_KEY_CTX bits (cmp_shift >= 24 in round 0)
#pragma unroll
    for (int j = 0; j < FC1_CHUNKS; j++) {
        const uint64_t a = wbase + (uint64_t)j * 128 + 2 * lane;
        ulonglong2 kk;
        if (full) kk = *reinterpret_cast<const ulonglong2 *>(key + a);
        else {
            kk.x = a < count ? key[a] : 0ull;
            kk.y = a + 1 < count ? key[a + 1] : 0ull;
        }
        k0[j] = kk.x >> cmp_shift;
        k1[j] = kk.y >> cmp_shift;
        c0[j] = (uint32_t)(kk.x & KISS_KEY_CTX_MASK);
        c1[j] = (uint32_t)(kk.y & KISS_KEY_CTX_MASK);
    }
    // the items either side of my wave's stretch
    const bool has_prev = wbase > 0 && wbase < count, has_next = wbase + FC1_WAVE_ITEMS < count;
    const uint64_t kprev = has_prev ? key[wbase - 1] >> cmp_shift : 0ull;
    const uint64_t knext = has_next ? key[wbase + FC1_WAVE_ITEMS] >> cmp_shift : 0ull;
    // the positions are not needed before the offsets are known: their loads overlap the flags and the look-back
    uint32_t p0[FC1_CHUNKS], p1[FC1_CHUNKS];
#pragma unroll
    for (int j = 0; j < FC1_CHUNKS; j++) {
        const uint64_t a = wbase + (uint64_t)j * 128 + 2 * lane;
        if (full) {
            const uint2 t = *reinterpret_cast<const uint2 *>(pos + a);
            p0[j] = t.x;
            p1[j] = t.y;
        } else {
            p0[j] = a < count ? pos[a] : 0u;
            p1[j] = a + 1 < count ? pos[a + 1] : 0u;
        }
    }
#ifdef FC_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FC_MARK(1); // keys, neighbours and positions have arrived
#endif
    // head(i) = item i starts a segment (differs from item i - 1; items past the end count as heads)
    uint32_t h01 = 0;        // my own head bits: bit 2j = first item, bit 2j + 1 = second item of chunk j
#pragma unroll
    for (int j = 0; j < FC1_CHUNKS; j++) {
        const uint64_t a = wbase + (uint64_t)j * 128 + 2 * lane;
        uint64_t up = __shfl_up(k1[j], 1, 64); // the second item of the lane below
        const uint64_t before = j == 0 ? kprev : lane_value_u64(k1[j > 0 ? j - 1 : 0], 63);
        if (lane == 0) up = before;
        const bool h0 = a == 0 || a >= count || up != k0[j];
        const bool h1 = a + 1 >= count || k0[j] != k1[j];
        h01 |= (h0 ? 1u : 0u) << (2 * j) | (h1 ? 1u : 0u) << (2 * j + 1);
    }
    // the head bits of the lane above, and of lane 0: the item after lane 63's second one is lane 0's first of the next chunk
    const uint32_t h01_up = __shfl_down(h01, 1, 64);
    const uint32_t h01_l0 = (uint32_t)__builtin_amdgcn_readlane((int)h01, 0);
    const bool next_head = !has_next || lane_value_u64(k1[FC1_CHUNKS - 1], 63) != knext; // head(first item after my wave)
    // survivors (tied with a neighbour) and the heads among them; ranks inside the wave
    uint32_t fl = 0;                              // bits 4j .. 4j+3: surv0, surv1, headsurv0, headsurv1
                                                  // (PAIRS) bits 16+2j, 17+2j: my first / second item is the first member of a pair
    // survivors / surviving heads / (PAIRS) pairs of my wave in front of my first item of chunk j: each below FC1_WAVE_ITEMS,
    // 10 bits a piece in one word (a word each costs eight registers more, which the kernel with PAIRS does not have)
    uint32_t rk[FC1_CHUNKS];
    static_assert(FC1_WAVE_ITEMS < 1024, "rank fields of 10 bits");
    uint32_t run_s = 0, run_h = 0, run_p = 0;     // (wave-uniform running totals)
    uint32_t pair_carry = 0; // (PAIRS, wave-uniform) lane 63's second item of the chunk before is the first member of a pair
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < FC1_CHUNKS; j++) {
        // (flags as 0 / 1 words, not bools: a bool of a lane is a 64-bit wave mask in scalar registers, and four chunks'
        //  worth of them at once do not fit the scalar file)
        const uint32_t h0 = (h01 >> (2 * j)) & 1u, h1 = (h01 >> (2 * j + 1)) & 1u;
        // bit 0: head(item after my second), bit 1: head(the one after that; 0 past my wave's stretch)
        const uint32_t nb = lane < 63u ? h01_up >> (2 * j) : (j + 1 < FC1_CHUNKS ? h01_l0 >> (2 * j + 2) : (next_head ? 1u : 0u));
        const uint32_t hn = nb & 1u;
        // (items past the end are heads and so is everything after them: they are no survivors without a look at `count`)
        uint32_t s0 = (h0 & h1) ^ 1u, s1 = (h1 & hn) ^ 1u;
        if (PAIRS) {
            const uint32_t hnn = (nb >> 1) & 1u;
            const uint32_t pf0 = h0 & (h1 ^ 1u) & hn;          // my two items are a pair
            const uint32_t pf1 = h1 & (hn ^ 1u) & hnn;         // my second item and the one after it (never the last of the stretch)
            uint32_t ps0 = __shfl_up(pf1, 1, 64);              // my first item is the second member of the lane below's pair
            if (lane == 0u) ps0 = pair_carry;
            pair_carry = (uint32_t)__builtin_amdgcn_readlane((int)pf1, 63);
            s0 &= (pf0 | ps0) ^ 1u;
            s1 &= (pf1 | pf0) ^ 1u;
            const uint64_t PF = __ballot((pf0 | pf1) != 0u); // (pf0 and pf1 of one lane exclude each other)
            rk[j] = (run_p + (uint32_t)__popcll(PF & below)) << 20;
            run_p += (uint32_t)__popcll(PF);
            fl |= (pf0 | (pf1 << 1)) << (16 + 2 * j);
        }
        const uint32_t m0 = s0 & h0, m1 = s1 & h1;
        const uint64_t S0 = __ballot(s0 != 0u), S1 = __ballot(s1 != 0u), M0 = __ballot(m0 != 0u), M1 = __ballot(m1 != 0u);
        if (!PAIRS) rk[j] = 0;
        rk[j] |= run_s + (uint32_t)__popcll(S0 & below) + (uint32_t)__popcll(S1 & below);
        rk[j] |= (run_h + (uint32_t)__popcll(M0 & below) + (uint32_t)__popcll(M1 & below)) << 10;
        run_s += (uint32_t)__popcll(S0) + (uint32_t)__popcll(S1);
        run_h += (uint32_t)__popcll(M0) + (uint32_t)__popcll(M1);
        fl |= (s0 | (s1 << 1) | (m0 << 2) | (m1 << 3)) << (4 * j);
    }
    if (lane == 0) {
        ws[wave][0] = run_s;
        ws[wave][1] = run_h;
        ws[wave][2] = run_p;
    }
    FC_MARK(2); // flags and ranks of my wave
    __syncthreads();
    FC_MARK(3); // ... of the slowest wave
    uint32_t ts = 0, th = 0, tp = 0, ws0 = 0, wh0 = 0, wp0 = 0; // tile totals; totals of the waves before mine
#pragma unroll
    for (int w = 0; w < FC1_THREADS / 64; w++) {
        if (w < wave) {
            ws0 += ws[w][0];
            wh0 += ws[w][1];
            if (PAIRS) wp0 += ws[w][2];
        }
        ts += ws[w][0];
        th += ws[w][1];
        if (PAIRS) tp += ws[w][2];
    }
    if (wave == 0) {
        constexpr uint64_t M31 = 0x7FFFFFFFull;
        const uint64_t mine = ((uint64_t)ts << 31) | (uint64_t)th;
        constexpr uint64_t M62 = (1ull << 62) - 1ull;
        uint64_t es = 0, eh = 0, ep = 0; // survivors / heads / pairs in all earlier tiles
        if (tile == 0) {
            if (lane == 0) {
                __hip_atomic_store(&desc[0], (2ull << 62) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (PAIRS) __hip_atomic_store(&desc[1], (2ull << 62) | (uint64_t)tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (lane == 0) {
                __hip_atomic_store(&desc[DS * tile], (1ull << 62) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (PAIRS)
                    __hip_atomic_store(&desc[DS * tile + 1], (1ull << 62) | (uint64_t)tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            int64_t base = (int64_t)tile;
            uint32_t spins = 0;
            for (;;) {
                const int64_t t = base - 1 - (int64_t)lane;
                const uint64_t v = t >= 0 ? __hip_atomic_load(&desc[DS * t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                          : (2ull << 62); // in front of tile 0: nothing
                uint32_t st = (uint32_t)(v >> 62);
                uint64_t v2 = 0;
                if (PAIRS) {
                    v2 = t >= 0 ? __hip_atomic_load(&desc[DS * t + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (2ull << 62);
                    if ((uint32_t)(v2 >> 62) != st) st = 0; // caught between its two stores: not ready, read again
                }
                const uint64_t incl = __ballot(st == 2u), ready = __ballot(st != 0u);
                const uint32_t first = incl ? (uint32_t)__builtin_ctzll(incl) : 64u;      // nearest running total
                const uint64_t need = first >= 63u ? ~0ull : ((2ull << first) - 1ull); // lanes 0 .. first
                if ((ready & need) != need) { // a predecessor this side of it has not published yet
                    if (++spins > FC1_SPIN_LIMIT) {
                        if (lane == 0) *err = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                uint64_t a = lane <= first ? (v >> 31) & M31 : 0ull, b = lane <= first ? v & M31 : 0ull;
                uint64_t c = lane <= first ? v2 & M62 : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    a += __shfl_xor(a, d, 64);
                    b += __shfl_xor(b, d, 64);
                    if (PAIRS) c += __shfl_xor(c, d, 64);
                }
                es += a;
                eh += b;
                ep += c;
                if (first < 64u) break;
                base -= 64;
            }
            if (lane == 0) {
                __hip_atomic_store(&desc[DS * tile], (2ull << 62) | ((es + ts) << 31) | (eh + th), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                if (PAIRS)
                    __hip_atomic_store(&desc[DS * tile + 1], (2ull << 62) | (ep + tp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (lane == 0) {
            s_excl[0] = (uint32_t)es;
            s_excl[1] = (uint32_t)eh;
            s_excl[2] = (uint32_t)ep;
            if (tile + 1 == tiles) {
                total[0] = ((es + ts) << 32) | (eh + th);
                total[1] = ep + tp; // (0 without PAIRS)
            }
        }
    }
    FC_MARK(4); // look-back (wave 0)
    __syncthreads();
    FC_MARK(5);
    if (wbase >= count) return;
    const uint32_t bs = s_excl[0] + ws0, bh = s_excl[1] + wh0, bp = s_excl[2] + wp0;
    // the store phase works its addresses and bounds out anew: computed ahead of the look-back and kept across it, they
    // are what pushes the kernel past its registers
    uint32_t lane_st = lane;
    asm volatile("" : "+v"(lane_st));
#pragma unroll KISS_FC1_STORE_UNROLL
    for (int j = 0; j < FC1_CHUNKS; j++) {
        const uint64_t a = wbase + (uint64_t)j * 128 + 2 * lane_st;
        const uint32_t f = (fl >> (4 * j)) & 15u;
        const uint32_t ni0 = bs + (rk[j] & 1023u), ni1 = ni0 + (f & 1u);
        const uint32_t sid0 = bh + ((rk[j] >> 10) & 1023u) + ((f >> 2) & 1u) - 1u;   // heads up to and including the item's own, minus one
        const uint32_t sid1 = sid0 + ((f >> 3) & 1u);
        if (f & 1u) {
            if (ni0 < cap) {
                npos[ni0] = p0[j];
                nslot[ni0] = (uint32_t)a;
                nseg[ni0] = sid0;
                if (f & 4u) nsegstart[sid0] = ni0;
                if (nctx) nctx[ni0] = c0[j]; // travels with the tied item through the first refinement round
            }
            c0[j] = 0; // tied so far: written when the item is finished, else gathered at placement
        }
        if (f & 2u) {
            if (ni1 < cap) {
                npos[ni1] = p1[j];
                nslot[ni1] = (uint32_t)(a + 1);
                nseg[ni1] = sid1;
                if (f & 8u) nsegstart[sid1] = ni1;
                if (nctx) nctx[ni1] = c1[j];
            }
            c1[j] = 0;
        }
        if (full) *reinterpret_cast<uint2 *>(octx + a) = make_uint2(c0[j], c1[j]);
        else {
            if (a < count) octx[a] = c0[j];
            if (a + 1 < count) octx[a + 1] = c1[j];
        }
    }
    if (PAIRS) {
#pragma unroll
        for (int j = 0; j < FC1_CHUNKS; j++) {
            const uint32_t a32 = (uint32_t)wbase + (uint32_t)j * 128u + 2u * lane_st; // (a slot: the list has fewer than 2^32 items)
            const uint32_t pf = (fl >> (16 + 2 * j)) & 3u;
            // the item after my second one: the first item of the lane above, of lane 0 of the next chunk for lane 63
            uint32_t pn = __shfl_down(p0[j], 1, 64);
            if (j + 1 < FC1_CHUNKS) {
                const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)p0[j + 1 < FC1_CHUNKS ? j + 1 : j], 0);
                if (lane == 63u) pn = w0;
            }
            if (pf) { // records in list order: a wave's stores of one chunk go to consecutive records
                const uint32_t ri = bp + (rk[j] >> 20);
                rec[ri] = (pf & 1u) ? p0[j] : p1[j];
                rec[rcol + ri] = (pf & 1u) ? p1[j] : pn;
                rec[2u * rcol + ri] = a32 + (pf >> 1);
            }
        }
    }
    FC_MARK(6); // stores issued
#ifdef FC_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FC_MARK(7); // stores done
#endif
}

// ---- tie flags as bytes (the doubling phase's first compaction over all n + 1 suffixes): 8 flags per load, and the
// suffix array is read only for the few entries that are tied ------------------------------------------------
__device__ __forceinline__ void fch_flags(const uint8_t *__restrict__ hb, uint64_t i0, uint64_t count, uint32_t &valid,
                                          uint32_t &survmask, uint32_t &headmask)
{
    valid = i0 >= count ? 0u : (count - i0 >= FC_ITEMS ? (uint32_t)FC_ITEMS : (uint32_t)(count - i0));
    survmask = headmask = 0;
    if (!valid) return;
    uint8_t h[FC_ITEMS + 1];
    if (valid == FC_ITEMS) {
        const uint64_t w = *reinterpret_cast<const uint64_t *>(hb + i0);
#pragma unroll
        for (int e = 0; e < FC_ITEMS; e++) h[e] = (uint8_t)(w >> (8 * e));
    } else {
#pragma unroll
        for (int e = 0; e < FC_ITEMS; e++) h[e] = (uint32_t)e < valid ? hb[i0 + e] : (uint8_t)1;
    }
    h[FC_ITEMS] = i0 + FC_ITEMS < count ? hb[i0 + FC_ITEMS] : (uint8_t)1;
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        if ((uint32_t)e < valid) {
            const uint64_t i = i0 + (uint64_t)e;
            const bool head = i == 0 || h[e] != 0;
            const bool nhead = i + 1 == count || h[e + 1] != 0;
            const bool surv = !(head && nhead);
            survmask |= (surv ? 1u : 0u) << e;
            headmask |= ((surv && head) ? 1u : 0u) << e;
        }
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_fch_count(const uint8_t *__restrict__ hb, uint64_t count,
                                                         uint64_t *__restrict__ tcnt)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint32_t valid, sm, hm;
    fch_flags(hb, i0, count, valid, sm, hm);
    uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ns += __shfl_xor(ns, d, 64);
        nh += __shfl_xor(nh, d, 64);
    }
    if (lane_id() == 0) {
        ws[threadIdx.x >> 6][0] = ns;
        ws[threadIdx.x >> 6][1] = nh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int w = 0; w < FC_THREADS / 64; w++) {
            a += ws[w][0];
            b += ws[w][1];
        }
        tcnt[blockIdx.x] = (a << 32) | b;
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_fch_compact(const uint8_t *__restrict__ hb,
                                                           const uint32_t *__restrict__ pos, uint64_t count,
                                                           const uint64_t *__restrict__ tex, uint32_t *__restrict__ npos,
                                                           uint32_t *__restrict__ nslot, uint32_t *__restrict__ nseg,
                                                           uint32_t *__restrict__ nsegstart)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint32_t valid, sm, hm;
    fch_flags(hb, i0, count, valid, sm, hm);
    const uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
    uint32_t is = ns, ih = nh;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t os = __shfl_up(is, d, 64), oh = __shfl_up(ih, d, 64);
        if ((int)lane_id() >= d) {
            is += os;
            ih += oh;
        }
    }
    if (lane_id() == 63) {
        ws[wave][0] = is;
        ws[wave][1] = ih;
    }
    __syncthreads();
    const uint64_t te = tex[blockIdx.x];
    uint32_t bs = (uint32_t)(te >> 32) + (is - ns), bh = (uint32_t)(te & 0xFFFFFFFFull) + (ih - nh);
    for (int w = 0; w < wave; w++) {
        bs += ws[w][0];
        bh += ws[w][1];
    }
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        if ((sm >> e) & 1u) {
            const uint32_t ni = bs++;
            if ((hm >> e) & 1u) bh++;
            const uint32_t sid = bh - 1u;
            npos[ni] = pos[i0 + e];
            nslot[ni] = (uint32_t)(i0 + e);
            nseg[ni] = sid;
            if ((hm >> e) & 1u) nsegstart[sid] = ni;
        }
    }
}

__global__ void k_fc_total(const uint64_t *__restrict__ tcnt, const uint64_t *__restrict__ tex, uint64_t tiles,
                           uint64_t *__restrict__ total)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) total[0] = tex[tiles - 1] + tcnt[tiles - 1];
}

// ---- the items of big segments after a refinement round (k_seg_finish's byte flags): count per tile, scan over tiles,
// compact -- the tile-wise form of the flag + compaction above ---------------------------------------------------------
__device__ __forceinline__ void bigb_flags(const uint8_t *__restrict__ bb, uint64_t i0, uint64_t count, uint32_t &valid,
                                           uint32_t &bigmask, uint32_t &headmask)
{
    valid = i0 >= count ? 0u : (count - i0 >= FC_ITEMS ? (uint32_t)FC_ITEMS : (uint32_t)(count - i0));
    bigmask = headmask = 0;
    if (!valid) return;
    uint64_t w = 0;
    if (valid == FC_ITEMS) w = *reinterpret_cast<const uint64_t *>(bb + i0);
    else
        for (uint32_t e = 0; e < valid; e++) w |= (uint64_t)bb[i0 + e] << (8 * e);
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        const uint32_t f = (uint32_t)(w >> (8 * e)) & 3u;
        bigmask |= (f & 1u) << e;
        headmask |= (f >> 1) << e;
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_bigb_count(const uint8_t *__restrict__ bb, uint64_t count,
                                                          uint64_t *__restrict__ tcnt)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint32_t valid, sm, hm;
    bigb_flags(bb, i0, count, valid, sm, hm);
    uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ns += __shfl_xor(ns, d, 64);
        nh += __shfl_xor(nh, d, 64);
    }
    if (lane_id() == 0) {
        ws[threadIdx.x >> 6][0] = ns;
        ws[threadIdx.x >> 6][1] = nh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int w = 0; w < FC_THREADS / 64; w++) {
            a += ws[w][0];
            b += ws[w][1];
        }
        tcnt[blockIdx.x] = (a << 32) | b;
    }
}

__global__ __launch_bounds__(FC_THREADS) void k_bigb_compact(const uint8_t *__restrict__ bb, const uint64_t *__restrict__ key,
                                                            const uint32_t *__restrict__ pos,
                                                            const uint32_t *__restrict__ slot, uint64_t count,
                                                            const uint64_t *__restrict__ tex, uint64_t *__restrict__ bkey,
                                                            uint32_t *__restrict__ bpos, uint32_t *__restrict__ bseg,
                                                            uint32_t *__restrict__ bslot, uint32_t *__restrict__ bsegstart)
{
    __shared__ uint32_t ws[FC_THREADS / 64][2];
    const int wave = threadIdx.x >> 6;
    const uint64_t i0 = ((uint64_t)blockIdx.x * FC_THREADS + threadIdx.x) * FC_ITEMS;
    uint32_t valid, sm, hm;
    bigb_flags(bb, i0, count, valid, sm, hm);
    const uint32_t ns = (uint32_t)__popc(sm), nh = (uint32_t)__popc(hm);
    uint32_t is = ns, ih = nh;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t os = __shfl_up(is, d, 64), oh = __shfl_up(ih, d, 64);
        if ((int)lane_id() >= d) {
            is += os;
            ih += oh;
        }
    }
    if (lane_id() == 63) {
        ws[wave][0] = is;
        ws[wave][1] = ih;
    }
    __syncthreads();
    const uint64_t te = tex[blockIdx.x];
    uint32_t bs = (uint32_t)(te >> 32) + (is - ns), bh = (uint32_t)(te & 0xFFFFFFFFull) + (ih - nh);
    for (int w = 0; w < wave; w++) {
        bs += ws[w][0];
        bh += ws[w][1];
    }
#pragma unroll
    for (int e = 0; e < FC_ITEMS; e++) {
        if ((sm >> e) & 1u) {
            const uint32_t kx = bs++;
            if ((hm >> e) & 1u) bh++;
            const uint32_t sid = bh - 1u; // big-segment heads up to and including this item's own
            if (key) bkey[kx] = key[i0 + e]; // (null: a pivot round follows, which keys the members against its reference string)
            bpos[kx] = pos[i0 + e];
            bslot[kx] = slot[i0 + e]; // slots stay in index order: the k-th item after the sort takes the k-th slot
            bseg[kx] = sid;
            if ((hm >> e) & 1u) bsegstart[sid] = kx;
        }
    }
}

// members of long groups -> compact arrays (dense group ids), remembering where they came from
__global__ __launch_bounds__(LS_THREADS) void k_big_extract(const uint64_t *__restrict__ key,
                                                           const uint32_t *__restrict__ pos, uint64_t count,
                                                           const uint64_t *__restrict__ big,
                                                           const uint64_t *__restrict__ ex, uint64_t *__restrict__ bkey,
                                                           uint32_t *__restrict__ bpos, uint32_t *__restrict__ bseg,
                                                           uint32_t *__restrict__ bidx)
{
    const uint64_t i = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (i >= count) return;
    const uint64_t f = big[i];
    if (!(f >> 32)) return;
    const uint64_t e = ex[i];
    const uint32_t kx = (uint32_t)(e >> 32);
    bkey[kx] = key[i];
    bpos[kx] = pos[i];
    bseg[kx] = (uint32_t)(e & 0xFFFFFFFFull) + (uint32_t)(f & 1ull) - 1u;
    bidx[kx] = (uint32_t)i;
}

// sorted on (group, key): the c-th item goes back to where the c-th extracted item came from
__global__ __launch_bounds__(LS_THREADS) void k_big_writeback(const uint64_t *__restrict__ skey,
                                                             const uint32_t *__restrict__ spos,
                                                             const uint32_t *__restrict__ bidx, uint64_t nbig,
                                                             uint64_t *__restrict__ okey, uint32_t *__restrict__ opos)
{
    const uint64_t c = (uint64_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (c >= nbig) return;
    const uint32_t i = bidx[c];
    okey[i] = skey[c];
    opos[i] = spos[c];
}

__global__ void k_last_total(const uint64_t *__restrict__ flags, const uint64_t *__restrict__ ex, uint64_t count,
                             uint64_t *__restrict__ total)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) total[0] = ex[count - 1] + flags[count - 1];
}

__global__ void k_set_u32(uint32_t *p, uint32_t v, uint32_t *zero_me)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *p = v;
        if (zero_me) *zero_me = 0;
    }
}

// The other half of k_ctx_lengths_anchor in lms_sort.hip: k_fc_compact gathers context words of KISS_CTX_BASES bases, and
// this never-launched second caller of kiss_load_ctx_n keeps the helper from being specialised for that one length, so the
// four k_fc_compact kernels stay the code they were while k_pivot_lcp was compiled in the same unit.
__global__ void k_ctx_lengths_anchor(const uint64_t *pk, uint32_t *out)
{
    out[threadIdx.x] = kiss_load_ctx_n(pk, out[threadIdx.x + 64], KISS_KEY_CTX_BASES);
}

} // namespace

namespace {

// the kernel of a count pass: the narrow forms where they apply, else k_fc_count
template <int SRC>
void launch_fc_count(kiss_hip_ctx *ctx, const FcJob &j, uint64_t tiles, uint64_t *tcnt)
{
    const dim3 grid((unsigned)tiles), block(FC_THREADS);
    if (SRC == FC_HEADS)
        hipLaunchKernelGGL(k_fch_count, grid, block, 0, ctx->stream, reinterpret_cast<const uint8_t *>(j.key), j.count, tcnt);
    else if (SRC == FC_KEY && !j.last_round)
        hipLaunchKernelGGL(k_fc0_count, grid, block, 0, ctx->stream, j.key, j.count, j.cmp_shift, tcnt);
    else
        hipLaunchKernelGGL((k_fc_count<SRC>), grid, block, 0, ctx->stream, j.key, j.seg, j.count, j.cmp_shift, j.last_round, tcnt);
}

// ... and of the compaction behind it: tex = the exclusive scan of that pass's tile counts
template <int SRC, bool HAS_SLOT>
void launch_fc_compact(kiss_hip_ctx *ctx, const FcJob &j, const FcOut &to, uint64_t tiles, const uint64_t *tex, bool *nctx_written)
{
    const dim3 grid((unsigned)tiles), block(FC_THREADS);
    uint8_t *hmark = j.tmark ? ctx->hfar : nullptr; // (the calls that mark taints are the retirements of the LMS sort)
    const bool survivors_only = !j.out && !j.isa && !j.octx;
    const bool round0 = !j.last_round && j.out && j.octx && !j.isa && j.cmp_shift >= 24;
    if (SRC == FC_HEADS && !HAS_SLOT && survivors_only)
        hipLaunchKernelGGL(k_fch_compact, grid, block, 0, ctx->stream, reinterpret_cast<const uint8_t *>(j.key), j.pos, j.count, tex,
                           to.npos, to.nslot, to.nseg, to.nsegstart);
    else if (SRC == FC_KEY && !HAS_SLOT && round0) {
        hipLaunchKernelGGL(k_fc0_compact, grid, block, 0, ctx->stream, j.key, j.pos, j.count, j.cmp_shift, tex, to.npos, to.nslot,
                           to.nseg, to.nsegstart, j.out == j.pos ? (uint32_t *)nullptr : j.out, j.octx, j.nctx);
        if (nctx_written) *nctx_written = j.nctx != nullptr;
    } else // (without slots an item's slot is its index: out == pos means the list is in place already)
        hipLaunchKernelGGL((k_fc_compact<SRC, HAS_SLOT>), grid, block, 0, ctx->stream, j.key, j.seg, j.pos, j.slot, j.count,
                           j.cmp_shift, j.last_round, tex, to.npos, to.nslot, to.nseg, to.nsegstart,
                           (!HAS_SLOT && j.out == j.pos) ? (uint32_t *)nullptr : j.out, j.isa, j.octx, j.tmark, j.payload,
                           j.isa_shift, j.cfix ? ctx->pk : (const uint64_t *)nullptr, j.cfix, hmark);
}

#ifdef FC_PROF
int fc_prof_report(kiss_hip_ctx *ctx, uint64_t tiles)
{
    unsigned long long h[12], z[12] = {0};
    KCHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(fc_prof), sizeof h));
    KCHECK(hipMemcpyToSymbol(HIP_SYMBOL(fc_prof), z, sizeof z));
    unsigned long long sum = 0;
    for (int i = 0; i < 8; i++) sum += h[i];
    fprintf(stderr, "[fc_prof] %llu tiles, %.2f us per tile (100 MHz clock):", (unsigned long long)tiles, (double)sum / 100.0 / (double)tiles);
    for (int i = 0; i < 8; i++) fprintf(stderr, " %d:%.1f%%", i, sum ? 100.0 * (double)h[i] / (double)sum : 0.0);
    fprintf(stderr, "\n");
    return KISS_HIP_OK;
}
#endif

} // namespace

namespace kiss_fc {

int tiles_total(kiss_hip_ctx *ctx, const uint64_t *tcnt, uint64_t *tex, uint64_t tiles, uint64_t *d_total, uint64_t *host_total)
{
    KTRY(kiss_scan_u64(ctx, tcnt, tex, tiles));
    hipLaunchKernelGGL(k_fc_total, dim3(1), dim3(64), 0, ctx->stream, tcnt, tex, tiles, d_total);
    KCHECK(hipGetLastError());
    return host_total ? read_u64(ctx, d_total, host_total) : KISS_HIP_OK;
}

int flags_total(kiss_hip_ctx *ctx, const uint64_t *flags, uint64_t *ex, uint64_t count, uint64_t *d_total, uint64_t *host_total)
{
    KTRY(kiss_scan_u64(ctx, flags, ex, count));
    hipLaunchKernelGGL(k_last_total, dim3(1), dim3(64), 0, ctx->stream, flags, ex, count, d_total);
    KCHECK(hipGetLastError());
    return host_total ? read_u64(ctx, d_total, host_total) : KISS_HIP_OK;
}

// The instantiations in use: keys in round 0 and in the closing compaction of a round (with segment ids and slots), head
// bytes with slots (pivot rounds) and without (the first compaction of the doubling forms).
int fc_count(kiss_hip_ctx *ctx, const FcJob &j, uint64_t *d_total)
{
    const uint64_t tiles = div_up(j.count, FC_TILE);
    if (2 * tiles > ctx->flags_cap) return KINTERNAL();
    uint64_t *tcnt = ctx->flags, *tex = ctx->flags + tiles;
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, j.count);
        switch (j.src) {
        case FC_KEY: launch_fc_count<FC_KEY>(ctx, j, tiles, tcnt); break;
        case FC_KEY_SEG: launch_fc_count<FC_KEY_SEG>(ctx, j, tiles, tcnt); break;
        case FC_HEADS: launch_fc_count<FC_HEADS>(ctx, j, tiles, tcnt); break;
        default: return KINTERNAL();
        }
        KCHECK(hipGetLastError());
    }
    return tiles_total(ctx, tcnt, tex, tiles, d_total);
}

int fc_compact(kiss_hip_ctx *ctx, const FcJob &j, const FcOut &to, bool *nctx_written)
{
    if (nctx_written) *nctx_written = false;
    const uint64_t tiles = div_up(j.count, FC_TILE);
    const uint64_t *tex = ctx->flags + tiles; // left there by fc_count
    const bool has_slot = j.slot != nullptr;
    KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, j.count);
    if (j.src == FC_KEY && !has_slot) launch_fc_compact<FC_KEY, false>(ctx, j, to, tiles, tex, nctx_written);
    else if (j.src == FC_KEY_SEG && has_slot) launch_fc_compact<FC_KEY_SEG, true>(ctx, j, to, tiles, tex, nctx_written);
    else if (j.src == FC_HEADS && has_slot) launch_fc_compact<FC_HEADS, true>(ctx, j, to, tiles, tex, nctx_written);
    else if (j.src == FC_HEADS) launch_fc_compact<FC_HEADS, false>(ctx, j, to, tiles, tex, nctx_written);
    else return KINTERNAL();
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}

bool fc0_onepass_fits(const kiss_hip_ctx *ctx, uint64_t count)
{
    const uint64_t tiles = div_up(count, FC1_TILE);
    return ctx->fc_desc && tiles >= 8 && 2 * tiles + 1 <= ctx->fc_desc_cap;
}

int fc0_onepass(kiss_hip_ctx *ctx, const Fc0Job &j, const FcOut &to, uint64_t *d_total, uint64_t *tot, uint64_t *npairs)
{
    const uint64_t tiles = div_up(j.count, FC1_TILE);
    uint64_t *desc = ctx->fc_desc;
    uint32_t *ticket = reinterpret_cast<uint32_t *>(desc + 2 * tiles);
    KTRY(kiss_zero_u32(ctx, desc, 4 * tiles + 2));
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, j.count);
        if (j.rec)
            hipLaunchKernelGGL(k_fc0_onepass<true>, dim3((unsigned)tiles), dim3(FC1_THREADS), 0, ctx->stream, j.key, j.pos, j.count,
                               j.cmp_shift, tiles, desc, ticket, ctx->rx_ctl + 1, to.npos, to.nslot, to.nseg, to.nsegstart, j.octx,
                               j.nctx, ctx->t_cap, d_total, j.rec, j.rcol);
        else
            hipLaunchKernelGGL(k_fc0_onepass<false>, dim3((unsigned)tiles), dim3(FC1_THREADS), 0, ctx->stream, j.key, j.pos, j.count,
                               j.cmp_shift, tiles, desc, ticket, ctx->rx_ctl + 1, to.npos, to.nslot, to.nseg, to.nsegstart, j.octx,
                               j.nctx, ctx->t_cap, d_total, (uint32_t *)nullptr, 0u);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_readback(ctx, d_total, 4)); // (survivors << 32 | heads), pairs
    std::memcpy(tot, ctx->h_pinned, sizeof(uint64_t));
    std::memcpy(npairs, ctx->h_pinned + 2, sizeof(uint64_t));
#ifdef FC_PROF
    KTRY(fc_prof_report(ctx, tiles));
#endif
    return KISS_HIP_OK;
}

int bigb_count(kiss_hip_ctx *ctx, const uint8_t *bb, uint64_t count, uint64_t *d_total, uint64_t *tot)
{
    const uint64_t tiles = div_up(count, FC_TILE);
    uint64_t *tcnt = ctx->flags, *tex = ctx->flags + tiles;
    if (2 * tiles > ctx->t_cap) return KINTERNAL();
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, count);
        hipLaunchKernelGGL(k_bigb_count, dim3((unsigned)tiles), dim3(FC_THREADS), 0, ctx->stream, bb, count, tcnt);
        KCHECK(hipGetLastError());
    }
    return tiles_total(ctx, tcnt, tex, tiles, d_total, tot);
}

int bigb_compact(kiss_hip_ctx *ctx, const uint8_t *bb, const uint64_t *key, const uint32_t *pos, const uint32_t *slot,
                 uint64_t count, const BigbOut &to, uint64_t nbig, uint64_t nbigseg)
{
    const uint64_t tiles = div_up(count, FC_TILE);
    KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, count);
    hipLaunchKernelGGL(k_bigb_compact, dim3((unsigned)tiles), dim3(FC_THREADS), 0, ctx->stream, bb, key, pos, slot, count,
                       ctx->flags + tiles /* left there by bigb_count */, to.bkey, to.bpos, to.bseg, to.bslot, to.bsegstart);
    set_u32(ctx, to.bsegstart + nbigseg, (uint32_t)nbig);
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}

int sort_big_members(kiss_hip_ctx *ctx, const BigSort &b)
{
    auto sync_point = [&](unsigned i) {
        if ((b.sync_points >> i) & 1u) (void)hipStreamSynchronize(ctx->stream);
    };
    RadixBufs rb;
    for (int i = 0; i < 2; i++) {
        rb.key[i] = b.kbuf[i];
        rb.pos[i] = b.pbuf[i];
        rb.seg[i] = b.sbuf[i];
    }
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, b.count);
        hipLaunchKernelGGL(k_big_extract, dim3((unsigned)div_up(b.count, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, b.key, b.pos,
                           b.count, b.flags, b.ex, rb.key[0], rb.pos[0], rb.seg[0], b.bidx);
        KCHECK(hipGetLastError());
    }
    sync_point(2);
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, b.nbig, b.key_lo_bit, bits_for(b.ngroups), &res));
    sync_point(3);
    {
        KTimer t(ctx, KISS_HIP_K_FLAG_COMPACT, b.nbig);
        hipLaunchKernelGGL(k_big_writeback, dim3((unsigned)div_up(b.nbig, LS_THREADS)), dim3(LS_THREADS), 0, ctx->stream, rb.key[res],
                           rb.pos[res], b.bidx, b.nbig, b.okey, b.opos);
        KCHECK(hipGetLastError());
    }
    sync_point(4);
    return KISS_HIP_OK;
}

void set_u32(kiss_hip_ctx *ctx, uint32_t *p, uint32_t v, uint32_t *zero_me)
{
    hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(64), 0, ctx->stream, p, v, zero_me);
}

int read_u64(kiss_hip_ctx *ctx, const void *dptr, uint64_t *out)
{
    KTRY(kiss_readback(ctx, dptr, 2));
    std::memcpy(out, ctx->h_pinned, sizeof(uint64_t));
    return KISS_HIP_OK;
}

int bits_for(uint64_t count)
{
    int b = 0;
    if (count > 1) {
        uint64_t v = count - 1;
        while (v) {
            b++;
            v >>= 1;
        }
    }
    return b;
}

} // namespace kiss_fc
