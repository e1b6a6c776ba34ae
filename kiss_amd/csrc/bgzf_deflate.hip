// bgzf_deflate.hip -- BGZF blocks compressed on the GPU (kiss_hip_bgzf_deflate_*).  The definition is in
// include/kiss_hip_deflate.h and restated in tests/deflate_model.py; DESIGN.md 4.23.
//
// k_deflate_block: ONE WORKGROUP OF 256 LANES PER BLOCK (a workgroup takes blocks b, b + gridDim.x, ...; the grid is one workgroup
// per CU, which is what its LDS lets a CU hold).  The workgroup owns the whole chain of one block:
//   stage : the payload into LDS once, as aligned words of the source funnelled to byte phase 0; the CRC-32 from LDS in 256 pieces
//           (bgzf_block.hpp, shared with fm_bam.hip).
//   match : segment by segment (256 positions, a lane each).  A lane hashes its four bytes, looks up T (8192 entries in LDS:
//           position + 1, the largest of the EARLIER segments, 0 empty) and compares both candidates word-wide from LDS.  The greedy
//           parse is resolved inside the segment: next[p] = p + max(1, len) is a chain from the carry-in start, found by pointer
//           doubling over the 256 entries (8 rounds).  The chosen positions are compacted by a ballot prefix into the token list (4
//           bytes a token, in global scratch: a slot per RESIDENT workgroup) and counted into the two histograms in LDS; then the
//           segment's positions enter T with atomicMax, so the order of the lanes cannot matter.
//   code  : the counts ranked by comparison across the lanes; the two-queue merge, the depths, the canonical codes and the three
//           exact costs by lane 0 (a few hundred steps each).
//   pack  : a stored block is copied out of LDS as k_bgzf does it.  Otherwise the payload's LDS becomes the bit stream: lane 0 writes
//           the header, then 256 tokens at a time get their bit offsets from a prefix sum with a running carry and OR their (at most
//           48) bits into the words; the stream is copied out word-wide.
// The block lands in a slot of its own (stride: block_bytes + 31 rounded up to 16, + 16); a u64 scan of the sizes and
// k_deflate_pack move the blocks together into out, word-wide, and write block_index and the end-of-file block.
//
// ADDRESSING.  Every global address is a kernel-argument base pointer plus a 64-bit offset, and what crosses lanes by ballot or
// shuffle (the votes, the prefix sums) is unsigned and indexes LDS only.  ONE EXCEPTION to "no pointer crosses lanes": the arguments
// a block needs only at its two ends (data, n, the slot base and stride, sizes) are parked in LDS by lane 0 and read back by all
// lanes through v_readfirstlane (df_parked), as two halves, each cast to uint32_t BEFORE it is widened: the builtin returns a
// signed int, and a low half of 2^31 or more widened with its sign fills the high half with ones (in the assembly: s_bfe_i64 with
// 0x200000 -- there must be none).  No scratch memory.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_deflate.h"

namespace {

#include "bgzf_block.hpp"

constexpr uint32_t DF_SEG = 256, DF_HASH_BITS = 13, DF_HASH_MUL = 0x9E3779B1u;
constexpr uint32_t DF_MIN_MATCH = 4, DF_MAX_MATCH = 258, DF_MAX_DIST = 32768;
constexpr uint32_t DF_LL = 286, DF_LL_ROOM = 288, DF_D = 30, DF_D_ROOM = 32, DF_CL = 19, DF_CL_ROOM = 20;
constexpr uint32_t DF_TOKEN_SLOT = 65536; // the tokens of one block: at most 65505
constexpr uint32_t DF_MATCH = 0x80000000u; // a token: this bit, (len - 3) << 16, dist - 1; or a literal's byte
enum { DF_STORED, DF_FIXED, DF_DYNAMIC, DF_LITERALS, DF_MATCHES, DF_MATCH_BYTES, DF_CTL_WORDS = 8 };
// what the lanes of a workgroup tell each other
enum { M_CRC, M_CARRY, M_USED, M_DEEP, M_DUSED, M_DWHICH, M_HLIT, M_HDIST, M_HCLEN, M_BTYPE, M_BITS, M_HEAD_BITS, M_LIT, M_MAT, M_MBYTES, M_WORDS };

enum { A_DATA, A_N, A_STAGE, A_STRIDE, A_SIZES, A_WORDS };

__device__ const uint8_t DF_CL_ORDER[DF_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DfLds {
    uint32_t tab[256];
    uint32_t pay[BGZF_PAY_WORDS + 4]; // the payload at byte phase 0; later the bit stream
    uint32_t T[1u << DF_HASH_BITS];
    uint32_t llc[DF_LL_ROOM], dc[DF_D_ROOM], clc[DF_CL_ROOM]; // counts
    uint32_t hc[DF_LL_ROOM], w[2 * DF_LL_ROOM];               // the counts a construction works on; the weights of its nodes
    uint16_t sorted[DF_LL_ROOM], par[2 * DF_LL_ROOM], dep[2 * DF_LL_ROOM]; // (a depth is below 286: more than a byte)
    uint16_t llcode[DF_LL_ROOM], dcode[DF_D_ROOM], clcode[DF_CL_ROOM]; // canonical codes, bit-reversed
    uint16_t jump[DF_SEG + 2];
    uint8_t lll[DF_LL_ROOM], dl[DF_D_ROOM], cll[DF_CL_ROOM];  // code lengths
    uint8_t mark[DF_SEG + 8];
    uint32_t wave[4];
    uint32_t m[M_WORDS];
    uint64_t arg[A_WORDS]; // kernel arguments that a block needs once or twice (see k_deflate_block)
};

__device__ __forceinline__ uint32_t df_ld32(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
// x, as a value the compiler does not look behind
__device__ __forceinline__ uint32_t df_fresh(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}
// a 64-bit word of LDS that all lanes read, as a value the compiler knows to be the same in all of them
__device__ __forceinline__ uint64_t df_parked(const uint64_t *p)
{
    const uint64_t v = *p;
    // (the builtin returns a signed int: each half goes back to unsigned BEFORE it is widened, or a low half of 2^31 or more
    // would fill the high half with ones)
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    return (uint64_t)hi << 32 | (uint64_t)lo;
}
// the common prefix of pb[p ..] and pb[q ..], at most cap; p + cap is inside the payload
__device__ __forceinline__ uint32_t df_match_len(const uint8_t *pb, uint32_t p, uint32_t q, uint32_t cap)
{
    uint32_t n = 0;
    while (n + 4u <= cap) {
        const uint32_t x = df_ld32(pb + p + n) ^ df_ld32(pb + q + n);
        if (x) return n + ((uint32_t)__builtin_ctz(x) >> 3);
        n += 4u;
    }
    while (n < cap && pb[p + n] == pb[q + n]) n++;
    return n;
}
// length 3 .. 258 and distance - 1 -> symbol, extra bits, their value
__device__ __forceinline__ void df_len_symbol(uint32_t len, uint32_t &sym, uint32_t &nb, uint32_t &v)
{
    const uint32_t k = len - 3u;
    if (len == 258u) {
        sym = 285u, nb = 0, v = 0;
    } else if (k < 8u) {
        sym = 257u + k, nb = 0, v = 0;
    } else {
        nb = 29u - (uint32_t)__builtin_clz(k); // floor(log2 k) - 2
        sym = 261u + 4u * nb + ((k >> nb) & 3u);
        v = k & ((1u << nb) - 1u);
    }
}
__device__ __forceinline__ void df_dist_symbol(uint32_t d, uint32_t &sym, uint32_t &nb, uint32_t &v)
{
    if (d < 4u) {
        sym = d, nb = 0, v = 0;
    } else {
        nb = 30u - (uint32_t)__builtin_clz(d); // floor(log2 d) - 1
        sym = 2u * nb + 2u + ((d >> nb) & 1u);
        v = d & ((1u << nb) - 1u);
    }
}
__device__ __forceinline__ uint32_t df_ll_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
__device__ __forceinline__ uint32_t df_d_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
__device__ __forceinline__ uint32_t df_fixed_ll(uint32_t sym) { return sym < 144u ? 8u : (sym < 256u ? 9u : (sym < 280u ? 7u : 8u)); }

// `bits` bits of v (at most 48) into the stream at bit `pos`
__device__ __forceinline__ void df_or_bits(uint32_t *words, uint32_t pos, uint64_t v, uint32_t bits)
{
    if (!bits) return;
    const uint32_t w = pos >> 5, s = pos & 31u;
    const uint32_t lo = (uint32_t)(v << s), mid = (uint32_t)(v >> (32u - s)), hi = s ? (uint32_t)(v >> (64u - s)) : 0u;
    if (lo) atomicOr(&words[w], lo);
    if (mid) atomicOr(&words[w + 1], mid);
    if (hi) atomicOr(&words[w + 2], hi);
}

// exclusive prefix sum of v over the 256 lanes (total: the sum of all); two barriers
__device__ __forceinline__ uint32_t df_scan(uint32_t t, uint32_t v, uint32_t *wave, uint32_t &total)
{
    const uint32_t lane = t & 63u, w = t >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((unsigned int)x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63u) wave[w] = x;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t s = wave[k];
        if (k < w) before += s;
        total += s;
    }
    __syncthreads();
    return before + x - v;
}

// Code lengths of the symbols [0, nsym) from cnt (LDS) within `limit` bits, into lens.  Called by all lanes; at least two counts
// are not 0.
__device__ __forceinline__ void df_huff(uint32_t t, DfLds &s, const uint32_t *cnt, uint32_t nsym, uint32_t limit, uint8_t *lens)
{
    for (uint32_t i = t; i < nsym; i += BGZF_THREADS) s.hc[i] = cnt[i];
    for (;;) {
        if (t == 0) s.m[M_USED] = 0;
        __syncthreads();
        // the used symbols sorted by (count, symbol): a rank by comparison
        for (uint32_t i = t; i < nsym; i += BGZF_THREADS) {
            const uint32_t c = s.hc[i];
            lens[i] = 0;
            if (!c) continue;
            uint32_t r = 0;
            for (uint32_t j = 0; j < nsym; j++) {
                const uint32_t o = s.hc[j];
                r += (o && (o < c || (o == c && j < i))) ? 1u : 0u;
            }
            s.sorted[r] = (uint16_t)i;
            s.w[r] = c;
            atomicAdd(&s.m[M_USED], 1u);
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t n = s.m[M_USED];
            uint32_t li = 0, ii = n;
            for (uint32_t node = n; node < 2u * n - 1u; node++) {
                uint32_t sum = 0;
                for (int k = 0; k < 2; k++) {
                    uint32_t pick;
                    if (li < n && (ii >= node || s.w[li] <= s.w[ii])) pick = li++;
                    else pick = ii++;
                    s.par[pick] = (uint16_t)node;
                    sum += s.w[pick];
                }
                s.w[node] = sum;
            }
            uint32_t deepest = 0;
            s.dep[2u * n - 2u] = 0;
            for (uint32_t node = 2u * n - 2u; node-- > 0u;) {
                const uint32_t d = (uint32_t)s.dep[s.par[node]] + 1u;
                s.dep[node] = (uint16_t)d;
                deepest = d > deepest ? d : deepest;
            }
            for (uint32_t k = 0; k < n; k++) lens[s.sorted[k]] = (uint8_t)s.dep[k]; // (read only when the deepest is within the limit of 15)
            s.m[M_DEEP] = deepest;
        }
        __syncthreads();
        if (s.m[M_DEEP] <= limit) break;
        for (uint32_t i = t; i < nsym; i += BGZF_THREADS) {
            const uint32_t c = s.hc[i];
            s.hc[i] = c ? (c + 1u) >> 1 : 0u;
        }
        __syncthreads(); // (M_DEEP is read by all before lane 0 writes it again)
    }
    __syncthreads();
}

// canonical codes of lens[0, nsym) (RFC 1951 3.2.2), each reversed to go out from its most significant bit.  One lane.
__device__ __forceinline__ void df_canonical(const uint8_t *lens, uint32_t nsym, uint16_t *codes)
{
    uint32_t count[16], next[16];
#pragma unroll
    for (int b = 0; b < 16; b++) count[b] = 0;
    for (uint32_t i = 0; i < nsym; i++) {
        const uint32_t n = lens[i];
#pragma unroll
        for (int b = 1; b < 16; b++) count[b] += n == (uint32_t)b ? 1u : 0u;
    }
    uint32_t code = 0;
    next[0] = 0;
#pragma unroll
    for (int b = 1; b < 16; b++) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (uint32_t i = 0; i < nsym; i++) {
        const uint32_t n = lens[i];
        uint32_t c = 0;
#pragma unroll
        for (int b = 1; b < 16; b++)
            if (n == (uint32_t)b) c = next[b]++;
        codes[i] = n ? (uint16_t)(__brev(c) >> (32u - n)) : (uint16_t)0;
    }
}

// len bytes of LDS (from byte 0 of words) to out + dst: aligned words of the destination, bytes at both ends
__device__ __forceinline__ void df_out_of_lds(uint32_t t, const uint32_t *words, uint32_t len, uint8_t *__restrict__ out, uint64_t dst)
{
    const uint8_t *const pb = (const uint8_t *)words;
    uint32_t head = (4u - (uint32_t)(((uint64_t)(uintptr_t)out + dst) & 3ull)) & 3u;
    head = head < len ? head : len;
    const uint32_t nw = (len - head) >> 2;
    if (t < head) out[dst + t] = pb[t];
    uint32_t *const ow = (uint32_t *)(out + (dst + head)); // (a multiple of 4)
    const uint32_t r = 8u * (head & 3u);
    for (uint32_t w = t; w < nw; w += BGZF_THREADS) {
        const uint32_t i = (head >> 2) + w;
        const uint32_t lo = words[i];
        ow[w] = r ? (lo >> r) | (words[i + 1] << (32u - r)) : lo;
    }
    const uint32_t done = head + 4u * nw;
    if (t < len - done) out[dst + done + t] = pb[done + t];
}

// The pointers and sizes that a block needs only where it begins and where it ends are parked in LDS and read back there: as
// kernel arguments they would sit in scalar registers across the whole body, which has none to spare (the first build spilled 76).
__global__ __launch_bounds__(BGZF_THREADS) void k_deflate_block(const uint8_t *data_, uint64_t n_, uint32_t bb, uint64_t blocks, uint32_t *__restrict__ tokens,
                                                               uint8_t *stage_, uint64_t stride_, uint64_t *sizes_, uint32_t grid)
{
    __shared__ DfLds s;
    s.tab[threadIdx.x] = crc_table_entry(threadIdx.x);
    if (threadIdx.x == 0) {
        s.arg[A_DATA] = (uint64_t)(uintptr_t)data_;
        s.arg[A_N] = n_;
        s.arg[A_STAGE] = (uint64_t)(uintptr_t)stage_;
        s.arg[A_STRIDE] = stride_;
        s.arg[A_SIZES] = (uint64_t)(uintptr_t)sizes_;
    }
    __syncthreads();
    uint32_t *const tok = tokens + (uint64_t)blockIdx.x * DF_TOKEN_SLOT;
    const uint8_t *const pb = (const uint8_t *)s.pay;
    for (uint64_t b = blockIdx.x; b < blocks; b += grid) {
        // (the lane number as a value the compiler takes anew for every block: the dozens of lane predicates below are then
        // computed where they are used, not kept in scalar registers across the whole loop, which ran out of them)
        const uint32_t t = df_fresh(threadIdx.x), lane = t & 63u;
        const uint64_t src = b * (uint64_t)bb, n = df_parked(&s.arg[A_N]);
        const uint32_t len = (uint32_t)(n - src < (uint64_t)bb ? n - src : (uint64_t)bb);
        // ---- stage: payload byte i is LDS byte i.  Every aligned word that is read holds at least one byte of the payload.
        {
            const uint64_t addr = df_parked(&s.arg[A_DATA]) + src;
            const uint32_t sh = (uint32_t)(addr & 3ull), r = 8u * sh;
            const uint32_t *const gw = (const uint32_t *)(uintptr_t)(addr - sh);
            const uint32_t in_words = (sh + len + 3u) >> 2, lds_words = (len + 3u) >> 2;
            for (uint32_t w = t; w < lds_words; w += BGZF_THREADS) {
                uint32_t v = gw[w];
                if (r) v = (v >> r) | ((w + 1u < in_words ? gw[w + 1u] : 0u) << (32u - r));
                if (w == lds_words - 1u && (len & 3u)) v &= (1u << (8u * (len & 3u))) - 1u;
                s.pay[w] = v;
            }
            for (uint32_t i = t; i < (1u << DF_HASH_BITS); i += BGZF_THREADS) s.T[i] = 0;
            for (uint32_t i = t; i < DF_LL_ROOM; i += BGZF_THREADS) s.llc[i] = i == 256u ? 1u : 0u;
            if (t < DF_D_ROOM) s.dc[t] = 0;
            if (t < M_WORDS) s.m[t] = 0;
        }
        __syncthreads();
        // the CRC: lane t over its piece, then times x^(8 * the bytes behind the piece)
        {
            const uint32_t c = crc_wave_of_pieces(s.tab, pb, len, t);
            if (lane == 0) atomicXor(&s.m[M_CRC], c);
        }
        // ---- match
        uint32_t start = 0, ntok = 0, n_lit = 0, n_mat = 0, n_mbytes = 0;
        for (uint32_t seg0 = 0; seg0 < len; seg0 += DF_SEG) {
            const uint32_t t1 = df_fresh(t); // (as above: what depends on the lane is computed per segment)
            const uint32_t t = t1, lane = t1 & 63u;
            const uint32_t p = seg0 + t;
            const bool valid = p < len, hashed = valid && p + 4u <= len;
            uint32_t mlen = 0, mdist = 0, h = 0;
            if (hashed) h = (df_ld32(pb + p) * DF_HASH_MUL) >> (32u - DF_HASH_BITS);
            if (valid && p >= start) { // (a position in front of the carry-in start is inside a match)
                const uint32_t cap = len - p < DF_MAX_MATCH ? len - p : DF_MAX_MATCH;
                if (p >= 1u && cap >= DF_MIN_MATCH) {
                    const uint32_t k = df_match_len(pb, p, p - 1u, cap);
                    if (k >= DF_MIN_MATCH) mlen = k, mdist = 1u;
                }
                const uint32_t e = hashed ? s.T[h] : 0u;
                if (e && p - (e - 1u) <= DF_MAX_DIST) {
                    const uint32_t k = df_match_len(pb, p, e - 1u, cap);
                    if (k >= DF_MIN_MATCH && k > mlen) mlen = k, mdist = p - (e - 1u);
                }
            }
            const uint32_t step = mlen ? mlen : 1u;
            s.jump[t] = (uint16_t)(valid && t + step < DF_SEG ? t + step : DF_SEG);
            s.mark[t] = valid && p == start ? 1 : 0;
            if (t == 0) s.jump[DF_SEG] = (uint16_t)DF_SEG, s.mark[DF_SEG] = 0;
            __syncthreads();
            // the positions the greedy parse visits: those at 0, 1, 2, ... steps from the start; after round r the first 2^r are marked
#pragma unroll 1
            for (int round = 0; round < 8; round++) {
                const uint32_t j = s.jump[t], jj = s.jump[j], mk = s.mark[t];
                __syncthreads();
                if (mk) s.mark[j] = 1;
                s.jump[t] = (uint16_t)jj;
                __syncthreads();
            }
            const bool chosen = valid && s.mark[t];
            const uint32_t seg_end = seg0 + DF_SEG < len ? seg0 + DF_SEG : len;
            if (chosen && p + step >= seg_end) s.m[M_CARRY] = p + step; // (the last one visited: one lane)
            const unsigned long long vote = __ballot(chosen);
            if (lane == 0) s.wave[t >> 6] = (uint32_t)__popcll(vote);
            if (chosen) {
                if (mlen) {
                    uint32_t sym, nb, v;
                    df_len_symbol(mlen, sym, nb, v);
                    atomicAdd(&s.llc[sym], 1u);
                    df_dist_symbol(mdist - 1u, sym, nb, v);
                    atomicAdd(&s.dc[sym], 1u);
                    n_mat++, n_mbytes += mlen;
                } else {
                    atomicAdd(&s.llc[pb[p]], 1u);
                    n_lit++;
                }
            }
            if (hashed) atomicMax(&s.T[h], p + 1u);
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t c = s.wave[k];
                if (k < (t >> 6)) before += c;
                total += c;
            }
            if (chosen) {
                const uint32_t at = ntok + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
                tok[at] = mlen ? DF_MATCH | (mlen - 3u) << 16 | (mdist - 1u) : (uint32_t)pb[p];
            }
            ntok += total;
            if (total) start = s.m[M_CARRY];
            __syncthreads(); // (wave, jump and mark are the next segment's)
        }
        if (n_lit) atomicAdd(&s.m[M_LIT], n_lit);
        if (n_mat) atomicAdd(&s.m[M_MAT], n_mat), atomicAdd(&s.m[M_MBYTES], n_mbytes);
        // ---- code
        // three constructions, one after the other: the literal/length code, the distance code, the code-length code
#pragma unroll 1
        for (uint32_t job = 0; job < 3u; job++) {
            if (t == 0 && job == 1u) {
                uint32_t used = 0, which = 0;
                for (uint32_t i = 0; i < DF_D; i++)
                    if (s.dc[i]) used++, which = i;
                s.m[M_DUSED] = used;
                s.m[M_DWHICH] = used == 1u ? which : 0u;
                s.lll[286] = s.lll[287] = 0;
            }
            if (t == 0 && job == 2u) {
                uint32_t hlit = 257u, hdist = 1u;
                for (uint32_t i = 257u; i < DF_LL; i++)
                    if (s.lll[i]) hlit = i + 1u;
                for (uint32_t i = 1u; i < DF_D; i++)
                    if (s.dl[i]) hdist = i + 1u;
                for (uint32_t i = 0; i < DF_CL_ROOM; i++) s.clc[i] = 0;
                for (uint32_t i = 0; i < hlit; i++) s.clc[s.lll[i]]++;
                for (uint32_t i = 0; i < hdist; i++) s.clc[s.dl[i]]++;
                s.m[M_HLIT] = hlit;
                s.m[M_HDIST] = hdist;
            }
            __syncthreads();
            if (job == 1u && s.m[M_DUSED] < 2u) { // no distance in use, or one: symbol 0, or that one, gets one bit
                if (t < DF_D) s.dl[t] = t == s.m[M_DWHICH] ? 1 : 0;
                __syncthreads();
                continue;
            }
            df_huff(t, s, job == 0 ? s.llc : (job == 1u ? s.dc : s.clc), job == 0 ? DF_LL : (job == 1u ? DF_D : DF_CL), job == 2u ? 7u : 15u,
                    job == 0 ? s.lll : (job == 1u ? s.dl : s.cll));
        }
        if (t == 0) {
            uint32_t hclen = 4u;
            for (uint32_t k = 4u; k < DF_CL; k++)
                if (s.cll[DF_CL_ORDER[k]]) hclen = k + 1u;
            uint32_t dyn = 0, fix = 0, head = 3u + 14u + 3u * hclen;
            for (uint32_t i = 0; i < DF_LL; i++) {
                const uint32_t c = s.llc[i], x = df_ll_extra(i);
                dyn += c * ((uint32_t)s.lll[i] + x);
                fix += c * (df_fixed_ll(i) + x);
            }
            for (uint32_t i = 0; i < DF_D; i++) {
                const uint32_t c = s.dc[i], x = df_d_extra(i);
                dyn += c * ((uint32_t)s.dl[i] + x);
                fix += c * (5u + x);
            }
            for (uint32_t i = 0; i < DF_CL; i++) head += s.clc[i] * (uint32_t)s.cll[i];
            const uint32_t cost0 = 40u + 8u * len, cost1 = 3u + fix, cost2 = head + dyn;
            uint32_t btype = 0, bits = cost0;
            if (cost1 < bits) btype = 1u, bits = cost1;
            if (cost2 < bits) btype = 2u, bits = cost2;
            s.m[M_HCLEN] = hclen;
            s.m[M_BTYPE] = btype;
            s.m[M_BITS] = bits;
            s.m[M_HEAD_BITS] = btype == 2u ? head : 3u;
            unsigned long long *const ctl = (unsigned long long *)(uintptr_t)s.arg[A_SIZES] + (blocks + 1); // (behind the sizes)
            atomicAdd(&ctl[DF_STORED + btype], 1ull);
            atomicAdd(&ctl[DF_LITERALS], (unsigned long long)s.m[M_LIT]);
            atomicAdd(&ctl[DF_MATCHES], (unsigned long long)s.m[M_MAT]);
            atomicAdd(&ctl[DF_MATCH_BYTES], (unsigned long long)s.m[M_MBYTES]);
        }
        __syncthreads();
        const uint32_t btype = s.m[M_BTYPE], bits = s.m[M_BITS], crc = ~s.m[M_CRC];
        uint8_t *const slot = (uint8_t *)(uintptr_t)(df_parked(&s.arg[A_STAGE]) + b * df_parked(&s.arg[A_STRIDE])); // this block's bytes
        uint32_t body; // the bytes of the deflate stream
        if (btype == 0) {
            body = len + 5u;
            if (t < 23u) slot[t] = bgzf_head_byte(t, len);
            df_out_of_lds(t, s.pay, len, slot, 23u);
        } else {
            body = (bits + 7u) >> 3;
            if (btype == 1u) {
                for (uint32_t i = t; i < DF_LL_ROOM; i += BGZF_THREADS) s.lll[i] = (uint8_t)df_fixed_ll(i);
                if (t < DF_D) s.dl[t] = 5;
            }
            for (uint32_t w = t; w < (bits >> 5) + 4u; w += BGZF_THREADS) s.pay[w] = 0; // (bits < 40 + 8 * 65505: inside pay)
            __syncthreads();
            if ((t & 63u) == 0 && t < 192u) { // a lane of three waves each: the codes of one table
                const uint32_t k = t >> 6;
                df_canonical(k == 0 ? s.lll : (k == 1u ? s.dl : s.cll), k == 0 ? DF_LL_ROOM : (k == 1u ? DF_D : DF_CL),
                             k == 0 ? s.llcode : (k == 1u ? s.dcode : s.clcode));
            }
            __syncthreads();
            if (t == 0) {
                uint32_t at = 0;
                df_or_bits(s.pay, at, 1u | btype << 1, 3u), at += 3u;
                if (btype == 2u) {
                    const uint32_t hlit = s.m[M_HLIT], hdist = s.m[M_HDIST], hclen = s.m[M_HCLEN];
                    df_or_bits(s.pay, at, (hlit - 257u) | (hdist - 1u) << 5 | (hclen - 4u) << 10, 14u), at += 14u;
                    for (uint32_t k = 0; k < hclen; k++) df_or_bits(s.pay, at, s.cll[DF_CL_ORDER[k]], 3u), at += 3u;
                    for (uint32_t i = 0; i < hlit + hdist; i++) {
                        const uint32_t l = i < hlit ? s.lll[i] : s.dl[i - hlit];
                        df_or_bits(s.pay, at, s.clcode[l], s.cll[l]), at += s.cll[l];
                    }
                }
            }
            uint32_t at = s.m[M_HEAD_BITS];
            for (uint32_t c0 = 0; c0 < ntok; c0 += BGZF_THREADS) {
                const uint32_t t1 = df_fresh(t);
                const uint32_t t = t1;
                uint64_t v = 0;
                uint32_t nb = 0;
                if (c0 + t < ntok) {
                    const uint32_t k = tok[c0 + t];
                    if (k & DF_MATCH) {
                        uint32_t sym, xb, xv;
                        df_len_symbol(((k >> 16) & 0xFFu) + 3u, sym, xb, xv);
                        v = s.llcode[sym], nb = s.lll[sym];
                        v |= (uint64_t)xv << nb, nb += xb;
                        df_dist_symbol(k & 0xFFFFu, sym, xb, xv);
                        v |= (uint64_t)s.dcode[sym] << nb, nb += s.dl[sym];
                        v |= (uint64_t)xv << nb, nb += xb;
                    } else {
                        v = s.llcode[k], nb = s.lll[k];
                    }
                }
                uint32_t total;
                const uint32_t before = df_scan(t, nb, s.wave, total);
                df_or_bits(s.pay, at + before, v, nb);
                at += total;
            }
            if (t == 0) df_or_bits(s.pay, at, s.llcode[256], s.lll[256]); // end of block
            __syncthreads();
            if (t < 18u) slot[t] = bgzf_head_byte(t, body - 5u); // (BSIZE: the bytes of the block - 1 = body + 25)
            df_out_of_lds(t, s.pay, body, slot, 18u);
        }
        if (t < 8u) {
            const uint32_t v = t < 4u ? crc : len;
            slot[18u + body + t] = (uint8_t)(v >> (8u * (t & 3u)));
        }
        if (t == 0) ((uint64_t *)(uintptr_t)s.arg[A_SIZES])[b] = 26ull + body;
        __syncthreads(); // (the LDS is the next block's)
    }
}

// The blocks from their slots to where the scan puts them (offs: blocks + 1, from 0), a workgroup per block; block_index; the
// end-of-file block by workgroup 0.  A slot starts at a multiple of 16 and has 16 spare bytes behind the largest block.
__global__ __launch_bounds__(BGZF_THREADS) void k_deflate_pack(const uint8_t *__restrict__ stage, uint64_t stride, const uint64_t *__restrict__ offs,
                                                              uint64_t blocks, int eof, uint8_t *__restrict__ out, uint64_t *__restrict__ block_index)
{
    const uint32_t t = threadIdx.x;
    if (blockIdx.x == 0) {
        const uint64_t end = offs[blocks];
        if (eof && t < KISS_HIP_BGZF_EOF_BYTES) out[end + t] = bgzf_eof_byte(t);
        if (block_index && t == 0) block_index[blocks] = end;
    }
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t dst = offs[b];
        const uint32_t len = (uint32_t)(offs[b + 1] - dst);
        if (block_index && t == 0) block_index[b] = dst;
        const uint8_t *const sb = stage + b * stride;
        const uint32_t *const sw = (const uint32_t *)sb; // (a multiple of 16)
        uint32_t head = (4u - (uint32_t)(((uint64_t)(uintptr_t)out + dst) & 3ull)) & 3u;
        head = head < len ? head : len;
        const uint32_t nw = (len - head) >> 2;
        if (t < head) out[dst + t] = sb[t];
        uint32_t *const ow = (uint32_t *)(out + (dst + head)); // (a multiple of 4)
        const uint32_t r = 8u * (head & 3u);
        for (uint32_t w = t; w < nw; w += BGZF_THREADS) {
            const uint32_t lo = sw[w];
            ow[w] = r ? (lo >> r) | (sw[w + 1u] << (32u - r)) : lo;
        }
        const uint32_t done = head + 4u * nw;
        if (t < len - done) out[dst + done + t] = sb[done + t];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct DeflatePlan {
    uint32_t bb;
    uint64_t blocks, bound;
};
int deflate_plan(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, const uint8_t *out, uint64_t out_capacity,
                 const uint64_t *block_index, uint64_t index_capacity, DeflatePlan &p, kiss_hip_bgzf_deflate_report &rep)
{
    p.bb = block_bytes ? block_bytes : KISS_HIP_BGZF_BLOCK_DEFAULT;
    if (p.bb > KISS_HIP_BGZF_BLOCK_MAX) return KISS_HIP_E_INVALID;
    if ((n && !data) || (out_capacity && !out)) return KISS_HIP_E_INVALID;
    if (n > (1ull << 62)) return KISS_HIP_E_UNSUPPORTED;
    p.blocks = div_up(n, (uint64_t)p.bb);
    p.bound = n + (uint64_t)KISS_HIP_BGZF_OVERHEAD * p.blocks + (eof ? KISS_HIP_BGZF_EOF_BYTES : 0u);
    rep.blocks = p.blocks;
    rep.out_bytes = p.bound;
    if (out_capacity < p.bound || (block_index && index_capacity < p.blocks + 1)) return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

int deflate_steps(kiss_hip_ctx *ctx, const uint8_t *data, uint64_t n, int eof, uint8_t *out, uint64_t *block_index, const DeflatePlan &p,
                  kiss_hip_bgzf_deflate_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t blocks = p.blocks;
    if ((blocks + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    if (ctx->cu_count <= 0) {
        KCHECK(hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (ctx->cu_count <= 0) ctx->cu_count = 1;
    }
    const uint64_t resident = blocks < (uint64_t)ctx->cu_count ? blocks : (uint64_t)ctx->cu_count; // (256 KiB of tokens each)
    const uint64_t stride = (((uint64_t)p.bb + KISS_HIP_BGZF_OVERHEAD + 15u) & ~15ull) + 16u;
    DevBuf tokens, stage, sizes;
    KTRY(tokens.take(ctx, FM_SLOT_DEFLATE_TOKENS, resident * DF_TOKEN_SLOT * 4));
    KTRY(stage.take(ctx, FM_SLOT_DEFLATE_STAGE, blocks * stride));
    KTRY(sizes.take(ctx, FM_SLOT_DEFLATE_SIZES, (blocks + 1 + DF_CTL_WORDS) * 8));
    uint64_t *const offs = (uint64_t *)sizes.p; // (scanned in place); behind them the counters of the call
    ev.mark(0);
    KTRY(kiss_zero_u32(ctx, offs + blocks, 2 * (1 + DF_CTL_WORDS)));
    if (blocks) {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_deflate_block, dim3((unsigned)resident), dim3(BGZF_THREADS), 0, ctx->stream, data, n, p.bb, blocks, (uint32_t *)tokens.p,
                           (uint8_t *)stage.p, stride, offs, (uint32_t)resident);
        KCHECK(hipGetLastError());
    }
    ev.mark(1);
    KTRY(kiss_scan_u64(ctx, offs, offs, blocks + 1));
    ev.mark(2);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        const uint64_t want = blocks ? blocks : 1;
        hipLaunchKernelGGL(k_deflate_pack, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(BGZF_THREADS), 0, ctx->stream, (const uint8_t *)stage.p,
                           stride, (const uint64_t *)offs, blocks, eof, out, block_index);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    uint64_t h[1 + DF_CTL_WORDS] = {0}; // the end of the last block, the counters
    KCHECK(hipMemcpyAsync(h, offs + blocks, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.out_bytes = h[0] + (eof ? KISS_HIP_BGZF_EOF_BYTES : 0u);
    rep.stored_blocks = h[1 + DF_STORED];
    rep.fixed_blocks = h[1 + DF_FIXED];
    rep.dynamic_blocks = h[1 + DF_DYNAMIC];
    rep.literals = h[1 + DF_LITERALS];
    rep.matches = h[1 + DF_MATCHES];
    rep.match_bytes = h[1 + DF_MATCH_BYTES];
    rep.ms_block = ev.ms(0, 1);
    rep.ms_scan = ev.ms(1, 2);
    rep.ms_copy = ev.ms(2, 3);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_bgzf_deflate_dev(kiss_hip_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out,
                              uint64_t out_capacity, uint64_t *block_index, uint64_t index_capacity, kiss_hip_bgzf_deflate_report *report,
                              void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx);
    kiss_hip_bgzf_deflate_report rep{};
    if (report) *report = rep;
    DeflatePlan p;
    const int planned = deflate_plan(data, n, block_bytes, eof, out, out_capacity, block_index, index_capacity, p, rep);
    if (report) *report = rep; // (the bound: the caller's second call)
    KTRY(planned);
    if (!ctx) return KISS_HIP_E_INVALID;
    if (!p.bound && !block_index) return KISS_HIP_OK;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    int rc = deflate_steps(ctx, data, n, eof, out, block_index, p, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_bgzf_deflate_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                               uint64_t *block_index, uint64_t index_capacity, kiss_hip_bgzf_deflate_report *report, int device)
{
    kiss_hip_bgzf_deflate_report rep{};
    if (report) *report = rep;
    DeflatePlan p;
    const int planned = deflate_plan(data, n, block_bytes, eof, out, out_capacity, block_index, index_capacity, p, rep);
    if (report) *report = rep;
    KTRY(planned);
    if (!n) { // nothing to compress: no device
        static const uint8_t eof_block[KISS_HIP_BGZF_EOF_BYTES] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0};
        for (uint32_t k = 0; eof && k < KISS_HIP_BGZF_EOF_BYTES; k++) out[k] = eof_block[k];
        if (block_index) block_index[0] = 0;
        return KISS_HIP_OK;
    }
    return kiss_one_shot_cached(device, fm_host_max_n(0, p.blocks + 1), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *d = st.up(data, n);
        uint8_t *o = st.room<uint8_t>(true, p.bound);
        uint64_t *bi = st.room<uint64_t>(block_index != nullptr, (p.blocks + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_bgzf_deflate_report r{};
        const int rc = kiss_hip_bgzf_deflate_dev(ctx, d, n, block_bytes, eof, o, p.bound, bi, p.blocks + 1, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(out, o, r.out_bytes);
        if (block_index) st.down(block_index, bi, (p.blocks + 1) * 8);
        return st.rc;
    });
}

} // extern "C"
