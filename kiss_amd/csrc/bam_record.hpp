// bam_record.hpp -- what the kernels that read unframed BAM records through their CSR share (bam_sort.hip, bai.hip): loads that the
// compiler may not reorder into wider ones, a 64-bit value across the lanes, the four bytes at any byte address read from the
// naturally aligned words that hold them, and THE check of a record's head -- the BAD kinds of include/kiss_hip_bam_sort.h, in
// one place for the sort and for everything that reads sorted records after it.
#pragma once
#include "fm_internal.hpp"
#include "../../include/kiss_hip_bam_sort.h"

__device__ __forceinline__ uint32_t bs_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t bs_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// v of lane `from`, as two unsigned halves (fm_sam_line.hpp has the pitfall this avoids)
__device__ __forceinline__ uint64_t bs_lane64(uint64_t v, int from)
{
    const uint32_t lo = (uint32_t)__shfl((unsigned int)(v & 0xFFFFFFFFull), from, 64);
    const uint32_t hi = (uint32_t)__shfl((unsigned int)(v >> 32), from, 64);
    return (uint64_t)hi << 32 | (uint64_t)lo;
}
// the four bytes at base + off (any byte offset, any base) from the aligned words that hold them: one word, or two funnelled
__device__ __forceinline__ uint32_t bs_word_at(const uint8_t *__restrict__ base, uint64_t off)
{
    const uintptr_t a = (uintptr_t)(base + off);
    const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3u) * 8u;
    const uint32_t lo = bs_ld32(w);
    const uint32_t hi = sh ? bs_ld32(w + 1) : 0u; // (an aligned word is never read unless one of its bytes is wanted)
    return __funnelshift_r(lo, hi, sh);
}

// The head of record r < records, checked: bad by any BAD kind of kiss_hip_bam_sort.h.  read: its bytes lie inside bam and are 36 or
// more, so that the fixed part may be read (only then are at, size, ref and pos set, and only then may a caller read further).
struct BsHead {
    bool bad, read;
    uint64_t at, size;
    int32_t ref, pos;
};
__device__ __forceinline__ BsHead bs_head(const uint8_t *__restrict__ bam, uint64_t bam_bytes, const uint64_t *__restrict__ rec_index, uint64_t records,
                                          uint32_t n_ref, uint64_t r)
{
    BsHead h{false, false, 0, 0, -1, -1};
    const uint64_t a = bs_ld64(rec_index + r), b = bs_ld64(rec_index + r + 1);
    if (r == 0 && a != 0) h.bad = true;
    if (r == records - 1 && b != bam_bytes) h.bad = true;
    if (b <= a || b > bam_bytes) h.bad = true;
    else if (b - a < KISS_HIP_BAM_RECORD_MIN) h.bad = true;
    if (b > a && b <= bam_bytes && b - a >= KISS_HIP_BAM_RECORD_MIN) { // (only then are the twelve bytes there to be read)
        h.read = true;
        h.at = a;
        h.size = b - a;
        const int32_t block_size = (int32_t)bs_word_at(bam, a);
        h.ref = (int32_t)bs_word_at(bam, a + 4);
        h.pos = (int32_t)bs_word_at(bam, a + 8);
        if (block_size < 0 || (uint64_t)block_size != h.size - 4) h.bad = true;
        if (h.ref < -1 || (int64_t)h.ref >= (int64_t)n_ref) h.bad = true;
        if (h.pos < -1) h.bad = true;
    }
    return h;
}
