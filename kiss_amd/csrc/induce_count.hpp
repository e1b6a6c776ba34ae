// induce_count.hpp -- the class counts of the induction's count pass over class bytes, four bytes to a 32-bit word.
//
// A class byte (induce.hip: cls_byte) holds the class in bits 1:0, "no bases left" in bit 2 and, where the count pass
// put it in place of a byte outside its stretch, "skip" in bit 3.  An item counts for its class when bits 2 and 3 are
// clear; an item with bit 2 set is not counted here (the count pass refreshes its word and counts it then).
//
// Plain C++ on both sides: k_induce_count (induce.hip) and the host program of tests/test_induce_count_packed.py
// compile the same lines.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KISS_CNT_HD __host__ __device__ __forceinline__
#else
#define KISS_CNT_HD inline
#endif

constexpr int KISS_CNT_MAX_WORDS = 63; // (four byte fields per class: 4 x 63 = 252 still fits the 8-bit total of a class)

// per class one word of four byte fields, field e = how many of the words added so far hold that class in byte e
struct KissClsAcc {
    uint32_t a[4];
};

KISS_CNT_HD void kiss_cls_acc_add(KissClsAcc &acc, uint32_t w)
{
    const uint32_t ones = 0x01010101u;
    const uint32_t lo = w, hi = w >> 1;
    const uint32_t live = ~(w >> 2) & ~(w >> 3) & ones; // neither "no bases left" nor "skip"
    acc.a[0] += live & ~lo & ~hi;
    acc.a[1] += live & lo & ~hi;
    acc.a[2] += live & ~lo & hi;
    acc.a[3] += live & lo & hi;
}

// the four byte fields of every class summed: class c in bits 8c+7 : 8c (no emit mask applied)
KISS_CNT_HD uint32_t kiss_cls_acc_sum(const KissClsAcc &acc)
{
    const uint32_t ones = 0x01010101u;
    return ((acc.a[0] * ones) >> 24) | (((acc.a[1] * ones) >> 24) << 8) | (((acc.a[2] * ones) >> 24) << 16) |
           ((acc.a[3] * ones) & 0xFF000000u);
}

// 8-bit class counts with the classes that the pass does not emit set to zero: bit c of emitmask = class c is emitted
KISS_CNT_HD uint32_t kiss_cls_emit(uint32_t cnt8, uint32_t emitmask)
{
    const uint32_t keep = ((emitmask & 1u) ? 0x000000FFu : 0u) | ((emitmask & 2u) ? 0x0000FF00u : 0u) |
                          ((emitmask & 4u) ? 0x00FF0000u : 0u) | ((emitmask & 8u) ? 0xFF000000u : 0u);
    return cnt8 & keep;
}

// items per emitted class among the 4 * nwords class bytes of w[0 .. nwords), nwords <= KISS_CNT_MAX_WORDS
KISS_CNT_HD uint32_t kiss_cls_count_packed(const uint32_t *w, int nwords, uint32_t emitmask)
{
    KissClsAcc acc = {{0u, 0u, 0u, 0u}};
    for (int i = 0; i < nwords; i++) kiss_cls_acc_add(acc, w[i]);
    return kiss_cls_emit(kiss_cls_acc_sum(acc), emitmask);
}
