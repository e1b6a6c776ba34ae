// The packed class counting of the induction's count pass (kiss_amd/csrc/induce_count.hpp) against its definition byte by
// byte.  A host program: the header is plain C++ here, and the kernel compiles the same lines.  Built and run by
// tests/test_induce_count_packed.py (with AddressSanitizer and UBSan); prints "ok <cases>" and exits 0, or says what differs.
#include "kiss_amd/csrc/induce_count.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

// the definition: a class byte counts for class (b & 3) when it has bases left (bit 2 clear), lies inside the stretch
// (bit 3 clear) and the pass emits that class; -> 8-bit count per class, class c in bits 8c+7 : 8c
static uint32_t by_bytes(const uint32_t *w, int nwords, uint32_t emitmask)
{
    uint32_t n[4] = {0, 0, 0, 0};
    for (int i = 0; i < nwords; i++)
        for (int e = 0; e < 4; e++) {
            const uint32_t b = (w[i] >> (8 * e)) & 0xFFu;
            const uint32_t cls = b & 3u;
            if ((b & 4u) == 0u && (b & 8u) == 0u && ((emitmask >> cls) & 1u)) n[cls]++;
        }
    for (int c = 0; c < 4; c++)
        if (n[c] > 255u) {
            std::printf("the definition itself overflows a field: class %d has %u\n", c, n[c]);
            std::exit(2);
        }
    return n[0] | (n[1] << 8) | (n[2] << 16) | (n[3] << 24);
}

static unsigned long cases = 0;

static void hold(const uint32_t *w, int nwords, uint32_t emitmask, const char *what)
{
    const uint32_t got = kiss_cls_count_packed(w, nwords, emitmask), want = by_bytes(w, nwords, emitmask);
    cases++;
    if (got != want) {
        std::printf("%s: %d words, first %08x, emit mask %x: packed %08x, byte by byte %08x\n", what, nwords, w[0], emitmask, got, want);
        std::exit(1);
    }
}

int main()
{
    // every byte value 0 .. 15 in each of the four byte positions, all at once: 16^4 words, each under all 16 emit masks
    for (uint32_t v = 0; v < 65536u; v++) {
        const uint32_t w = (v & 15u) | (((v >> 4) & 15u) << 8) | (((v >> 8) & 15u) << 16) | (((v >> 12) & 15u) << 24);
        for (uint32_t emit = 0; emit < 16u; emit++) hold(&w, 1, emit, "one word");
    }
    // a lane's nine words (induce.hip: two 16-byte pieces and one word of the 129th): all four bytes of all nine words
    // the same value, so every field of a class stands at 9 and its total at 36 -- a field that ran into its neighbour,
    // or a total past eight bits, shows; then the same for the largest number of words the header allows
    for (int nwords : {9, KISS_CNT_MAX_WORDS}) {
        for (uint32_t b = 0; b < 16u; b++) {
            const std::vector<uint32_t> w((size_t)nwords, b * 0x01010101u);
            for (uint32_t emit = 0; emit < 16u; emit++) hold(w.data(), nwords, emit, "equal words");
        }
        // ... and with the four classes in the four positions, in every rotation (each class's count is in one field only)
        for (int r = 0; r < 4; r++) {
            uint32_t word = 0;
            for (int e = 0; e < 4; e++) word |= (uint32_t)((e + r) & 3) << (8 * e);
            const std::vector<uint32_t> w((size_t)nwords, word);
            for (uint32_t emit = 0; emit < 16u; emit++) hold(w.data(), nwords, emit, "rotated classes");
        }
    }
    // nine words of mixed bytes from a small generator, every emit mask
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int t = 0; t < 20000; t++) {
        uint32_t w[9];
        for (int i = 0; i < 9; i++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            w[i] = (uint32_t)(s >> 32) & 0x0F0F0F0Fu;
        }
        for (int nwords = 0; nwords <= 9; nwords++) hold(w, nwords, (uint32_t)t & 15u, "mixed words");
    }
    std::printf("ok %lu\n", cases);
    return 0;
}
