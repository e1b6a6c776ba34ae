// bgzf_block.hpp -- what the two units that write BGZF blocks share (fm_bam.hip: stored blocks; bgzf_deflate.hip: compressed
// ones): the CRC-32 of a payload in LDS, in pieces that are combined, and the fixed bytes of a block.  Included inside the unit's
// anonymous namespace.
#pragma once

constexpr int BGZF_THREADS = 256;
constexpr uint32_t BGZF_PAY_WORDS = 16384; // 65505 payload bytes and 3 of phase, rounded up
constexpr uint32_t CRC_POLY = 0xEDB88320u;

// a * b modulo the CRC-32 polynomial, reflected: bit 31 is x^0
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}
// x^(8 * 2^j) modulo the polynomial, j = 0 .. 15
struct CrcPowers {
    uint32_t x[16];
    constexpr CrcPowers() : x{}
    {
        uint32_t v = 0x40000000u; // x^1
        for (int k = 0; k < 3; k++) v = crc_mul(v, v);
        for (int j = 0; j < 16; j++) {
            x[j] = v;
            v = crc_mul(v, v);
        }
    }
};
// x^(8 m) modulo the polynomial, m < 2^16
__device__ __forceinline__ uint32_t crc_x8n(uint32_t m)
{
    constexpr CrcPowers P;
    uint32_t p = 0x80000000u; // x^0
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (m >> j & 1u) p = crc_mul(p, P.x[j]);
    return p;
}

// the fixed bytes of a block in front of its payload (18 of BGZF, 5 of the stored deflate block); total = the bytes of the block
__device__ __forceinline__ uint8_t bgzf_head_byte(uint32_t k, uint32_t len)
{
    const uint32_t bsize = len + KISS_HIP_BGZF_OVERHEAD - 1u;
    switch (k) {
    case 0: return 0x1f;
    case 1: return 0x8b;
    case 2: return 8;
    case 3: return 4;
    case 9: return 0xff;
    case 10: return 6;
    case 12: return 'B';
    case 13: return 'C';
    case 14: return 2;
    case 16: return (uint8_t)bsize;
    case 17: return (uint8_t)(bsize >> 8);
    case 18: return 1;
    case 19: return (uint8_t)len;
    case 20: return (uint8_t)(len >> 8);
    case 21: return (uint8_t)~len;
    case 22: return (uint8_t)(~len >> 8);
    default: return 0;
    }
}
__device__ __forceinline__ uint8_t bgzf_eof_byte(uint32_t k)
{
    if (k < 16) return bgzf_head_byte(k, 0);
    return k == 16 ? 0x1b : (k == 18 ? 0x03 : 0);
}

// the table of the byte-wise CRC: entry t by lane t of 256
__device__ __forceinline__ uint32_t crc_table_entry(uint32_t t)
{
    uint32_t c = t;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    return c;
}

// The CRC-32 of the len bytes at pb (LDS) by the 256 lanes of a workgroup, tab the table above in LDS: lane t runs the table CRC
// over its piece [t * piece, (t + 1) * piece), piece = ceil(len / 256), from 0 (lane 0 from 0xFFFFFFFF), and multiplies its register
// by x^(8 * the bytes behind the piece).  -> the XOR of the products over the lane's WAVE, in every lane of it; the caller XORs
// the four waves together (lane 0 of each into a word of LDS) and complements.
__device__ __forceinline__ uint32_t crc_wave_of_pieces(const uint32_t *tab, const uint8_t *pb, uint32_t len, uint32_t t)
{
    const uint32_t piece = (len + BGZF_THREADS - 1u) / BGZF_THREADS;
    const uint32_t beg = t * piece < len ? t * piece : len;
    const uint32_t end = beg + piece < len ? beg + piece : len;
    uint32_t c = t == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t k = beg; k < end; k++) c = tab[(c ^ pb[k]) & 0xFFu] ^ (c >> 8);
    if (end > beg && end < len) c = crc_mul(c, crc_x8n(len - end));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c ^= (uint32_t)__shfl_xor((unsigned int)c, o, 64);
    return c;
}
