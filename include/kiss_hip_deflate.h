/* kiss_hip_deflate.h -- BGZF blocks compressed on the device: kiss_hip_bgzf_deflate_* frames any bytes as kiss_hip_bgzf_* does
 * (kiss_hip_bam.h, which this header includes: the block sizes, the end-of-file block, the status codes, the ctx and the two
 * promises of a device entry), with the payload of every block coded as DEFLATE (RFC 1951).  kiss_amd/csrc/bgzf_deflate.hip;
 * DESIGN.md 4.23; the definition restated as plain loops in tests/deflate_model.py.
 *
 * THE BLOCK.  data[0, n) is cut into payloads of block_bytes (0 means 65280; allowed 1 .. 65505, anything else is
 * KISS_HIP_E_INVALID); the last one may be shorter.  A block is the 18 bytes of the BGZF header (BSIZE = the bytes of the block
 * - 1), ONE deflate block with BFINAL = 1, the CRC-32 of the payload and ISIZE.  The encoder computes, exactly in bits, what the
 * token sequence of the payload takes stored (BTYPE 00: 40 + 8 L bits), with the fixed codes (01) and with dynamic codes (10), and
 * writes the smallest; a tie goes to the lower BTYPE.  So a block never takes more than L + 31 bytes, and a block coded as
 * stored is byte for byte the block kiss_hip_bgzf_dev writes.  The output is a pure function of (data, n, block_bytes, eof).
 *
 * THE TOKENS of a payload P[0, L):
 *   candidates: the positions are cut into segments of 256.  h(p) = (the four bytes at p as a little-endian u32 * 0x9E3779B1
 *     modulo 2^32) >> 19, defined for p + 4 <= L.  T[h] is the LARGEST position of an EARLIER segment with that hash.  Position p
 *     has at most two candidates: T[h(p)] when it exists and p - T[h(p)] <= 32768, and p - 1.  (After a segment's lookups all its
 *     positions enter T with a maximum: the order inside the segment cannot matter.)
 *   match: len(p, q) = the common prefix of P[p ..] and P[q ..], at most min(258, L - p).  A match needs len >= 4.  The longer
 *     candidate wins, a tie goes to the smaller distance.  A match may overlap itself (distance 1 is a run).
 *   parse: greedy from p = 0: a position with a match emits (len, dist) and moves on by len, any other a literal and moves on by
 *     1.  No lazy evaluation.
 * THE CODES.  The literal/length symbols (286; end-of-block counted once) and the distance symbols (30) get their code lengths
 * from their counts: the symbols with a non-zero count sorted by (count, symbol); the two-queue merge, which takes the leaf when
 * leaf <= internal; the lengths are the depths.  If a length exceeds the limit (15; 7 for the code-length code) every non-zero
 * count becomes (c + 1) >> 1 and the construction runs again.  Codes are canonical (RFC 1951 3.2.2).  With no distance symbol in
 * use, or one, distance symbol 0 (or that one) gets length 1.  The dynamic header: HLIT and HDIST trimmed of trailing zeros (at
 * least 257 and 1); the lengths sent with the code-length symbols 0 .. 15 only (never 16 .. 18); HCLEN trimmed in the order of RFC
 * 1951 (at least 4).  Huffman codes are packed from their most significant bit, extra bits and header fields from their least;
 * the stream is zero-padded to a byte.
 *
 * THE CALL.  out[0, out_bytes) holds the blocks PACKED one after the other, the end-of-file block (28 bytes) behind them when
 * eof != 0.  out_capacity must be at least the worst case n + 31 * blocks + 28 * (eof != 0), blocks = ceil(n / block_bytes);
 * below it the call returns KISS_HIP_E_INVALID, the report holds blocks and THAT BOUND in out_bytes, and nothing is written.
 * Bytes of out behind out_bytes are not written either.  block_index is optional: blocks + 1 u64, a CSR over out from 0;
 * block_index[blocks] = out_bytes less the end-of-file block.  index_capacity < blocks + 1 with block_index not NULL:
 * KISS_HIP_E_INVALID, nothing written.  Other KISS_HIP_E_INVALID: ctx NULL, data NULL with n > 0, out NULL with out_capacity > 0.
 * n = 0 writes no block, only the end-of-file block when asked, and needs no device.  data and out may lie at any address and
 * must not overlap.  Scratch (the token lists of the resident workgroups, the blocks before they are packed, their sizes) lives in
 * named slots of the ctx: no allocation after the first call of a size.  KISS_HIP_E_UNSUPPORTED: more blocks than the ctx can scan.
 * Report: blocks, out_bytes, how many blocks were coded stored / fixed / dynamic, and the parse of all payloads (literals, matches,
 * match_bytes: literals + match_bytes = n) whichever coding was written; the times of the three passes.
 * KNOWN PROPERTY: one workgroup of 256 lanes per block, one block resident per CU (the payload, the hash table and the code tables
 * take 106 KiB of LDS).  Scratch kept in the ctx after a call: 256 KiB of tokens per resident workgroup -- min(blocks, the
 * compute units of the device), 64 MiB at most on a device of 256 -- plus the blocks before they are packed (about the worst-case
 * output) and 8 bytes per block.  The kernels count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_DEFLATE_H
#define KISS_HIP_DEFLATE_H

#include "kiss_hip_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kiss_hip_bgzf_deflate_report {
    uint64_t blocks, out_bytes, stored_blocks, fixed_blocks, dynamic_blocks, literals, matches, match_bytes;
    /* block: the kernel that matches, codes and packs a block; scan: the sizes of the blocks; copy: the blocks packed into out */
    float ms_total, ms_block, ms_scan, ms_copy;
} kiss_hip_bgzf_deflate_report;

/* report is a host pointer; data, out and block_index are device pointers */
int kiss_hip_bgzf_deflate_dev(kiss_hip_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out,
                              uint64_t out_capacity, uint64_t *block_index, uint64_t index_capacity, kiss_hip_bgzf_deflate_report *report,
                              void *stream);
/* the same with host pointers */
int kiss_hip_bgzf_deflate_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                               uint64_t *block_index, uint64_t index_capacity, kiss_hip_bgzf_deflate_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
