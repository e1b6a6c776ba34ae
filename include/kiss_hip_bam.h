/* kiss_hip_bam.h -- the BAM output written on the device: the alignment records of a batch (kiss_hip_fmi_bam_*) and the BGZF
 * framing of any bytes, with the CRC-32 of every block computed on the device (kiss_hip_bgzf_*).  kiss_amd/csrc/fm_bam.hip;
 * DESIGN.md 4.22; the definition restated in tests/bam_model.py.  Declared beside kiss_hip_sam.h, which it includes: the input
 * struct, the status codes, the ctx and the two promises of a device entry (stream, alignment) are the ones written there.
 *
 * 1. THE RECORDS.
 * Input: kiss_hip_sam_input exactly as kiss_hip_fmi_sam_* takes it.  WHICH records a read has, in which order, and their FLAG,
 * MAPQ, place (RNAME, POS), RNEXT / PNEXT, TLEN and tags are the rules of kiss_hip_sam.h: one SAM line is one BAM record, and
 * the device code describes a line once for both writers (kiss_amd/csrc/fm_sam_line.hpp).
 * A record is little-endian and packed (L the bases of the read, k the alignment of a hit record):
 *   block_size i32: the bytes of the record that follow this field;
 *   refID i32, pos i32: the hit's ref and POS - 1; an unmapped record: those of its place, without a place -1 and -1;
 *   l_read_name u8: name_len + 1;  mapq u8: MAPQ modulo 256;
 *   bin u16: reg2bin(pos, pos + max(1, reflen)) of the SAM specification, computed with signed 64-bit shifts and reduced to its
 *     low 16 bits; reflen = the sum of the lengths of the M and D ops; an unmapped record uses reg2bin(pos, pos + 1), which is
 *     4680 for pos = -1;
 *   n_cigar_op u16;  flag u16: FLAG;  l_seq u32: L;
 *   next_refID i32, next_pos i32: the record INDEX of the place (two records of one name are two indices; SAM's '=' is not
 *     looked at) and PNEXT - 1; without a place -1 and -1;
 *   tlen i32: the low 32 bits of the signed TLEN;
 *   read_name: the name bytes and a NUL;
 *   cigar, u32 each: [k.rbeg << 4 | 4] the ops as they stand (len << 4 | op; M 0, I 1, D 2) [(L - k.rend) << 4 | 4], a clip only
 *     when its length is not 0; an unmapped record has none;
 *   seq, (L + 1) / 2 bytes: two bases per byte, the first in the high nibble; code 0..3 is 1, 2, 4, 8 (A, C, G, T), anything
 *     above 3 is 15; a reverse hit stores the reverse complement; an odd L leaves the last low nibble 0;
 *   qual, L bytes: (qual[i] - 33) modulo 256, reversed for a reverse hit; with qual NULL every byte is 0xFF;
 *   tags of a hit record, in SAM's order and with fixed types, so that the size of a record does not depend on its values:
 *     NM I (u32); MD Z with a NUL (only with md); AS I; XS I (not on SECONDARY hits); YS I, YT Z "CP", YR C 1 where the SAM line
 *     has them.  An unmapped record has no tags.
 * R = 0 is KISS_HIP_E_INVALID: a BAM record names its reference by index.
 * A read is BAD iff it is BAD for the SAM call, or
 *   its name has 0 bytes or more than 254, or L >= 2^28;
 *   a hit of it that exists (aln < C, ref < R, tbeg >= bounds[ref]) has POS - 1 >= 2^31; or its pair chooses for the PARTNER a
 *     hit o != NONE with o < H that exists in this sense and has POS - 1 >= 2^31 (that is this read's PNEXT - 1);
 *   a RECORD of it has more than 65535 cigar entries with its clips, an op code above 2, or a block_size of 2^31 or more.
 * With a BAD read the call returns KISS_HIP_E_INVALID, the report holds bad (how many reads) and first_bad, and NOTHING is
 * written to bam, rec_index or read_rec.  The last group is only looked for in a batch that has no BAD read of the other groups:
 * bad and first_bad then count that group alone.
 * Output: bam -- the records one after the other, no BGZF and no file header; rec_index -- optional, records + 1 u64, CSR over the
 * records, from 0; read_rec -- Q + 1 u64, the first record of every read, read_rec[Q] = records.
 * Report: records, bam_bytes, unmapped_records, longest (the longest record with its block_size field), bad, first_bad, the times.
 * SIZE, THEN FILL; the NULL-pointer rules; zero reads (KISS_HIP_OK, read_rec[0] = 0 and rec_index[0] = 0); the limits and the
 * alignment promises are those of kiss_hip_fmi_sam_*, with bam for sam, rec_index for line_index, read_rec for read_line.  bam
 * may lie at any address.
 * KNOWN PROPERTY: one wave writes one record; the nine words of the fixed part and the tags are written by one lane each, the
 * name, the ops, SEQ, QUAL and MD by the lanes together.
 *
 * 2. THE FRAMING.
 * kiss_hip_bgzf_dev cuts data[0, n) into payloads of block_bytes (0 means 65280; allowed 1 .. 65505, anything else is
 * KISS_HIP_E_INVALID); the last payload may be shorter.  Block b is written at out + b * (block_bytes + 31):
 *   1f 8b 08 04, MTIME 0 (4 bytes), XFL 0, OS ff, XLEN 6 (u16), 'B' 'C', SLEN 2 (u16), BSIZE u16 = the bytes of the block - 1;
 *   the header of a stored deflate block: 01, LEN u16, ~LEN u16 (LEN = the payload's bytes);
 *   the payload;
 *   CRC-32 of the payload u32 (IEEE 802.3, reflected, as zlib's crc32) and ISIZE u32 = LEN.
 * eof != 0 appends the 28-byte BGZF end-of-file block (KISS_HIP_BGZF_EOF_BYTES).  n = 0 writes no block, only that one when asked.
 * Report: blocks = ceil(n / block_bytes), out_bytes = n + 31 * blocks + 28 * (eof != 0), the device time.
 * out_capacity below out_bytes: KISS_HIP_E_INVALID with the totals in the report, NOTHING WRITTEN.  Other KISS_HIP_E_INVALID: ctx
 * NULL, data NULL with n > 0, out NULL with out_capacity > 0.  data and out may lie at any address and must not overlap.
 * KNOWN PROPERTY: one workgroup frames one block: it reads the payload once into LDS, copies it out and checksums it there; every
 * lane runs a table-driven CRC over a contiguous piece and the pieces are combined by multiplication with x^(8 len) modulo the
 * polynomial.  All addressing is 64-bit.  The kernels count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_BAM_H
#define KISS_HIP_BAM_H

#include "kiss_hip_sam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_BGZF_BLOCK_DEFAULT 65280u
#define KISS_HIP_BGZF_BLOCK_MAX 65505u
#define KISS_HIP_BGZF_OVERHEAD 31u
#define KISS_HIP_BGZF_EOF_BYTES 28u

typedef struct kiss_hip_bam_report {
    uint64_t records, bam_bytes, unmapped_records, longest, bad, first_bad;
    /* count: the checks, the records of every read, the bytes of every record and the two scans; emit: the pass that writes */
    float ms_total, ms_count, ms_emit;
    uint32_t reserved_;
} kiss_hip_bam_report;

typedef struct kiss_hip_bgzf_report {
    uint64_t blocks, out_bytes;
    float ms_total;
    uint32_t reserved_;
} kiss_hip_bgzf_report;

/* in and report are host pointers; every other pointer, and every pointer inside *in, is a device pointer */
int kiss_hip_fmi_bam_dev(kiss_hip_ctx *ctx, const kiss_hip_sam_input *in, uint8_t *bam, uint64_t bam_capacity, uint64_t *rec_index,
                         uint64_t rec_capacity, uint64_t *read_rec, kiss_hip_bam_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_sam_host) */
int kiss_hip_fmi_bam_host(const kiss_hip_sam_input *in, uint8_t *bam, uint64_t bam_capacity, uint64_t *rec_index, uint64_t rec_capacity,
                          uint64_t *read_rec, kiss_hip_bam_report *report, int device);

/* report is a host pointer, data and out are device pointers */
int kiss_hip_bgzf_dev(kiss_hip_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                      kiss_hip_bgzf_report *report, void *stream);
/* the same with host pointers */
int kiss_hip_bgzf_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                       kiss_hip_bgzf_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
