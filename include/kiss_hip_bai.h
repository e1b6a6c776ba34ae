/* kiss_hip_bai.h -- the BAI index of a coordinate-sorted BAM file, built on the device from the arrays the file is framed from
 * (kiss_hip_bai_*): what stands behind kiss_hip_bam_sort_* and beside kiss_hip_bgzf_* / kiss_hip_bgzf_deflate_*.
 * kiss_amd/csrc/bai.hip; the definition restated as plain loops in tests/bai_model.py.  Declared beside
 * kiss_hip_bam_sort.h, which it includes: the status codes, the ctx and the two promises of a device entry (stream, alignment)
 * are the ones written in kiss_hip_sam.h.
 *
 * INPUT.  bam[0, bam_bytes): unframed BAM records in SO:coordinate order, and rec_index, records + 1 u64, the CSR over them from
 * 0, as kiss_hip_bam_sort_* writes both.  n_ref: the references of the file's header.  block_bytes: the payload bytes with which
 * the records are framed (0: 65280; 1 .. 65505).  block_index: optional, blocks + 1 u64 (blocks = ceil(bam_bytes /
 * block_bytes)), the compressed offset of every block as kiss_hip_bgzf_deflate_* writes it; NULL: stored blocks, block b starts
 * at b * (block_bytes + 31).  file_base: the bytes of the file in front of the first record block (the framed header).
 *
 * FIELDS READ OF A RECORD, all little-endian, from the record's start, from naturally aligned words wherever the record lies:
 * block_size (byte 0, i32), refID (4, i32), pos (8, i32), l_read_name (12, u8), n_cigar_op (16, u16), flag (18, u16) and the
 * cigar words at 36 + l_read_name (u32 each, len << 4 | op).  Nothing else is read; the record's bin field is not trusted.
 *
 * INTERVAL of a placed record (refID >= 0): beg = pos.  With flag & 4: end = beg + 1, and the cigar is not read.  Otherwise end =
 * beg + max(1, reflen), reflen the sum (in 64 bits) of the lengths of the ops with code 0, 2, 3, 7 or 8.  bin = reg2bin(beg, end)
 * of the SAM specification; the record covers the 16 KiB windows beg >> 14 .. (end - 1) >> 14.
 *
 * VIRTUAL OFFSETS.  voff_at(u), 0 <= u <= bam_bytes: b = u / block_bytes, coff(b) = file_base + (block_index ? block_index[b] :
 * b * (block_bytes + 31)), voff_at(u) = coff(b) << 16 | u % block_bytes.  voff(r) = voff_at(rec_index[r]), vend(r) =
 * voff_at(rec_index[r + 1]): a record that ends exactly on a block's end ends at offset 0 of the next block (for the last block,
 * of whatever follows the record blocks: the end-of-file block), where a BGZF reader's tell stands after it.  coff(bam_bytes /
 * block_bytes), the largest one, of 2^48 or more: KISS_HIP_E_UNSUPPORTED.  ORDER of the answers, with and without a block_index:
 * a block_index that decreases, then BAD records, then an offset that is too far: records that are BAD and too far are BAD.
 *
 * BAD INPUT.  Record r is BAD by any BAD kind of kiss_hip_bam_sort.h, or
 *   r > 0, neither r nor r - 1 is BAD by one of those kinds, and key(r) < key(r - 1) with that header's key (not sorted);
 *   refID >= 0 and pos == -1;
 *   not flag & 4, and 36 + l_read_name + 4 * n_cigar_op exceeds the record's bytes;
 *   not flag & 4, and an op code above 8 (the ops are not read when the rule above holds);
 *   refID >= 0 and end > 2^29: the BAI format ends there, and the CSI index is not built.
 * A record counts once.  With a BAD record the call returns KISS_HIP_E_INVALID, the report holds bad and first_bad (bai_bytes
 * stays 0), and NOTHING is written.
 *
 * OUTPUT.  bai[0, bai_bytes) holds the bytes of FILE.bai:
 *   "BAI\1"; n_ref i32
 *   per reference, in order:
 *     n_bin i32
 *     per bin in ascending bin number: bin u32; n_chunk i32; (chunk_beg u64, chunk_end u64) x n_chunk
 *     n_intv i32; ioffset u64 x n_intv
 *   n_no_coor u64
 * Chunks: the records of a reference, in file order, fall into maximal runs of consecutive records with the same bin; each run
 * is one chunk (voff(first), vend(last)) of that bin, and a bin's chunks stand in file order.  NO FURTHER MERGING: the format
 * allows it and does not require it, so the bytes need not equal those of `samtools index`; what is claimed is a valid index per
 * the specification.  Pseudo-bin 37450: present iff the reference has a record, last; two chunks, (voff(first record of the
 * reference), vend(last one)) and (n_mapped, n_unmapped), unmapped meaning flag & 4.  Linear index: n_intv = 1 + max((end - 1) >>
 * 14) over the reference's records, 0 without records; ioffset[w] is the smallest voff(r) over the records that cover window w; a
 * window that no record covers takes the value of the nearest covered window to its right (the last one is always covered).  A
 * reference without records has n_bin = 0 and n_intv = 0.  n_no_coor: the records with refID == -1.
 * Report: records, bam_bytes (as given), bai_bytes, chunks, bins (real bins, without the pseudo-bins), windows (the sum of n_intv),
 * mapped (placed, not flag & 4), unmapped_placed (placed, flag & 4), no_coor, bad, first_bad, the times.
 *
 * PROTOCOL.  SIZE, THEN FILL, as kiss_hip_fmi_bam_*: bai_capacity < bai_bytes is KISS_HIP_E_INVALID with the totals in the report
 * and NOTHING WRITTEN; bai may be NULL while the capacity is 0.  records == 0 (bam_bytes must be 0 then): KISS_HIP_OK and the 8 +
 * 8 * n_ref + 8 bytes of an empty index; the host entry needs no device for it.  KISS_HIP_E_INVALID: ctx NULL, rec_index NULL, bam
 * NULL with bam_bytes > 0, bai NULL with bai_capacity > 0, block_bytes above 65505, a block_index that decreases (checked on the
 * device, before the records).  KISS_HIP_E_UNSUPPORTED: records >= 2^32, n_ref >= 2^31, file_base >= 2^48, or more records,
 * references, chunks or windows (2^32 in all) than the ctx sorts in its work arrays and scans in its scratch.  report may be NULL.
 * bam and bai may lie at any byte address and must not overlap; rec_index and block_index are 8-byte aligned.  The fields of bai
 * are 4-aligned within the file only: a u64 is written as two words, and where bai itself is not 4-aligned, as single bytes.  No
 * access is not naturally aligned.  Scratch lives in slots of the ctx: no allocation after the first call of a size.  Everything
 * runs on the caller's stream.  The kernels count under KISS_HIP_K_FM_QUERY.
 * KNOWN PROPERTY: one lane per record; a cigar above 8 ops and a record above 4 windows are handed to the whole wave.  The window
 * minima are u32 atomic minima of the record index (file order is beg order); the chunks are ordered by the library's stable
 * radix sort over (reference, bin); one scan gives every byte offset.  No LDS, no scratch memory. */
#ifndef KISS_HIP_BAI_H
#define KISS_HIP_BAI_H

#include "kiss_hip_bam_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_BAI_PSEUDO_BIN 37450u
#define KISS_HIP_BAI_MAX_END (1u << 29)

typedef struct kiss_hip_bai_report {
    uint64_t records, bam_bytes, bai_bytes, chunks, bins, windows, mapped, unmapped_placed, no_coor, bad, first_bad;
    /* record: the checks, intervals, runs and their scans; window: the window minima and the chunk records; sort: the radix sort
     * of the chunks; emit: the sizes, their scan and the bytes */
    float ms_total, ms_record, ms_window, ms_sort, ms_emit;
} kiss_hip_bai_report;

/* report is a host pointer, every other pointer a device pointer */
int kiss_hip_bai_dev(kiss_hip_ctx *ctx, const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                     uint32_t n_ref, uint32_t block_bytes, const uint64_t *block_index, uint64_t file_base, uint8_t *bai,
                     uint64_t bai_capacity, kiss_hip_bai_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_bam_sort_host) */
int kiss_hip_bai_host(const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                      uint32_t block_bytes, const uint64_t *block_index, uint64_t file_base, uint8_t *bai, uint64_t bai_capacity,
                      kiss_hip_bai_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
