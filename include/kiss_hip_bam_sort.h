/* kiss_hip_bam_sort.h -- the BAM records of a file put into coordinate order on the device (kiss_hip_bam_sort_*): what stands
 * between kiss_hip_fmi_bam_* and kiss_hip_bgzf_* / kiss_hip_bgzf_deflate_* for a file whose header says SO:coordinate.
 * kiss_amd/csrc/bam_sort.hip; the definition restated as plain loops in tests/bam_sort_model.py.  Declared
 * beside kiss_hip_bam.h, which it includes: the status codes, the ctx and the two promises of a device entry (stream, alignment)
 * are the ones written in kiss_hip_sam.h.
 *
 * INPUT.  bam[0, bam_bytes) holds unframed BAM records one after the other and rec_index, records + 1 u64, is the CSR over them,
 * as kiss_hip_fmi_bam_* writes both: record r is bam[rec_index[r], rec_index[r + 1]).  Of a record the call reads three fields,
 * all little-endian i32: block_size at byte 0, refID at byte 4, pos at byte 8.  A record lies at no particular alignment; the
 * fields are read from naturally aligned words.  n_ref is the number of references of the file's header.
 *
 * ORDER.  Record a comes before record b iff key(a) < key(b), or the keys are equal and a < b (the sort is stable).
 * key = (rk, pos + 1), compared lexicographically; rk = refID for 0 <= refID < n_ref and rk = n_ref for refID == -1, so that the
 * records without a place come last.  That is a valid SO:coordinate order: an unmapped mate that was placed at its partner keeps
 * the partner's refID and pos and so stays beside it, as samtools sort has it.  The order is this comparison; how the key is
 * packed is the library's business (rk above pos + 1 in one u64, sorted by the 5 .. 8 byte passes that the bits of n_ref need).
 *
 * BAD INPUT.  Record r is BAD iff
 *   r == 0 and rec_index[0] != 0;  or  r == records - 1 and rec_index[records] != bam_bytes;
 *   rec_index[r + 1] <= rec_index[r] (the index is strictly increasing), or rec_index[r + 1] > bam_bytes (which the two rules
 *     above imply for some record; the record that reaches past the bytes is counted itself, and nothing of it is read);
 *   it has fewer than 36 bytes;
 *   its block_size is not its bytes - 4;
 *   refID < -1 or refID >= n_ref;  pos < -1.
 * All of it is checked on the device, in one pass over the records.  With a BAD record the call returns KISS_HIP_E_INVALID, the
 * report holds bad (how many records) and first_bad (the lowest such r), and NOTHING is written to out, out_index or order.
 *
 * OUTPUT.  out[0, bam_bytes): the records in sorted order, each one byte for byte.  out_index -- optional, records + 1 u64, the
 * CSR of the sorted records, from 0.  order -- optional, records u32: order[s] is the input index of the record in slot s.
 * Report: records and bam_bytes (as given), unplaced (the records with refID == -1), longest (the longest record with its
 * block_size field), bad, first_bad, the times.
 *
 * out_capacity < bam_bytes: KISS_HIP_E_INVALID with records and bam_bytes in the report, NOTHING WRITTEN; the size is known
 * beforehand, so there is no sizing call.  records == 0 (bam_bytes must be 0 then): KISS_HIP_OK and out_index[0] = 0; the host
 * entry needs no device for it.  records >= 2^32, or more records than the ctx can sort (its reservation for max_n, as
 * kiss_hip_fmi_select_dev has it): KISS_HIP_E_UNSUPPORTED.  Other KISS_HIP_E_INVALID: ctx NULL, rec_index NULL, bam NULL with
 * bam_bytes > 0, out NULL with out_capacity > 0.  report may be NULL.
 * bam and out may lie at any byte address and must not overlap; rec_index and out_index are 8-byte aligned, order 4-byte.
 * Scratch lives in slots of the ctx: no allocation after the first call of a size.  Everything runs on the caller's stream.
 * KNOWN PROPERTY: one lane checks one record and writes its key; the stable radix sort of the library orders (key, index);
 * one wave copies 2048 destination bytes, whatever records they belong to (it finds its first record by a search in the sorted
 * CSR), as naturally aligned 4-byte words that a byte funnel shift makes of two naturally aligned source words; bytes in front
 * of the first word, behind the last one and in a word that two records share are written singly.  A long record is therefore
 * copied by as many waves as it has granules.  All addressing is 64-bit.  The kernels count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_BAM_SORT_H
#define KISS_HIP_BAM_SORT_H

#include "kiss_hip_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_BAM_RECORD_MIN 36u /* block_size and the 32 bytes of the fixed part */

typedef struct kiss_hip_bam_sort_report {
    uint64_t records, bam_bytes, unplaced, longest, bad, first_bad;
    /* key: the checks and the keys; sort: the radix sort; copy: the sizes in sorted order, their scan and the gather */
    float ms_total, ms_key, ms_sort, ms_copy;
} kiss_hip_bam_sort_report;

/* report is a host pointer, every other pointer a device pointer */
int kiss_hip_bam_sort_dev(kiss_hip_ctx *ctx, const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                          uint32_t n_ref, uint8_t *out, uint64_t out_capacity, uint64_t *out_index, uint32_t *order,
                          kiss_hip_bam_sort_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_bam_host) */
int kiss_hip_bam_sort_host(const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                           uint8_t *out, uint64_t out_capacity, uint64_t *out_index, uint32_t *order,
                           kiss_hip_bam_sort_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
