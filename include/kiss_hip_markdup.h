/* kiss_hip_markdup.h -- the duplicate templates of a BAM file marked on the device (kiss_hip_bam_markdup_*): FLAG 0x400 set on
 * every record of a template that repeats the ends of a better one, what `samtools markdup` or Picard MarkDuplicates do on the
 * host between the sort and the index.  It stands between kiss_hip_fmi_bam_* and kiss_hip_bam_sort_*: the records are marked in
 * the order they were written, where the records of a read are contiguous and the two mates of a pair adjacent, so that no
 * ms / MC tag of `samtools fixmate` is needed.  kiss_amd/csrc/bam_markdup.hip; the definition restated as plain
 * loops in tests/markdup_model.py.  It includes kiss_hip_bam_sort.h: the status codes, the ctx and the two promises of a device
 * entry (stream, alignment) are the ones written in kiss_hip_sam.h, the BAD kinds of a record's head those of the sort.
 *
 * INPUT.  bam[0, bam_bytes) holds unframed BAM records one after the other and rec_index, records + 1 u64, is the CSR over them,
 * as kiss_hip_fmi_bam_* writes both, IN THE ORDER IT WRITES THEM (not sorted).  n_ref is the number of references of the header.
 * The call reads of a record: block_size, refID, pos, l_read_name, n_cigar_op, flag, l_seq, read_name, cigar and qual.
 *
 * DEFINITION.
 *   template   a maximal run of consecutive records whose read_name fields are equal: the same l_read_name and the same
 *              l_read_name bytes (the closing NUL is one of them, whatever it holds).  Templates are numbered in file order.
 *   primary    a record with flag & 0x900 == 0.  A primary is mapped iff flag & 4 == 0 and refID >= 0.
 *   end        of a mapped primary: (refID, u5, strand), compared lexicographically.  strand = flag >> 4 & 1.
 *              lead  = the sum of the lengths of the ops of the longest prefix of the cigar that holds only S and H ops,
 *              trail = the same of the longest suffix (a cigar of nothing but S and H ops: both are the whole cigar),
 *              reflen = the sum of the lengths of its M, D, N, = and X ops.
 *              strand 0: u5 = pos - lead;  strand 1: u5 = pos + reflen - 1 + trail.  (No cigar: lead = trail = reflen = 0.)
 *              u5 is computed in i64; -2^32 <= u5 < 2^32 must hold (see BAD INPUT).
 *   score      of a template: the sum, over its primary records (mapped or not), of the qual bytes q with min_qual <= q and
 *              q != 0xFF, in u64.  (min_qual = 15: Picard's SUM_OF_BASE_QUALITIES.  min_qual > 255 counts nothing.)
 *   class      of a template, by its mapped primaries:
 *                none       there is none;
 *                fragment   there is exactly one;
 *                pair       there are exactly two, one with flag & 0xC0 == 0x40 and the other with flag & 0xC0 == 0x80;
 *                ambiguous  anything else.  Never a duplicate, never the reason for one.
 *              The key of a pair is (lo, hi): its two ends, the smaller one first (which mate it belongs to is not in the key).
 *   duplicates Among the pairs of one key the one with the highest score is kept, ties to the lowest template; every other pair
 *              of that key is a duplicate.  A fragment is a duplicate if any pair (duplicate or not) has an end equal to the
 *              fragment's end; otherwise among the fragments of one end the highest score is kept, ties to the lowest template,
 *              and the others are duplicates.
 *
 * OUTPUT.  Every record of a duplicate template -- secondary and supplementary records and an unmapped mate included -- gets
 * flag | 0x400, every other record flag & ~0x400 (a stale bit is cleared); nothing else of bam changes, no size, so rec_index
 * and whatever was derived from the other fields (sort keys, bins, an index) stay what they were.  dup -- optional, records
 * bytes: dup[r] = 1 iff record r belongs to a duplicate template, else 0.
 * Report: records (as given), templates, pairs, fragments, unmapped_templates (class none), ambiguous; dup_pairs and dup_fragments
 * (templates), dup_records (records that carry 0x400 afterwards); bad, first_bad; the times.
 *
 * BAD INPUT.  Record r is BAD iff
 *   it is BAD by any kind of kiss_hip_bam_sort.h (the index, fewer than 36 bytes, block_size, refID, pos);  or
 *   l_read_name == 0;  or
 *   36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > its bytes (the fixed fields ask for more than the record has;
 *     nothing behind the fixed part of such a record is read);  or
 *   one of its cigar ops has a code above 8 (every record's cigar is checked, mapped or not);  or
 *   it is a mapped primary and u5 < -2^32 or u5 >= 2^32 (the packed end does not hold it; a clip of 2^32 bases is no read).
 * All of it is checked on the device.  With a BAD record the call returns KISS_HIP_E_INVALID, the report holds bad (how many
 * records) and first_bad (the lowest such r), and NOTHING is written to bam or dup.
 *
 * records == 0 (bam_bytes must be 0 then): KISS_HIP_OK, the host entry needs no device for it.  KISS_HIP_E_UNSUPPORTED:
 * records >= 2^32, or more records than the ctx can sort (its reservation for max_n, as kiss_hip_bam_sort_dev has it: the items
 * that are sorted are never more than the records); n_ref >= 2^30 (an end is packed into one u64: 30 bits of refID, 33 of u5,
 * the strand); bam_bytes > 2^54 (a score stays below 2^63).  KISS_HIP_E_INVALID: ctx NULL, rec_index NULL, bam NULL with
 * bam_bytes > 0, records == 0 with bam_bytes > 0.  dup and report may be NULL.
 * bam and dup may lie at any byte address and must not overlap; rec_index is 8-byte aligned.  Scratch lives in slots of the
 * ctx: no allocation after the first call of a size.  Everything runs on the caller's stream.
 * KNOWN PROPERTY: one lane checks one record, compares its name with its predecessor's and sums a cigar of up to 8 ops and a
 * qual of up to 256 bytes; longer ones are handed to the whole wave.  The lane of a template's first record then walks the
 * records of its template (one lane, however many records share the name), classes it and, behind one scan, writes its items:
 * one per fragment and two per pair keyed by end, one per pair keyed by (lo, hi).  The library's stable radix sort orders both
 * kinds, word after word from the least significant, by the byte passes that the bits in use ask for; an item whose predecessor
 * in that order has the same key is a duplicate (for a fragment: a pair's item or a better fragment stands in front of it).
 * One lane per record then rewrites the byte that holds 0x400 (byte 19 of the record), as a single-byte store.  All addressing
 * is 64-bit.  The kernels count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_MARKDUP_H
#define KISS_HIP_MARKDUP_H

#include "kiss_hip_bam_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_MARKDUP_MIN_QUAL_DEFAULT 15u
#define KISS_HIP_MARKDUP_MAX_N_REF 0x3FFFFFFFu /* n_ref up to here */
#define KISS_HIP_BAM_FLAG_DUP 0x400u

typedef struct kiss_hip_markdup_report {
    uint64_t records, templates, pairs, fragments, unmapped_templates, ambiguous;
    uint64_t dup_pairs, dup_fragments, dup_records;
    uint64_t bad, first_bad;
    /* record: the checks, names, ends and scores; class: the templates classed, the scan, their items; sort: the radix sorts
     * and the run heads; mark: the flags rewritten */
    float ms_total, ms_record, ms_class, ms_sort, ms_mark;
} kiss_hip_markdup_report;

/* report is a host pointer, every other pointer a device pointer; bam is marked in place */
int kiss_hip_bam_markdup_dev(kiss_hip_ctx *ctx, uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                             uint32_t n_ref, uint32_t min_qual, uint8_t *dup, kiss_hip_markdup_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_bam_sort_host) */
int kiss_hip_bam_markdup_host(uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                              uint32_t min_qual, uint8_t *dup, kiss_hip_markdup_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
