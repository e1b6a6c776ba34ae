/* kiss_hip_pileup.h -- per-position pileup counts of the mappings, accumulated on the device (kiss_amd/csrc/fm_pileup.hip;
 * DESIGN.md 4.21; the definition restated in tests/fm_pileup_model.py).  Declared beside kiss_hip.h and kiss_hip_md.h: the
 * status codes, the ctx, the records and the two promises of a device entry (stream, alignment) are the ones written there.
 *
 * A pileup answers "what does the data say at text position j": how many aligned read bases cover it, which of them differ
 * from the text, how many reads delete it, how many insert something behind it.  Its size depends on the text and not on the
 * reads, so it is the one result of the mapper that can be summed over any number of batches.
 *
 * THE DEFINITION.
 * Input: text (n bytes), reads / read_index / Q / both_strands, alns, chain_index (V + 1), cigar and cigar_index (C + 1) exactly
 * as kiss_hip_fmi_md_dev takes them; the virtual read of an alignment, its read Rv (the reverse complement read in place for odd
 * v under both_strands) and the op words (len << 4 | op) are the ones written in kiss_hip_md.h.  Optionally hits with H, and
 * pairs with P (pairs needs hits); params; a WINDOW lo <= hi <= n of text positions, W = hi - lo; counts: 8 PLANES of W u32,
 * plane-major: plane k, position j is counts[k * W + (j - lo)]; accumulate.
 * Planes: 0 COV, 1..4 ALT_A ALT_C ALT_G ALT_T, 5 ALT_N, 6 DEL, 7 INS (KISS_HIP_PILEUP_*).
 * ITEMS, their MAPQ and flags:
 *   neither hits nor pairs: item a is alignment a, C items, NO FILTER (params are checked and otherwise ignored).
 *   hits without pairs: item h is hits[h] (0 <= h < H): aln, flags and mapq are the hit's.
 *   pairs: 2 P items, item 2 p + m is mate m of pair p.  pairs[p].flags & KISS_HIP_PAIR_BAD_INPUT: both items are BAD.  Else a
 *     hit index (hit1 / hit2) of KISS_HIP_PAIR_NONE: the item is UNMAPPED; a hit index >= H: BAD.  Else with proper_only != 0
 *     and a pair without KISS_HIP_PAIR_PROPER: FILTERED.  Else aln is that hit's, mapq is mapq1 / mapq2 of the pair and flags
 *     are the hit's with KISS_HIP_HIT_SECONDARY cleared: the chosen hit is the mate's primary line, as in the SAM.
 *     (Supplementary hits of paired reads are not items.)
 *   An item with mapq < min_mapq or flags & skip_flags is FILTERED; its alignment is not looked at.
 *   Then the item is BAD exactly when the MD call calls it bad: aln >= C, or the alignment has ops and one of: an op code above
 *   2 or a length of 0, lengths that do not add up to the record, rend > L, tend > n, rbeg > rend, tbeg > tend.
 *   Every other item is COUNTED -- one whose alignment has no ops too: it adds nothing and is not bad.
 *   BAD, FILTERED and UNMAPPED items add nothing and are counted in the report; the call still returns KISS_HIP_OK.
 *   items = bad + filtered + unmapped + counted.
 * WALK of a counted item: i = rbeg, j = tbeg; through the ops in order:
 *   M (0) of length l, per column: add 1 to COV at j; if Rv[i] > 3 add 1 to ALT_N at j, else if Rv[i] != text[j] add 1 to plane
 *         1 + Rv[i] at j (a text byte above 3 never equals a base); then i += 1, j += 1.
 *   D (2) of length l: add 1 to DEL at each of j .. j + l - 1; j += l.
 *   I (1) of length l: add 1, once per op, to INS at j - 1, the last text position in front of the inserted bases; with j == 0
 *         there is no such position and nothing is added; i += l.
 *   An add at a position outside [lo, hi) is dropped and counted in `clipped`.  Adds are modulo 2^32.
 * So the read bases equal to the text at j number COV - ALT_A - ALT_C - ALT_G - ALT_T - ALT_N, and the depth in samtools' sense
 * is COV + DEL.
 * accumulate == 0: all 8 W words are zeroed first (with zero items too); otherwise the call adds onto what is there.
 * Report: items, bad, filtered, unmapped, counted; over the counted items, inside the window or not: columns (M columns),
 * alt_columns (M columns that add to one of ALT_A .. ALT_N), deleted_bases (the lengths of the D ops), insertions (the I ops, one
 * at j == 0 too); clipped (the adds dropped); the device times.
 * Nothing outside text[0, n), the read of the item and counts[0, 8 W) is ever touched, whatever the records hold.
 * KISS_HIP_E_INVALID, with counts untouched: a required pointer NULL (every input but hits and pairs; params; counts unless
 * W == 0); pairs without hits; lo > hi or hi > n; reserved_ != 0; min_mapq > 255; a bit of skip_flags outside the three hit
 * flags; a chain_index, read_index or cigar_index that decreases; a zero-length read.
 * Limits (KISS_HIP_E_UNSUPPORTED): n above KISS_HIP_MAX_N; V of 2^31 or more; H, 2 P or C of 2^32 or more.
 * Alignment: counts 4 bytes; text and reads any address; alns, hits, pairs (read field by field) and cigar 4 bytes; the three
 * indices 8 bytes.
 * KNOWN PROPERTY: one wave walks one item, op by op, 64 columns of an op per step, one atomic add per column and plane; many
 * items on one position queue up on that word.  All addressing is 64-bit.  The kernels also count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_PILEUP_H
#define KISS_HIP_PILEUP_H

#include "kiss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_PILEUP_PLANES 8u
#define KISS_HIP_PILEUP_COV 0u
#define KISS_HIP_PILEUP_ALT_A 1u
#define KISS_HIP_PILEUP_ALT_C 2u
#define KISS_HIP_PILEUP_ALT_G 3u
#define KISS_HIP_PILEUP_ALT_T 4u
#define KISS_HIP_PILEUP_ALT_N 5u
#define KISS_HIP_PILEUP_DEL 6u
#define KISS_HIP_PILEUP_INS 7u

/* the defaults of the Python entries and of the command line: 0, KISS_HIP_HIT_SECONDARY, 0 */
typedef struct kiss_hip_pileup_params { uint32_t min_mapq, skip_flags, proper_only, reserved_; } kiss_hip_pileup_params;

typedef struct kiss_hip_pileup_report {
    uint64_t items, bad, filtered, unmapped, counted;
    uint64_t columns, alt_columns, deleted_bases, insertions, clipped;
    /* check: the indices; walk: the zeroing and the one kernel that adds */
    float ms_total, ms_check, ms_walk;
    uint32_t reserved_;
} kiss_hip_pileup_report;

/* every pointer except params and report is a device pointer */
int kiss_hip_fmi_pileup_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            int both_strands, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar,
                            const uint64_t *cigar_index, const kiss_hip_hit *hits, uint64_t H, const kiss_hip_pair *pairs, uint64_t P,
                            const kiss_hip_pileup_params *params, uint64_t lo, uint64_t hi, uint32_t *counts, int accumulate,
                            kiss_hip_pileup_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_md_host).  counts_on_device != 0: counts
 * alone is a device pointer (kiss_hip_alloc_dev), so that a host program accumulates over many calls and fetches the sums once
 * (kiss_hip_copy_to_host). */
int kiss_hip_fmi_pileup_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q, int both_strands,
                             const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar, const uint64_t *cigar_index,
                             const kiss_hip_hit *hits, uint64_t H, const kiss_hip_pair *pairs, uint64_t P,
                             const kiss_hip_pileup_params *params, uint64_t lo, uint64_t hi, uint32_t *counts, int counts_on_device,
                             int accumulate, kiss_hip_pileup_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
