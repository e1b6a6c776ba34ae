/* kiss_hip_md.h -- the MD:Z tag of alignments, written on the device (kiss_amd/csrc/fm_md.hip; the definition
 * restated in tests/fm_md_model.py).  Declared beside kiss_hip.h, which it includes: the status codes, the ctx, the records and
 * the two promises of a device entry (stream, alignment) are the ones written there.
 *
 * The MD string of an alignment says which text bases lie under it, so that a reader of the SAM line recovers the reference
 * without the genome.  It can only be made where the text, the read and the ops meet: nothing the align call leaves behind
 * holds it (the record has counts, the CIGAR has M for matches and mismatches alike).
 *
 * THE DEFINITION.
 * Input: text (n bytes of 0..3), reads / read_index / Q / both_strands exactly as in kiss_hip_fmi_align_dev; alns, chain_index
 * (V + 1 u64, V = 2 Q with both_strands, else Q), cigar and cigar_index (C + 1 u64) as the align call or the merge call wrote
 * them, C = chain_index[V] - chain_index[0].  cigar_index is trusted to point inside cigar, read_index inside reads.
 * Optionally hits with H, as kiss_hip_fmi_select_dev wrote them: ITEM h (0 <= h < H) is alignment hits[h].aln; no other field
 * of a hit is read, a hit may name any alignment, and two hits may name the same one.  hits == NULL (H is then ignored): item a
 * is alignment a, and there are C items.
 * Alignment a belongs to the LARGEST virtual read v with chain_index[v] <= chain_index[0] + a (< chain_index[v + 1]).  Its read
 * Rv is read v / 2 (both_strands) or v; for odd v under both_strands the reverse complement, read in place: Rv[i] =
 * comp(R[L - 1 - i]), comp(x) = 3 - x for x <= 3 and x for a no-base.
 * Walk of one item: i = rbeg, j = tbeg, run = 0; through the ops (u32, len << 4 | op) in order:
 *   M (0) of length l, per column: if Rv[i] <= 3 and Rv[i] == S[j] then run += 1, else emit run in decimal and the letter
 *         "ACGT"[S[j]] ('N' for a text byte above 3) and set run = 0 -- a no-base never matches --; then i += 1, j += 1.
 *   I (1) of length l: i += l.  An insertion does not end a run.
 *   D (2) of length l: emit run in decimal, '^', the l letters of S[j .. j + l); run = 0, j += l.  The '^' belongs to the OP,
 *         not to adjacency in the text: 2D1I3D gives ..^AC0^GTA.., a mismatch right behind a deletion ^AC0T.
 * At the end emit run.  So the string matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)* and its numbers plus its letters add up to
 * tend - tbeg.
 * An item is BAD iff its aln >= C, or the alignment has ops and one of: an op with a code above 2 or a length of 0; the lengths
 * of the M and I ops do not add up to rend - rbeg; those of the M and D ops do not add up to tend - tbeg; rend > L, tend > n,
 * rbeg > rend or tbeg > tend.  A BAD item gets the empty string and counts of 0 and is counted in the report; the call still
 * returns KISS_HIP_OK.  Nothing outside text[0, n) and the read of the item is ever read, whatever the records hold.
 * An alignment WITHOUT OPS (not aligned, or its band was too wide) is not bad: it gets the empty string and counts of 0.
 * Output: md -- ASCII bytes, no terminator; md_index -- items + 1 u64, CSR over the items, from 0; optional md_counts -- 2 u32
 * per item: the mismatch columns (letters outside a deletion) and the deleted bases.
 * Report: items, bad, md_bytes, mismatch_columns, deleted_bases, longest (the longest string), the device times.
 * SIZE, THEN FILL (the align call's protocol): md_capacity below md_bytes: KISS_HIP_E_INVALID with the totals in the report,
 * NOTHING WRITTEN; call again with room.  md may be NULL while md_capacity is 0.
 * Other KISS_HIP_E_INVALID: a required pointer NULL (every input but hits; md_index), a chain_index, read_index or cigar_index
 * that decreases, a zero-length read.  Zero items: KISS_HIP_OK, md_index[0] = 0.
 * Limits (KISS_HIP_E_UNSUPPORTED): n above KISS_HIP_MAX_N; V of 2^31 or more; 2^32 items or more; more items than the ctx's
 * scratch scans (a ctx created with max_n >= 4 * items always holds them).
 * Alignment: text, reads and md any address; alns, hits (read field by field), cigar and md_counts 4 bytes; the four indices 8
 * bytes.
 * KNOWN PROPERTY: one wave walks one item, op by op, 64 columns of an op per step: an item costs about the sum over its ops of
 * ceil(len / 64) steps.  A 150-base hit has 1 to 5 ops; an item of a thousand one-base ops is slow, and finite.
 * All addressing is 64-bit.  The kernels also count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_MD_H
#define KISS_HIP_MD_H

#include "kiss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kiss_hip_md_report {
    uint64_t items, bad, md_bytes, mismatch_columns, deleted_bases, longest;
    /* count: the checks, the sizing walk and the scan; emit: the walk that writes */
    float ms_total, ms_count, ms_emit;
    uint32_t reserved_;
} kiss_hip_md_report;

/* every pointer except report is a device pointer */
int kiss_hip_fmi_md_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                        int both_strands, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar,
                        const uint64_t *cigar_index, const kiss_hip_hit *hits, uint64_t H, uint8_t *md, uint64_t *md_index,
                        uint32_t *md_counts, uint64_t md_capacity, kiss_hip_md_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_chain_host) */
int kiss_hip_fmi_md_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q, int both_strands,
                         const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar, const uint64_t *cigar_index,
                         const kiss_hip_hit *hits, uint64_t H, uint8_t *md, uint64_t *md_index, uint32_t *md_counts,
                         uint64_t md_capacity, kiss_hip_md_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
