/* kiss_hip_sam.h -- the alignment lines of the SAM output, written on the device (kiss_amd/csrc/fm_sam.hip; the
 * definition restated in tests/fm_sam_model.py, which is held byte for byte against the host writer of the command line).
 * Declared beside kiss_hip.h, which it includes: the status codes, the ctx, the records and the two promises of a device entry
 * (stream, alignment) are the ones written there.
 *
 * THE DEFINITION.
 * Input (kiss_hip_sam_input, filled on the host as a kiss_hip_fmi_view is; every pointer in it is a device pointer for the _dev
 * entry and a host pointer for the _host entry):
 *   reads, read_index (Q + 1 u64), Q: the codes of the reads (0..3, anything above prints N) as every call takes them;
 *   qual: the quality bytes under the same index, printed as they stand; NULL prints '*';
 *   names, name_off (Q u64), name_len (Q u32): QNAME of read q is names[name_off[q] .. + name_len[q]), the spans as
 *     kiss_hip_reads_parse_dev writes them.  The bytes are printed as they stand: the caller strips /1 and /2 and supplies
 *     names for reads that have none.  The spans are trusted to lie inside names;
 *   alns and C, cigar, cigar_index (C + 1 u64): as the align or the merge call wrote them (ops: len << 4 | op).  cigar_index is
 *     trusted to point inside cigar;
 *   hits, hit_index (Q + 1 u64): as the select call wrote them; H = hit_index[Q], the hits of read q are
 *     [hit_index[q], hit_index[q + 1]);
 *   pairs: NULL means single end.  Otherwise Q / 2 kiss_hip_pair records, reads 2 p and 2 p + 1 are the mates of pair p, and Q
 *     must be even;
 *   source (NULL, or C u32) and first_alns: the merge call's aln_source; an alignment a with source[a] >= first_alns came from
 *     the rescue;
 *   md (NULL: no MD:Z: field) and md_index (H + 1 u64): the strings of the MD call made with hits, one per hit.  md_index is
 *     trusted to point inside md;
 *   ref_names, ref_name_index (R + 1 u64), bounds (R + 1 u64), R: the name of record r is
 *     ref_names[ref_name_index[r] .. ref_name_index[r + 1]), its first text position bounds[r].  R = 0: RNAME is '*' and POS
 *     is the text position + 1.
 * The lines.  Columns are separated by a tab, a line ends with '\n'.
 *   A HIT LINE of hit h (alignment k = alns[hits[h].aln]) of read q (L bases): QNAME; FLAG; RNAME (the name of record
 *   hits[h].ref); POS = k.tbeg - bounds[ref] + 1; MAPQ; CIGAR = [k.rbeg 'S'] the ops as <len><M|I|D> (a code above 2 prints '?')
 *   [L - k.rend 'S']; RNEXT; PNEXT; TLEN; SEQ ("ACGT"[c], N above 3; for a reverse hit the reverse complement); QUAL (reversed
 *   for a reverse hit); NM:i: (k.mismatches + k.ins + k.del) modulo 2^32; MD:Z: with md; AS:i: the hit's score; XS:i: the
 *   hit's sub unless the hit is SECONDARY; then YS:i:, YT:Z:CP and YR:i:1 as below.
 *   FLAG = the bits of the line, 16 for a REVERSE hit and, unless the line is the CHOSEN one of a pair, 256 for SECONDARY and
 *   2048 for SUPPLEMENTARY.
 *   AN UNMAPPED LINE of read q: QNAME; FLAG = bits | 4; RNAME and POS of its place, or '*' and 0; 0; '*'; '=' with a place,
 *   else '*'; PNEXT = POS; 0; SEQ and QUAL forward.  No tags.
 *   SINGLE END: read q has max(1, its hits) lines: its hits in hit order with bits 0, RNEXT '*', PNEXT 0, TLEN 0, the hit's
 *   MAPQ; or the unmapped line with bits 0 and no place.
 *   PAIRED: the lines of mate 1, then of mate 2.  For mate i (0 / 1) of pair p: mine = its chosen hit (hit1 / hit2), other =
 *   the partner's; 0xFFFFFFFF is none.  bits = 1 | (64, 128 for i = 0, 1) | 8 if other is none | 32 if other is REVERSE.  The
 *   PLACE is (RNAME, POS) of other, else of mine, else none.  mine none: ONE unmapped line at the place, whatever hits the mate
 *   has.  Else first the CHOSEN line, hit mine: bits | 2 if the pair is PROPER; MAPQ = mapq1 / mapq2 of the pair; TLEN = the
 *   pair's tlen when other is set and tlen is not 0, positive when tbeg(mine) < tbeg(other) or they are equal and i = 0, else
 *   negative; YS:i: the score of other when set; YT:Z:CP when PROPER.  Then the mate's other hits in hit order: bits, the hit's
 *   own MAPQ, TLEN 0; the mate's hit number 0, displaced by the pair, gets bits | 256 and MAPQ 0.  On every hit line of a pair:
 *   PNEXT = POS of the place; RNEXT = '=' when the name BYTES of the place's record and the line's record are equal (two
 *   records of one name give '='; with R = 0 always '='), else the name of the place's record; YR:i:1 when source is given
 *   and source[aln] >= first_alns.  YR:i:1 only with pairs.
 * A read is BAD iff a hit of it has aln >= C or (R > 0 and) ref >= R, or its alignment has rbeg > rend, rend > L or (R > 0 and)
 * tbeg < bounds[ref]; or its pair carries KISS_HIP_PAIR_BAD_INPUT or chooses for it a hit outside the read's own.  With a BAD
 * read the call returns KISS_HIP_E_INVALID, the report holds bad (how many) and first_bad (the first one), and NOTHING is
 * written to sam, line_index or read_line.  For a BAD read no byte outside its own records is read.
 * Output: sam -- the lines, ASCII, no terminator; line_index -- optional, lines + 1 u64, CSR over the lines, from 0; read_line
 * -- Q + 1 u64, the first line of every read, read_line[Q] = lines.
 * Report: lines, sam_bytes, unmapped_lines, longest (the longest line), bad, first_bad, the device times.
 * SIZE, THEN FILL (the MD call's protocol): sam_capacity below sam_bytes, or line_index given and line_capacity below lines:
 * KISS_HIP_E_INVALID with the totals in the report, NOTHING WRITTEN; call again with room.  sam may be NULL while sam_capacity
 * is 0.
 * Other KISS_HIP_E_INVALID: a required pointer NULL (in, read_line; reads, read_index, names, name_off, name_len, alns, cigar,
 * cigar_index, hits, hit_index; md_index with md; ref_names, ref_name_index and bounds with R > 0); Q odd with pairs; a
 * read_index, hit_index, cigar_index, md_index or ref_name_index that decreases; a zero-length read.
 * Zero reads: KISS_HIP_OK, read_line[0] = 0 (and line_index[0] = 0).
 * Limits (KISS_HIP_E_UNSUPPORTED): Q of 2^31 or more; 2^32 hits, alignments, records or lines or more; more reads or lines
 * than the ctx's scratch scans (a ctx created with max_n >= 4 * (lines + 1) always holds them).
 * Alignment: reads, qual, names, md, ref_names and sam any address; alns, hits, pairs (read field by field), cigar, name_len
 * and source 4 bytes; every index, name_off, bounds, line_index and read_line 8 bytes.
 * KNOWN PROPERTY: one wave writes one line; the numbers and tags of a line are written by one lane each, SEQ, QUAL, the names,
 * MD and the ops by the lanes together.
 * All addressing is 64-bit.  The kernels also count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_SAM_H
#define KISS_HIP_SAM_H

#include "kiss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kiss_hip_sam_input {
    const uint8_t *reads;
    const uint64_t *read_index;
    const uint8_t *qual;
    const uint8_t *names;
    const uint64_t *name_off;
    const uint32_t *name_len;
    const kiss_hip_aln *alns;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const kiss_hip_hit *hits;
    const uint64_t *hit_index;
    const kiss_hip_pair *pairs;
    const uint32_t *source;
    const uint8_t *md;
    const uint64_t *md_index;
    const uint8_t *ref_names;
    const uint64_t *ref_name_index;
    const uint64_t *bounds;
    uint64_t Q, C, R, first_alns;
} kiss_hip_sam_input;

typedef struct kiss_hip_sam_report {
    uint64_t lines, sam_bytes, unmapped_lines, longest, bad, first_bad;
    /* count: the checks, the lines of every read, the bytes of every line and the two scans; emit: the pass that writes */
    float ms_total, ms_count, ms_emit;
    uint32_t reserved_;
} kiss_hip_sam_report;

/* in and report are host pointers; every other pointer, and every pointer inside *in, is a device pointer */
int kiss_hip_fmi_sam_dev(kiss_hip_ctx *ctx, const kiss_hip_sam_input *in, uint8_t *sam, uint64_t sam_capacity, uint64_t *line_index,
                         uint64_t line_capacity, uint64_t *read_line, kiss_hip_sam_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_md_host) */
int kiss_hip_fmi_sam_host(const kiss_hip_sam_input *in, uint8_t *sam, uint64_t sam_capacity, uint64_t *line_index,
                          uint64_t line_capacity, uint64_t *read_line, kiss_hip_sam_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
