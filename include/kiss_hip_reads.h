/* kiss_hip_reads.h -- files of reads parsed on the device (kiss_amd/csrc/reads.hip; the definition restated in
 * tests/reads_model.py).  Declared beside kiss_hip.h, which it includes: the status codes, the ctx, and the two promises of a
 * device entry (stream, alignment) are the ones written there.
 *
 * THE DEFINITION.  Both formats are line based.  A LINE is a maximal run of bytes between '\n's; a last piece without '\n' is a
 * line if it is not empty, an empty piece behind the last '\n' is none; one trailing '\r' is taken off a line.  Codes: A/a 0,
 * C/c 1, G/g 2, T/t 3, every other byte 4 (a '\r' that is not the last byte of its line among them).
 *   KISS_HIP_READS_LINES : a line that is empty after the strip, or that starts with '>', is no read; every other line is one
 *                          read.  Its NAME is taken from the line directly in front of it if that line starts with '>': the
 *                          bytes behind '>' up to the first space, tab or line end.  No such line, or an empty name: a span of
 *                          length 0 (the caller substitutes the decimal read number).  No qualities.
 *   KISS_HIP_READS_FASTQ : the strict four-line form.  Lines that are empty after the strip are dropped at the END of the file
 *                          only.  Record r is lines 4 r .. 4 r + 3: '@' + name (up to the first space, tab or line end; length
 *                          0: the default name), the sequence (it may be empty: a read of length 0, kept, and counted in
 *                          empty_reads with first_empty), '+' and anything, the quality string (copied byte for byte, as many
 *                          bytes as the sequence).  Roles come from the line number alone: '@' or '+' at the start of a quality
 *                          line means nothing.  A record is BAD with kind 1 (no '@'), 2 (no '+') or 3 (lengths differ), the
 *                          lowest that applies; a last record of fewer than four lines is kind 4 whatever it holds.  With bad
 *                          records the call returns KISS_HIP_E_INVALID, the report carries bad_records, first_bad (the smallest
 *                          bad record index) and first_bad_kind, and nothing is written.  Multi-line FASTQ is refused so.
 *   KISS_HIP_READS_AUTO  : FASTQ iff the first byte of the file is '@', else LINES.
 *
 * kiss_hip_reads_parse_dev: d_raw (bytes bytes, any address) -> d_codes (the codes of the reads one after the other), d_qual (NULL,
 * or the quality bytes at the same offsets; LINES writes none), d_read_index (reads + 1 u64: where read q starts in d_codes),
 * d_name_off / d_name_len (NULL, or per read the span of its name inside d_raw: u64 offset, u32 length).
 * SIZE, THEN FILL: bases_capacity and reads_capacity are the entries available in d_codes / d_qual and in d_name_off /
 * d_name_len; d_read_index holds reads_capacity + 1.  A capacity below the total: KISS_HIP_E_INVALID with report->reads and
 * report->bases filled (always, for a well-formed input) and bad_records == 0, NOTHING WRITTEN; call again with room.  d_codes
 * (and d_qual) may be NULL while bases_capacity is 0.  Nothing is written behind a capacity.
 * Alignment: d_raw, d_codes, d_qual any address; d_read_index and d_name_off 8 bytes; d_name_len 4 bytes.
 * Other KISS_HIP_E_INVALID: ctx, d_read_index or (bytes > 0) d_raw NULL, an unknown format, one of d_name_off / d_name_len
 * without the other.  bytes == 0: KISS_HIP_OK, no reads, d_read_index[0] = 0.
 * Limit (KISS_HIP_E_UNSUPPORTED): bytes above KISS_HIP_READS_MAX_BYTES (offsets into the file are 32-bit), or more bytes than the
 * ctx's scratch scans: a ctx created with max_n >= 4 * bytes always holds the file (its scans take about 0.32 max_n entries).
 * KNOWN PROPERTIES: the codes and qualities are copied by a pass that is parallel over the BYTES of the file, so a read of any
 * length costs what its bytes cost; a name is measured by one lane, so a header line of a megabyte without a blank is walked by
 * one lane.
 * Report: format (the one parsed, never AUTO), lines (of the whole file), reads, bases, no_base (codes of 4), empty_reads and
 * first_empty (FASTQ; KISS_HIP_READS_NONE when there is none), has_qual (FASTQ: 1), bad_records, first_bad (or
 * KISS_HIP_READS_NONE), first_bad_kind (0: none), and the device times of the passes.  report may be NULL.
 * A file that does not fit one call goes through in batches: kiss_hip_reads_part.h, beside this header, parses the first whole
 * records of a chunk and says where the next chunk starts. */
#ifndef KISS_HIP_READS_H
#define KISS_HIP_READS_H

#include "kiss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_READS_AUTO 0
#define KISS_HIP_READS_LINES 1
#define KISS_HIP_READS_FASTQ 2
#define KISS_HIP_READS_NONE 0xFFFFFFFFFFFFFFFFull
#define KISS_HIP_READS_MAX_BYTES 0xFFFFF000ull
#define KISS_HIP_READS_BAD_NO_AT 1u
#define KISS_HIP_READS_BAD_NO_PLUS 2u
#define KISS_HIP_READS_BAD_LENGTHS 3u
#define KISS_HIP_READS_BAD_TRUNCATED 4u

typedef struct kiss_hip_reads_report {
    uint64_t lines, reads, bases, no_base, empty_reads, first_empty, bad_records, first_bad;
    uint32_t format, has_qual, first_bad_kind, reserved_;
    /* lines: newlines counted and the line starts compacted; reads: one lane per line or record, the scan of the lengths; copy:
     * the byte-parallel pass and the index / name spans */
    float ms_total, ms_lines, ms_reads, ms_copy;
} kiss_hip_reads_report;

int kiss_hip_reads_parse_dev(kiss_hip_ctx *ctx, const uint8_t *d_raw, uint64_t bytes, int format, uint8_t *d_codes, uint8_t *d_qual,
                             uint64_t bases_capacity, uint64_t *d_read_index, uint64_t *d_name_off, uint32_t *d_name_len,
                             uint64_t reads_capacity, kiss_hip_reads_report *report, void *stream);
/* the same with host pointers: the upload, the parse and the download on the device's cached one-shot context (as
 * kiss_hip_fmi_chain_host).  name_off / name_len are spans into raw. */
int kiss_hip_reads_parse_host(const uint8_t *raw, uint64_t bytes, int format, uint8_t *codes, uint8_t *qual, uint64_t bases_capacity,
                              uint64_t *read_index, uint64_t *name_off, uint32_t *name_len, uint64_t reads_capacity,
                              kiss_hip_reads_report *report, int device);

/* Two parsed batches made one: read 2 p is read p of the first, read 2 p + 1 read p of the second (the order
 * kiss_hip_fmi_pair_dev expects of mates).  codes_a / index_a (P_a + 1 u64) / qual_a and the same of b in; codes, read_index
 * (P_a + P_b + 1 u64) and qual out.  qual_a, qual_b and qual are given all three or not at all.  Names are not moved: the
 * caller owns them.  *bases_out (may be NULL) = index_a[P_a] + index_b[P_b], the bases of the output.
 * bases_capacity: entries available in codes / qual; below the total: KISS_HIP_E_INVALID with *bases_out set, nothing written.
 * Other KISS_HIP_E_INVALID, nothing written: P_a != P_b (a pair has one read of each), a required pointer NULL, an index that
 * decreases or does not start at 0 (looked at on the device before anything is written).  codes_a / codes_b / codes may be NULL
 * where they hold no base.  KISS_HIP_E_UNSUPPORTED: P_a of 2^31 or more.  Alignment: byte arrays any address, the indices 8
 * bytes.  The copy is parallel over the bases: a lane takes 16 bases of the output, wherever the reads end. */
int kiss_hip_reads_interleave_dev(kiss_hip_ctx *ctx, const uint8_t *codes_a, const uint64_t *index_a, const uint8_t *qual_a, uint64_t P_a,
                                  const uint8_t *codes_b, const uint64_t *index_b, const uint8_t *qual_b, uint64_t P_b, uint8_t *codes,
                                  uint64_t *read_index, uint8_t *qual, uint64_t bases_capacity, uint64_t *bases_out, void *stream);
/* the same with host pointers (the device's cached one-shot context) */
int kiss_hip_reads_interleave_host(const uint8_t *codes_a, const uint64_t *index_a, const uint8_t *qual_a, uint64_t P_a,
                                   const uint8_t *codes_b, const uint64_t *index_b, const uint8_t *qual_b, uint64_t P_b, uint8_t *codes,
                                   uint64_t *read_index, uint8_t *qual, uint64_t bases_capacity, uint64_t *bases_out, int device);

#ifdef __cplusplus
}
#endif
#endif
