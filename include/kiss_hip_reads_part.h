/* kiss_hip_reads_part.h -- a read file parsed in batches: the first whole records of a CHUNK of the file, and how many bytes they
 * took (kiss_amd/csrc/reads.hip; the definition restated in tests/reads_part_model.py).  Declared beside
 * kiss_hip_reads.h, which it includes: lines, the '\r' strip, codes, names, bad kinds, the size-then-fill protocol, the limits and
 * the KISS_HIP_E_* answers are the parse call's.  The two entries are kiss_hip_reads_parse_dev / _host plus `final` and
 * `max_records`.
 *
 * COMPLETE LINES.  final != 0: the chunk is the end of the file; its complete lines are the lines of the parse definition.
 * final == 0: only lines ended by a '\n' inside the chunk are complete; the piece behind the last '\n' is not.
 *   KISS_HIP_READS_FASTQ : kept = the number of complete lines up to the last one that is not empty after the strip, final or not:
 *                          lines that are empty so far are never consumed early (four blank lines are no record).
 *                          records_complete = ceil(kept / 4) with final (a truncated last record counts, so that the parse
 *                          refuses it as kind 4), floor(kept / 4) without.
 *                          records = records_complete, or min(max_records, records_complete) when max_records > 0.
 *                          final and records == records_complete: bytes_used = bytes, and the prefix is parsed as the parse call
 *                          parses a file (trailing empty lines are dropped).  Otherwise bytes_used is the offset behind the '\n'
 *                          of line 4 records - 1 (0 when records is 0), and the prefix is parsed with roles by line number and NO
 *                          LINE DROPPED: an empty quality line that ends the prefix belongs to an empty read, as it would in the
 *                          whole file.
 *   KISS_HIP_READS_LINES : a record is a read line.  bytes_used is the offset behind the '\n' of read line number `records` (0
 *                          when records is 0), so a '>' line at the end of the chunk is never parted from its read; final and
 *                          records == records_complete: bytes_used = bytes.
 *   KISS_HIP_READS_AUTO  : looks at the first byte of the CHUNK.  A caller resolves the format on the first chunk (the report
 *                          names it) and passes it afterwards.
 * READING ON.  records == 0 and bytes_used == 0 without final: the caller needs a longer chunk.  Otherwise the next chunk starts
 * at bytes_used.  Name spans are offsets into the chunk; a span of length 0 stands for the decimal number of the read IN THE
 * FILE: the caller adds the records consumed before.  first_bad is relative to the chunk.
 * THE PROPERTY.  For every byte string and every way to feed it -- any chunk size, any max_records, the unused tail carried in
 * front of the next chunk, final on the last one -- the batches, concatenated, are the parse of the whole file: codes,
 * qualities, index, names, empty_reads.  If the file has bad records, the first failing batch reports the whole file's first_bad
 * (once the records before it are added) and first_bad_kind.
 *
 * Report: `parsed` is the kiss_hip_reads_report of the prefix (lines: those of the prefix; with final and every record taken, of
 * the chunk); records_complete, records and bytes_used are filled whenever the call got as far as looking at the chunk, a prefix
 * with bad records and a capacity too small among them.  ms_total and ms_lines of `parsed` include the passes that find the cut.
 * Nothing is read outside [d_raw, d_raw + bytes); nothing is written behind a capacity. */
#ifndef KISS_HIP_READS_PART_H
#define KISS_HIP_READS_PART_H

#include "kiss_hip_reads.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kiss_hip_reads_part_report {
    kiss_hip_reads_report parsed;
    uint64_t records_complete, records, bytes_used;
} kiss_hip_reads_part_report;

int kiss_hip_reads_parse_part_dev(kiss_hip_ctx *ctx, const uint8_t *d_raw, uint64_t bytes, int format, int final, uint64_t max_records,
                                  uint8_t *d_codes, uint8_t *d_qual, uint64_t bases_capacity, uint64_t *d_read_index, uint64_t *d_name_off,
                                  uint32_t *d_name_len, uint64_t reads_capacity, kiss_hip_reads_part_report *report, void *stream);
/* the same with host pointers (the device's cached one-shot context); name_off / name_len are spans into raw */
int kiss_hip_reads_parse_part_host(const uint8_t *raw, uint64_t bytes, int format, int final, uint64_t max_records, uint8_t *codes,
                                   uint8_t *qual, uint64_t bases_capacity, uint64_t *read_index, uint64_t *name_off, uint32_t *name_len,
                                   uint64_t reads_capacity, kiss_hip_reads_part_report *report, int device);

#ifdef __cplusplus
}
#endif
#endif
