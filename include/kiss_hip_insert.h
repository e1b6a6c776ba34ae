/* kiss_hip_insert.h -- the insert size of a paired library, estimated from the pairs on the device (kiss_amd/csrc/fm_insert.hip;
 * DESIGN.md 4.17; the definition restated in tests/fm_insert_model.py).  Declared beside kiss_hip.h, which it includes: the
 * status codes, the ctx, the records and the two promises of a device entry (stream, alignment) are the ones written there.
 *
 * kiss_hip_pair_params carries ins_min, ins_max and ins_mean, and the pair call and the rescue plan take them as given.  This
 * call measures them: it looks at the first hit of either mate of every pair, keeps the pairs that say something about the
 * library, and turns the histogram of their inserts into the three values.  It runs between the select call and the pair call,
 * on what the select call left on the device.  One definition, entirely in integers; all interval arithmetic is signed 64-bit,
 * as in select and pair.  ONLY forward-then-reverse libraries, as in the pair call.
 *
 * THE DEFINITION.
 * Input: hits, hit_index (Q + 1 u64 over the READS, Q even, P = Q / 2), alns and aln_count exactly as in kiss_hip_fmi_pair_dev.
 * Nothing else is read: no text, no reads, no bounds.
 * Parameters (kiss_hip_insert_params, all u32; in parentheses the defaults of Python and the command line): min_mapq (20),
 * max_insert (10000; 1 .. KISS_HIP_INSERT_MAX = 65535), min_samples (25), out_mult (2), map_mult (3), sd_mult (4); the three
 * mults at most 255.
 * SAMPLE.  Only hit number 0 of each mate is looked at: h1 = hits[hit_index[2 p]], h2 = hits[hit_index[2 p + 1]].  Every pair
 * lands in exactly one class; the classes are tested in this order and the first that holds wins:
 *   1. unmapped   : a segment is empty.
 *   2. bad_input  : h1.aln or h2.aln is outside [0, aln_count).  Nothing outside alns is read, whatever the arrays hold.
 *   3. low_mapq   : either mapq is below min_mapq.
 *   4. discordant : the ref fields differ; or the strands (KISS_HIP_HIT_REVERSE) are equal; or either hit has tbeg >= tend; or,
 *                   with f the forward hit and r the reverse one, not (f.tbeg <= r.tbeg and f.tend <= r.tend).
 *   5. too_long   : T = r.tend - f.tbeg > max_insert.
 *   6. otherwise the pair is a SAMPLE of value T, and 1 <= T <= max_insert.
 * So a sample is a pair whose first hits are concordant in the pair call's sense with ins_min = 1 and ins_max = max_insert, and
 * whose two MAPQs pass.  hist[0 .. max_insert], u32: hist[T] = the samples of value T; hist[0] is always 0.
 * STATISTICS, with N = the number of samples:
 *   rank_j = floor(j * N / 4) for j = 1, 2, 3; q_j = the smallest T whose inclusive cumulative count exceeds rank_j -- the
 *   element of 0-based rank rank_j of the sorted samples.  q25, q50, q75 = q_1, q_2, q_3; IQR = q75 - q25.
 *   The USED samples are those with q25 - out_mult * IQR <= T <= q75 + out_mult * IQR; M = their number (M >= 1 when N >= 1),
 *   sum = the sum of T over them.  mean = floor((sum + floor(M / 2)) / M).  dev2 = the sum of (T - mean)^2 over the used
 *   samples (it fits u64: Q is below 2^32 and T below 2^16); var = floor(dev2 / M); sd = the largest integer s with s * s <= var.
 *   ins_min = max(0, min(q25 - map_mult * IQR, mean - sd_mult * sd)); ins_max = max(q75 + map_mult * IQR, mean + sd_mult * sd);
 *   ins_mean = mean.
 * KISS_HIP_INSERT_OK is set in flags iff N >= max(min_samples, 1).  Otherwise every statistic -- used, q25, q50, q75, mean, sd,
 * ins_min, ins_max, ins_mean -- is 0; the class counts, samples and the histogram are still written.
 * Output: the report, and optionally the histogram into the caller's hist, max_insert + 1 u32 on the device (4-byte aligned);
 * with hist == NULL the histogram lives in the ctx's scratch.  The report: P, the five class counts, samples, used, flags, the
 * statistics, the device times.  P = unmapped + bad_input + low_mapq + discordant + too_long + samples.
 * KISS_HIP_E_INVALID: a required pointer NULL (hits, hit_index, alns, params, report), Q odd, a hit_index that decreases (hist
 * then holds no result), a parameter over its limit, max_insert == 0.  KISS_HIP_E_UNSUPPORTED: Q of 2^32 or more,
 * hit_index[Q] of 2^32 - 1 or more -- as the pair call.  Q == 0: KISS_HIP_OK, everything zero, no OK flag.
 * Alignment: hits and alns (read field by field) and hist 4 bytes; hit_index 8 bytes.
 * The call runs on the caller's stream and synchronises it once, to fetch the report's words.
 * The counts are integer sums: the result does not depend on the order in which the pairs are looked at.
 * All addressing is 64-bit.  The kernels also count under KISS_HIP_K_FM_QUERY. */
#ifndef KISS_HIP_INSERT_H
#define KISS_HIP_INSERT_H

#include "kiss_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KISS_HIP_INSERT_MAX 65535u
#define KISS_HIP_INSERT_OK 1u

typedef struct kiss_hip_insert_params { uint32_t min_mapq, max_insert, min_samples, out_mult, map_mult, sd_mult; } kiss_hip_insert_params;

typedef struct kiss_hip_insert_report {
    uint64_t P, unmapped, bad_input, low_mapq, discordant, too_long, samples, used;
    uint32_t flags, q25, q50, q75, mean, sd, ins_min, ins_max, ins_mean;
    /* hist: the arrays zeroed and the pairs looked at; stats: the one workgroup over the bins */
    float ms_total, ms_hist, ms_stats;
} kiss_hip_insert_report;

/* every pointer except params and report is a device pointer; hist may be NULL */
int kiss_hip_fmi_insert_dev(kiss_hip_ctx *ctx, const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                            uint64_t aln_count, const kiss_hip_insert_params *params, uint32_t *hist, kiss_hip_insert_report *report,
                            void *stream);
/* the same with host pointers (the device's cached one-shot context, as kiss_hip_fmi_pair_host); hits holds hit_index[Q]
 * records; hist: max_insert + 1 u32 on the host, or NULL */
int kiss_hip_fmi_insert_host(const kiss_hip_hit *hits, const uint64_t *hit_index, uint64_t Q, const kiss_hip_aln *alns,
                             uint64_t aln_count, const kiss_hip_insert_params *params, uint32_t *hist, kiss_hip_insert_report *report,
                             int device);

#ifdef __cplusplus
}
#endif
#endif
