// bam_markdup.hip -- the duplicate templates of a BAM file marked on the GPU (kiss_hip_bam_markdup_*): FLAG 0x400 on every record
// of a template that repeats the ends of a better one.  The definition is in include/kiss_hip_markdup.h and restated in
// tests/markdup_model.py; DESIGN.md 4.26.
//
//   record : ONE LANE PER RECORD (k_mk_record): the head check of the sort (bs_head), the fixed fields against the record's bytes,
//            the name against the predecessor's name, the cigar (reference length, leading and trailing clips, op codes) and, for a
//            primary record, the qualities that count.  A cigar of up to 8 ops and a qual of up to 256 bytes are the lane's; longer
//            ones are handed to the WHOLE WAVE, record after record (65535 ops: 1024 rounds of one load; a read of 10 000 bases:
//            40 rounds).  Out come the packed end of a mapped primary, the record's score and three bits: starts a template,
//            0x40, 0x80.
//   class  : one lane per record (k_mk_class); the lane of a template's first record walks the records of its template, classes
//            it, keeps its ends and its score at the first record's place and tells every record of it where that is.  It counts
//            the items the template will write -- (ends, pairs) in the two halves of one u64 -- and ONE kiss_scan_u64 places both
//            kinds.  A template is named by its first record: that ascends with the template's number, so ties fall alike.
//   items  : one lane per record (k_mk_items): a fragment writes one end item, a pair two end items and one pair item.
//   sort   : kiss_radix_sort, stable, word after word from the least significant (k_mk_key puts the next word of every item, in
//            the order reached so far, into the ctx's radix arrays): end items by (end, pair before fragment, score descending),
//            pair items by (lo, hi, score descending); the items were written in template order, so the template closes every key.
//            Only the bytes in use are sorted: the ends by the bits of n_ref, the scores by the bits of the largest one; and
//            where an end and a score fit one u64 together they are ONE key and one sort (ends: one sort, pairs: two).
//   heads  : one lane per sorted item: an item whose predecessor has the same key is no head of its run.  A pair item that is
//            none is a duplicate; a fragment's end item that is none has a pair's item or a better fragment in front of it.
//   mark   : one lane per record (k_mk_mark): byte 19 of the record, which holds 0x400, rewritten as a single-byte store where
//            it changes; dup[r].  Nothing else writes to bam, and nothing at all before every check has passed.
//
// ADDRESSING.  As bam_sort.hip: 64-bit offsets from kernel-argument base pointers, 64-bit values cross lanes as two halves, every
// load and store naturally aligned (unaligned fields through bs_word_at, tails byte by byte).  No LDS, no scratch.
#include "bam_record.hpp" // the word reads and the check of a record's head, shared with bam_sort.hip and bai.hip
#include "../../include/kiss_hip_markdup.h"

namespace {

constexpr int MK_THREADS = 256;
constexpr uint32_t MK_LIGHT_OPS = 8;    // a cigar up to here is summed by the record's lane
constexpr uint32_t MK_LIGHT_QUAL = 256; // a qual up to here as well
constexpr uint64_t MK_NO_END = ~0ull;   // (no end packs to it: refID is below 2^30 - 1)
constexpr int64_t MK_U5_BIAS = 1ll << 32;
constexpr uint32_t MK_HEAD = 1u; // bits of a record: starts a template; bits 1 and 2: flag 0x40, 0x80
enum { MK_NOT_FIRST = 0, MK_NONE, MK_FRAGMENT, MK_PAIR, MK_AMBIGUOUS }; // what t_class holds at a record
// control block of a call (u64 words).  MK_BAD and MK_NFIRST (the largest ~r of a bad record r) are touched by a wave that holds
// a bad record, which is rare.  The counts that nearly every wave adds to are kept MK_SHARDS times, a 128-byte line apart, and a
// workgroup adds to the copy of its number: atomics of different waves to ONE address take their turn at the L2 (3.7 * 10^3
// waves with three of them each: 0.28 ms, four times everything else in the kernel); the host adds the copies up.
enum { MK_BAD = 0, MK_NFIRST, MK_HEAD_WORDS = 16 };
enum { MK_TEMPLATES = 0, MK_PAIRS, MK_FRAGMENTS, MK_NONES, MK_AMBIGUOUS_N, MK_MAX_SCORE, MK_DUP_PAIRS, MK_DUP_FRAGMENTS, MK_DUP_RECORDS,
       MK_SHARD_WORDS = 16 };
constexpr int MK_SHARDS = 64;
constexpr int MK_CTL_WORDS = MK_HEAD_WORDS + MK_SHARDS * MK_SHARD_WORDS;
__device__ __forceinline__ unsigned long long *mk_shard(unsigned long long *ctl)
{
    return ctl + MK_HEAD_WORDS + (blockIdx.x & (unsigned)(MK_SHARDS - 1)) * MK_SHARD_WORDS;
}

__device__ __forceinline__ uint64_t mk_wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += bs_lane64(v, (int)(lane_id() ^ (uint32_t)o));
    return v;
}
__device__ __forceinline__ uint64_t mk_wave_max(uint64_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint64_t t = bs_lane64(v, (int)(lane_id() ^ (uint32_t)o));
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t mk_qual1(uint32_t q, uint32_t min_qual) { return q >= min_qual && q != 0xFFu ? q : 0u; }
__device__ __forceinline__ uint32_t mk_qual4(uint32_t w, uint32_t min_qual)
{
    return mk_qual1(w & 0xFFu, min_qual) + mk_qual1(w >> 8 & 0xFFu, min_qual) + mk_qual1(w >> 16 & 0xFFu, min_qual) + mk_qual1(w >> 24, min_qual);
}
__device__ __forceinline__ bool mk_ref_op(uint32_t op) { return ((0x18Du >> op) & 1u) != 0; } // M, D, N, =, X
__device__ __forceinline__ bool mk_clip_op(uint32_t op) { return op == 4u || op == 5u; }      // S, H

// One lane per record: the checks, whether it starts a template, its end, its score
__global__ __launch_bounds__(MK_THREADS) void k_mk_record(const uint8_t *__restrict__ bam, uint64_t bam_bytes, const uint64_t *__restrict__ rec_index,
                                                         uint64_t records, uint32_t n_ref, uint32_t min_qual, uint64_t *__restrict__ rec_end,
                                                         uint64_t *__restrict__ rec_score, uint32_t *__restrict__ rec_bits,
                                                         unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    const uint32_t lane = lane_id();
    const bool live = r < records;
    bool bad = false, ok = false; // ok: the fixed fields fit the record, so that name, cigar and qual may be read
    uint64_t a = 0, size = 0;
    int32_t ref = -1, pos = -1;
    uint32_t l_name = 0, n_ops = 0, flag = 0, l_seq = 0;
    if (live) {
        const BsHead h = bs_head(bam, bam_bytes, rec_index, records, n_ref, r);
        bad = h.bad;
        if (h.read) { // (only then are the 36 bytes there to be read)
            a = h.at, size = h.size, ref = h.ref, pos = h.pos;
            l_name = bs_word_at(bam, a + 12) & 0xFFu;
            const uint32_t w16 = bs_word_at(bam, a + 16);
            n_ops = w16 & 0xFFFFu;
            flag = w16 >> 16;
            l_seq = bs_word_at(bam, a + 20);
            if (l_name == 0) bad = true;
            if (36ull + l_name + 4ull * n_ops + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > size) bad = true;
            ok = !bad;
        }
    }
    const bool primary = ok && (flag & 0x900u) == 0;
    const bool mapped = primary && (flag & 4u) == 0 && ref >= 0;
    const uint64_t name_at = a + 36u, cigar_at = name_at + l_name, qual_at = cigar_at + 4ull * n_ops + ((uint64_t)l_seq + 1) / 2;

    // the name against the predecessor's: the predecessor's fields are checked as far as they are read
    bool head = true;
    if (ok && r > 0) {
        const uint64_t pa = bs_ld64(rec_index + r - 1);
        if (pa < a && a - pa >= KISS_HIP_BAM_RECORD_MIN) { // (a <= bam_bytes: this record was read)
            const uint32_t pl = bs_word_at(bam, pa + 12) & 0xFFu;
            if (pl == l_name && 36ull + pl <= a - pa) {
                bool same = true;
                uint32_t i = 0;
                for (; i + 4 <= l_name && same; i += 4) same = bs_word_at(bam, name_at + i) == bs_word_at(bam, pa + 36u + i);
                for (; i < l_name && same; i++) same = bam[name_at + i] == bam[pa + 36u + i];
                head = !same;
            }
        }
    }

    uint64_t lead = 0, trail = 0, reflen = 0, score = 0;
    bool bad_op = false;
    const bool heavy_c = ok && n_ops > MK_LIGHT_OPS, heavy_q = primary && l_seq > MK_LIGHT_QUAL;
    if (ok && !heavy_c) {
        bool in_lead = true;
        for (uint32_t i = 0; i < n_ops; i++) {
            const uint32_t w = bs_word_at(bam, cigar_at + 4ull * i), op = w & 15u, len = w >> 4;
            bad_op |= op > 8u;
            if (mk_ref_op(op)) reflen += len;
            if (mk_clip_op(op)) {
                if (in_lead) lead += len;
                trail += len;
            } else {
                in_lead = false;
                trail = 0;
            }
        }
    }
    if (primary && !heavy_q) {
        uint32_t i = 0, s = 0;
        for (; i + 4 <= l_seq; i += 4) s += mk_qual4(bs_word_at(bam, qual_at + i), min_qual);
        for (; i < l_seq; i++) s += mk_qual1(bam[qual_at + i], min_qual);
        score = s;
    }
    // the long cigars and long quals of the wave, one record after the other, by all 64 lanes
    unsigned long long heavy = __ballot(heavy_c || heavy_q);
    while (heavy) {
        const int l = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const uint64_t c_at = bs_lane64(cigar_at, l), q_at = bs_lane64(qual_at, l);
        const uint32_t n = (uint32_t)__shfl((int)n_ops, l, 64), L = (uint32_t)__shfl((int)l_seq, l, 64);
        const bool do_c = __shfl((int)heavy_c, l, 64) != 0, do_q = __shfl((int)heavy_q, l, 64) != 0;
        if (do_c) {
            // first: the first op that is no clip (n: none); behind: one past the last such op (0: none)
            uint64_t s = 0, first = n, behind = 0;
            bool bo = false;
            for (uint32_t i = lane; i < n; i += 64) {
                const uint32_t w = bs_word_at(bam, c_at + 4ull * i), op = w & 15u;
                bo |= op > 8u;
                if (mk_ref_op(op)) s += w >> 4;
                if (!mk_clip_op(op)) {
                    first = i < first ? i : first;
                    behind = i + 1;
                }
            }
            s = mk_wave_sum(s);
            first = ~mk_wave_max(~first);
            behind = mk_wave_max(behind);
            const bool any = __ballot(bo) != 0;
            uint64_t ld = 0, tr = 0;
            for (uint64_t i = lane; i < first; i += 64) ld += bs_word_at(bam, c_at + 4ull * i) >> 4;
            for (uint64_t i = behind + lane; i < n; i += 64) tr += bs_word_at(bam, c_at + 4ull * i) >> 4;
            ld = mk_wave_sum(ld);
            tr = mk_wave_sum(tr);
            if ((int)lane == l) reflen = s, lead = ld, trail = tr, bad_op = any;
        }
        if (do_q) {
            uint64_t s = 0;
            for (uint64_t i = 4ull * lane; i < L; i += 256) {
                if (i + 4 <= L) {
                    s += mk_qual4(bs_word_at(bam, q_at + i), min_qual);
                } else {
                    for (uint64_t j = i; j < L; j++) s += mk_qual1(bam[q_at + j], min_qual);
                }
            }
            s = mk_wave_sum(s);
            if ((int)lane == l) score = s;
        }
    }
    if (bad_op) bad = true;
    uint64_t end = MK_NO_END;
    if (mapped && !bad) {
        const uint32_t strand = flag >> 4 & 1u;
        const int64_t u5 = strand ? (int64_t)pos + (int64_t)reflen - 1 + (int64_t)trail : (int64_t)pos - (int64_t)lead;
        if (u5 < -MK_U5_BIAS || u5 >= MK_U5_BIAS) bad = true;
        else end = (uint64_t)(uint32_t)ref << 34 | (uint64_t)(u5 + MK_U5_BIAS) << 1 | strand;
    }
    if (live) {
        rec_end[r] = end;
        rec_score[r] = primary ? score : 0;
        rec_bits[r] = (head ? MK_HEAD : 0u) | (flag >> 6 & 3u) << 1;
        if (bad) atomicMax(&ctl[MK_NFIRST], (unsigned long long)~r);
    }
    const unsigned long long B = __ballot(bad);
    if (lane == 0 && B) atomicAdd(&ctl[MK_BAD], (unsigned long long)__popcll(B));
}

// One lane per record and one behind the last (it closes the array for the scan); the lane of a template's first record works
__global__ __launch_bounds__(MK_THREADS) void k_mk_class(const uint64_t *__restrict__ rec_end, const uint64_t *__restrict__ rec_score,
                                                        const uint32_t *__restrict__ rec_bits, uint64_t records, uint32_t *__restrict__ tmpl_of,
                                                        uint32_t *__restrict__ t_class, uint64_t *__restrict__ t_lo, uint64_t *__restrict__ t_hi,
                                                        uint64_t *__restrict__ t_score, uint64_t *__restrict__ counts, unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    uint32_t cls = MK_NOT_FIRST;
    uint64_t cnt = 0, score = 0;
    if (r < records && (bs_ld32(rec_bits + r) & MK_HEAD)) {
        uint32_t mapped = 0, m0 = 0, m1 = 0;
        uint64_t e0 = 0, e1 = 0, j = r;
        do {
            const uint64_t e = bs_ld64(rec_end + j);
            const uint32_t b = bs_ld32(rec_bits + j);
            score += bs_ld64(rec_score + j);
            if (e != MK_NO_END) {
                if (mapped == 0) e0 = e, m0 = b >> 1 & 3u;
                else if (mapped == 1) e1 = e, m1 = b >> 1 & 3u;
                mapped = mapped < 3 ? mapped + 1 : 3;
            }
            tmpl_of[j] = (uint32_t)r;
            j++;
        } while (j < records && !(bs_ld32(rec_bits + j) & MK_HEAD));
        cls = mapped == 0 ? MK_NONE : mapped == 1 ? MK_FRAGMENT : mapped == 2 && (m0 ^ m1) == 3u && m0 != 0 && m0 != 3u ? MK_PAIR : MK_AMBIGUOUS;
        uint64_t lo = e0, hi = e1;
        if (cls == MK_PAIR && e1 < e0) lo = e1, hi = e0;
        if (cls == MK_FRAGMENT) cnt = 1;
        if (cls == MK_PAIR) cnt = 2 | 1ull << 32;
        t_lo[r] = lo;
        t_hi[r] = hi;
        t_score[r] = score;
    }
    if (r < records) t_class[r] = cls;
    if (r <= records) counts[r] = cnt;
    const uint64_t best = mk_wave_max(cnt ? score : 0);
    const unsigned long long P = __ballot(cls == MK_PAIR), F = __ballot(cls == MK_FRAGMENT), N = __ballot(cls == MK_NONE), A = __ballot(cls == MK_AMBIGUOUS);
    if (lane_id() == 0) {
        unsigned long long *const c = mk_shard(ctl);
        if (P | F | N | A) atomicAdd(&c[MK_TEMPLATES], (unsigned long long)__popcll(P | F | N | A));
        if (P) atomicAdd(&c[MK_PAIRS], (unsigned long long)__popcll(P));
        if (F) atomicAdd(&c[MK_FRAGMENTS], (unsigned long long)__popcll(F));
        if (N) atomicAdd(&c[MK_NONES], (unsigned long long)__popcll(N));
        if (A) atomicAdd(&c[MK_AMBIGUOUS_N], (unsigned long long)__popcll(A));
        if (best > bs_ld64((const uint64_t *)c + MK_MAX_SCORE)) atomicMax(&c[MK_MAX_SCORE], (unsigned long long)best);
    }
}

// the arrays of the items: E end items, P pair items
struct MkItems {
    uint64_t *e_end, *e_w; // the end; 0 for a pair's item, 1 + (the largest score - its score) for a fragment's
    uint32_t *e_tmpl;
    uint64_t *p_lo, *p_hi, *p_w; // the largest score - its score
    uint32_t *p_tmpl;
};

// One lane per record; the first record of a fragment or a pair writes the template's items.  offs: counts, scanned
__global__ __launch_bounds__(MK_THREADS) void k_mk_items(uint64_t records, const uint32_t *__restrict__ t_class, const uint64_t *__restrict__ t_lo,
                                                        const uint64_t *__restrict__ t_hi, const uint64_t *__restrict__ t_score,
                                                        const uint64_t *__restrict__ offs, uint64_t max_score, MkItems it)
{
    const uint64_t r = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    if (r >= records) return;
    const uint32_t cls = bs_ld32(t_class + r);
    if (cls != MK_FRAGMENT && cls != MK_PAIR) return;
    const uint64_t off = bs_ld64(offs + r), e = off & 0xFFFFFFFFull, p = off >> 32;
    const uint64_t w = max_score - bs_ld64(t_score + r);
    it.e_end[e] = bs_ld64(t_lo + r);
    it.e_tmpl[e] = (uint32_t)r;
    if (cls == MK_FRAGMENT) {
        it.e_w[e] = w + 1;
        return;
    }
    it.e_w[e] = 0;
    it.e_end[e + 1] = bs_ld64(t_hi + r);
    it.e_tmpl[e + 1] = (uint32_t)r;
    it.e_w[e + 1] = 0;
    it.p_lo[p] = bs_ld64(t_lo + r);
    it.p_hi[p] = bs_ld64(t_hi + r);
    it.p_w[p] = w;
    it.p_tmpl[p] = (uint32_t)r;
}

// The next word of a sort: key[s] = word[the item in slot s] moved to the top of the u64; with `minor`, a less significant word
// of minor_bits bits that fits below it, both in one key: (word << minor_bits | minor).  order null: the items as they were
// written, and pos is set to them; else order is pos itself, the order that the sorts so far have reached (each lane reads its
// own slot of it and writes its own slot of key)
__global__ __launch_bounds__(MK_THREADS) void k_mk_key(const uint64_t *__restrict__ word, const uint64_t *__restrict__ minor, int minor_bits,
                                                      const uint32_t *order, uint64_t count, int shift, uint64_t *__restrict__ key, uint32_t *pos)
{
    const uint64_t s = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    if (s >= count) return;
    const uint64_t i = order ? (uint64_t)bs_ld32(order + s) : s;
    uint64_t k = bs_ld64(word + i);
    if (minor) k = k << minor_bits | bs_ld64(minor + i);
    key[s] = k << shift;
    if (!order) pos[s] = (uint32_t)s;
}

// One lane per sorted item: an item whose predecessor has its key is a duplicate -- a pair item always, an end item when it is
// a fragment's.  w1: the second word of the key (null: the key is w0 alone)
__global__ __launch_bounds__(MK_THREADS) void k_mk_heads(const uint32_t *__restrict__ sorted, uint64_t count, const uint64_t *__restrict__ w0,
                                                        const uint64_t *__restrict__ w1, const uint32_t *__restrict__ tmpl,
                                                        const uint32_t *__restrict__ t_class, uint32_t *__restrict__ t_dup, int ctl_word,
                                                        unsigned long long *__restrict__ ctl)
{
    const uint64_t s = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    bool dup = false;
    if (s > 0 && s < count) {
        const uint64_t i = bs_ld32(sorted + s), ip = bs_ld32(sorted + s - 1);
        bool same = bs_ld64(w0 + i) == bs_ld64(w0 + ip);
        if (same && w1) same = bs_ld64(w1 + i) == bs_ld64(w1 + ip);
        const uint32_t t = bs_ld32(tmpl + i);
        dup = same && (w1 || bs_ld32(t_class + t) == MK_FRAGMENT);
        if (dup) t_dup[t] = 1u;
    }
    const unsigned long long D = __ballot(dup);
    if (lane_id() == 0 && D) atomicAdd(&mk_shard(ctl)[ctl_word], (unsigned long long)__popcll(D));
}

// One lane per record: the byte that holds 0x400, dup[r]
__global__ __launch_bounds__(MK_THREADS) void k_mk_mark(uint8_t *__restrict__ bam, const uint64_t *__restrict__ rec_index, uint64_t records,
                                                       const uint32_t *__restrict__ tmpl_of, const uint32_t *__restrict__ t_dup, uint8_t *__restrict__ dup,
                                                       unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * MK_THREADS + threadIdx.x;
    bool d = false;
    if (r < records) {
        d = bs_ld32(t_dup + bs_ld32(tmpl_of + r)) != 0;
        uint8_t *const p = bam + bs_ld64(rec_index + r) + 19u; // the high byte of flag
        const uint8_t was = *p, now = d ? (uint8_t)(was | 4u) : (uint8_t)(was & ~4u);
        if (now != was) *p = now;
        if (dup) dup[r] = d ? 1 : 0;
    }
    const unsigned long long D = __ballot(d);
    if (lane_id() == 0 && D) atomicAdd(&mk_shard(ctl)[MK_DUP_RECORDS], (unsigned long long)__popcll(D));
}

struct MarkArgs {
    uint8_t *bam;
    uint64_t bam_bytes;
    const uint64_t *rec_index;
    uint64_t records;
    uint32_t n_ref, min_qual;
    uint8_t *dup;
};

// what needs no device
int mark_args_check(const MarkArgs &a, kiss_hip_markdup_report &rep)
{
    if (!a.rec_index || (a.bam_bytes && !a.bam)) return KISS_HIP_E_INVALID;
    if (a.records == 0 && a.bam_bytes) return KISS_HIP_E_INVALID;
    rep.records = a.records;
    if (a.records > 0xFFFFFFFFull || a.bam_bytes > (1ull << 54) || a.n_ref > KISS_HIP_MARKDUP_MAX_N_REF) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

// the whole bytes that `bits` bits take at the top of a u64: how far a word is moved up
int mk_shift(int bits) { return 64 - (bits + 7) / 8 * 8; }

// One word of a sort (with `minor`: two words that fit one key, `bits` the bits of both): the keys of the items in the order
// reached so far (first: as they were written), sorted.  rb: the order so far is in its buffers [0]; the order reached afterwards
// as well.
int mk_sort_word(kiss_hip_ctx *ctx, RadixBufs &rb, const uint64_t *word, const uint64_t *minor, int minor_bits, uint64_t count, int bits, bool first)
{
    const int shift = mk_shift(bits);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, count);
        hipLaunchKernelGGL(k_mk_key, dim3(fm_grid(count, MK_THREADS)), dim3(MK_THREADS), 0, ctx->stream, word, minor, minor_bits,
                           first ? nullptr : (const uint32_t *)rb.pos[0], count, shift, rb.key[0], rb.pos[0]);
        KCHECK(hipGetLastError());
    }
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, count, shift, 0, &res));
    if (res) {
        uint64_t *const k = rb.key[0];
        uint32_t *const p = rb.pos[0];
        rb.key[0] = rb.key[1], rb.key[1] = k;
        rb.pos[0] = rb.pos[1], rb.pos[1] = p;
    }
    return KISS_HIP_OK;
}

int mark_steps(kiss_hip_ctx *ctx, const MarkArgs &a, kiss_hip_markdup_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t n = a.records;
    if (n == 0) {
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    // the items, never more than the records, are sorted in the ctx's LMS key arrays; their counts are scanned in its scratch
    if (n > ctx->m_cap || (n + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    FmCtl<MK_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_MARKDUP_CTL));
    FmSlab rs, is;
    const uint64_t o_end = rs.carve(n * 8), o_score = rs.carve(n * 8), o_lo = rs.carve(n * 8), o_hi = rs.carve(n * 8), o_tscore = rs.carve(n * 8),
                   o_counts = rs.carve((n + 1) * 8), o_bits = rs.carve(n * 4), o_tmpl = rs.carve(n * 4), o_class = rs.carve(n * 4), o_dup = rs.carve(n * 4);
    const uint64_t half = n / 2 + 1; // a pair has two records or more
    const uint64_t o_eend = is.carve(n * 8), o_ew = is.carve(n * 8), o_plo = is.carve(half * 8), o_phi = is.carve(half * 8), o_pw = is.carve(half * 8),
                   o_etmpl = is.carve(n * 4), o_ptmpl = is.carve(half * 4);
    DevBuf rec, items;
    KTRY(rec.take(ctx, FM_SLOT_MARKDUP_REC, rs.size));
    KTRY(items.take(ctx, FM_SLOT_MARKDUP_ITEMS, is.size));
    uint8_t *const rp = (uint8_t *)rec.p, *const ip = (uint8_t *)items.p;
    uint64_t *const rec_end = (uint64_t *)(rp + o_end), *const rec_score = (uint64_t *)(rp + o_score), *const t_lo = (uint64_t *)(rp + o_lo),
                    *const t_hi = (uint64_t *)(rp + o_hi), *const t_score = (uint64_t *)(rp + o_tscore), *const counts = (uint64_t *)(rp + o_counts);
    uint32_t *const rec_bits = (uint32_t *)(rp + o_bits), *const tmpl_of = (uint32_t *)(rp + o_tmpl), *const t_class = (uint32_t *)(rp + o_class),
                    *const t_dup = (uint32_t *)(rp + o_dup);
    const MkItems it{(uint64_t *)(ip + o_eend), (uint64_t *)(ip + o_ew), (uint32_t *)(ip + o_etmpl), (uint64_t *)(ip + o_plo),
                     (uint64_t *)(ip + o_phi),  (uint64_t *)(ip + o_pw), (uint32_t *)(ip + o_ptmpl)};
    unsigned long long *const h = ctl.h;
    const dim3 threads(MK_THREADS);
    ev.mark(0);
    KTRY(ctl.zero());
    KTRY(kiss_zero_u32(ctx, t_dup, n));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_mk_record, dim3(fm_grid(n, MK_THREADS)), threads, 0, ctx->stream, (const uint8_t *)a.bam, a.bam_bytes, a.rec_index, n, a.n_ref,
                           a.min_qual, rec_end, rec_score, rec_bits, ctl.d);
        KCHECK(hipGetLastError());
    }
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_mk_class, dim3(fm_grid(n + 1, MK_THREADS)), threads, 0, ctx->stream, (const uint64_t *)rec_end, (const uint64_t *)rec_score,
                           (const uint32_t *)rec_bits, n, tmpl_of, t_class, t_lo, t_hi, t_score, counts, ctl.d);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, counts, counts, n + 1));
    uint64_t totals = 0;
    KCHECK(hipMemcpyAsync(&totals, counts + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    KTRY(ctl.fetch_sync());
    rep.ms_record = ev.ms(0, 1);
    if (h[MK_BAD]) {
        rep.bad = h[MK_BAD];
        rep.first_bad = ~h[MK_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    uint64_t max_score = 0;
    for (int shard = 0; shard < MK_SHARDS; shard++) {
        const unsigned long long *const c = h + MK_HEAD_WORDS + shard * MK_SHARD_WORDS;
        rep.templates += c[MK_TEMPLATES];
        rep.pairs += c[MK_PAIRS];
        rep.fragments += c[MK_FRAGMENTS];
        rep.unmapped_templates += c[MK_NONES];
        rep.ambiguous += c[MK_AMBIGUOUS_N];
        max_score = c[MK_MAX_SCORE] > max_score ? c[MK_MAX_SCORE] : max_score;
    }
    const uint64_t E = totals & 0xFFFFFFFFull, P = totals >> 32;
    if (E > n || P > half || E != rep.fragments + 2 * rep.pairs || P != rep.pairs) return KINTERNAL();
    if (E) {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_mk_items, dim3(fm_grid(n, MK_THREADS)), threads, 0, ctx->stream, n, (const uint32_t *)t_class, (const uint64_t *)t_lo,
                           (const uint64_t *)t_hi, (const uint64_t *)t_score, (const uint64_t *)counts, max_score, it);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    const int end_bits = fm_bits(a.n_ref, 30) + 34, score_bits = fm_bits(max_score + 2, 63); // e_w is 0 .. max_score + 1
    const bool fits = end_bits + score_bits <= 64; // an end and a score in one key: one sort, and one histogram pass, fewer
    if (E > 1) {
        RadixBufs rb = kiss_ctx_radix_bufs(ctx);
        if (fits) {
            KTRY(mk_sort_word(ctx, rb, it.e_end, it.e_w, score_bits, E, end_bits + score_bits, true));
        } else {
            KTRY(mk_sort_word(ctx, rb, it.e_w, nullptr, 0, E, score_bits, true));
            KTRY(mk_sort_word(ctx, rb, it.e_end, nullptr, 0, E, end_bits, false));
        }
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, E);
        hipLaunchKernelGGL(k_mk_heads, dim3(fm_grid(E, MK_THREADS)), threads, 0, ctx->stream, (const uint32_t *)rb.pos[0], E, (const uint64_t *)it.e_end,
                           (const uint64_t *)nullptr, (const uint32_t *)it.e_tmpl, (const uint32_t *)t_class, t_dup, (int)MK_DUP_FRAGMENTS, ctl.d);
        KCHECK(hipGetLastError());
    }
    if (P > 1) {
        RadixBufs rb = kiss_ctx_radix_bufs(ctx);
        if (fits) {
            KTRY(mk_sort_word(ctx, rb, it.p_hi, it.p_w, score_bits, P, end_bits + score_bits, true));
        } else {
            KTRY(mk_sort_word(ctx, rb, it.p_w, nullptr, 0, P, score_bits, true));
            KTRY(mk_sort_word(ctx, rb, it.p_hi, nullptr, 0, P, end_bits, false));
        }
        KTRY(mk_sort_word(ctx, rb, it.p_lo, nullptr, 0, P, end_bits, false));
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, P);
        hipLaunchKernelGGL(k_mk_heads, dim3(fm_grid(P, MK_THREADS)), threads, 0, ctx->stream, (const uint32_t *)rb.pos[0], P, (const uint64_t *)it.p_lo,
                           (const uint64_t *)it.p_hi, (const uint32_t *)it.p_tmpl, (const uint32_t *)t_class, t_dup, (int)MK_DUP_PAIRS, ctl.d);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_mk_mark, dim3(fm_grid(n, MK_THREADS)), threads, 0, ctx->stream, a.bam, a.rec_index, n, (const uint32_t *)tmpl_of,
                           (const uint32_t *)t_dup, a.dup, ctl.d);
        KCHECK(hipGetLastError());
    }
    ev.mark(4);
    KTRY(ctl.fetch());
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    for (int shard = 0; shard < MK_SHARDS; shard++) {
        const unsigned long long *const c = h + MK_HEAD_WORDS + shard * MK_SHARD_WORDS;
        rep.dup_pairs += c[MK_DUP_PAIRS];
        rep.dup_fragments += c[MK_DUP_FRAGMENTS];
        rep.dup_records += c[MK_DUP_RECORDS];
    }
    rep.ms_class = ev.ms(1, 2);
    rep.ms_sort = ev.ms(2, 3);
    rep.ms_mark = ev.ms(3, 4);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_bam_markdup_dev(kiss_hip_ctx *ctx, uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                             uint32_t n_ref, uint32_t min_qual, uint8_t *dup, kiss_hip_markdup_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_markdup_report rep{};
    if (report) *report = rep;
    const MarkArgs a{bam, bam_bytes, rec_index, records, n_ref, min_qual, dup};
    int rc = mark_args_check(a, rep);
    if (report) *report = rep;
    if (rc) return rc;
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    rc = mark_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_bam_markdup_host(uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                              uint32_t min_qual, uint8_t *dup, kiss_hip_markdup_report *report, int device)
{
    kiss_hip_markdup_report rep{};
    const MarkArgs a{bam, bam_bytes, rec_index, records, n_ref, min_qual, dup};
    const int rc0 = mark_args_check(a, rep);
    if (report) *report = rep;
    if (rc0) return rc0;
    if (records == 0) return KISS_HIP_OK;
    return kiss_one_shot_cached(device, fm_host_max_n(0, records + 1), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        uint8_t *dbam = const_cast<uint8_t *>(st.up((const uint8_t *)bam, bam_bytes));
        const uint64_t *dri = st.up(rec_index, (records + 1) * 8);
        uint8_t *ddup = st.room<uint8_t>(dup != nullptr, records);
        if (st.rc) return st.rc;
        const int rc = kiss_hip_bam_markdup_dev(ctx, dbam, bam_bytes, dri, records, n_ref, min_qual, ddup, report, nullptr);
        if (rc) return rc;
        st.down(bam, dbam, bam_bytes);
        if (dup) st.down(dup, ddup, records);
        return st.rc;
    });
}

} // extern "C"
