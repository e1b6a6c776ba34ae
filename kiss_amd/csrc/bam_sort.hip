// bam_sort.hip -- the BAM records of a file put into coordinate order on the GPU (kiss_hip_bam_sort_*).  The definition is in
// include/kiss_hip_bam_sort.h and restated in tests/bam_sort_model.py; DESIGN.md 4.24.
//
//   key    : ONE LANE PER RECORD (k_bam_sort_key): its two index entries, the three words of its head read from naturally aligned
//            words, every check of the header, and (key, r) into the ctx's radix arrays.  key = (rk << 32 | pos + 1) moved to the
//            top of the u64, so that the sort runs only the 5 .. 8 byte passes that the bits of n_ref ask for.
//   sort   : kiss_radix_sort, stable, on those arrays (as fm_select.hip uses it).
//   sizes  : one lane per sorted slot (k_bam_sort_sizes): the bytes of record order[s]; kiss_scan_u64 makes the sorted CSR of them.
//   gather : ONE WAVE PER 2048 DESTINATION BYTES (k_bam_gather), a granule that starts on a 4-byte boundary of the destination's
//            ADDRESS.  The wave finds the record that holds its first byte by a 64-ary search in the sorted CSR (the lanes probe 64
//            places at once: three steps for 2^18 records), then lane l keeps the start, in the destination and in the source, of
//            record first + l: a granule meets at most 2048 / 36 + 2 = 58 records, since a record has 36 bytes or more, and
//            their 59 boundaries fit the wave.  Lane l then owns the words l, l + 64, .. of the granule.  A word that lies inside
//            one record is stored whole, funnelled from the one or two aligned source words that hold its bytes; the words at
//            the ends of the output and the words that two records share are written byte by byte.  So the cost of a byte does
//            not depend on the record it belongs to: a record of 300 000 bytes is copied by 147 waves, not by one.
//            (The other way, one wave per record and long records cut up, needs a list of the pieces and a second kind of wave.)
//
// ADDRESSING.  As fm_bam.hip: every address is a kernel-argument base pointer plus a 64-bit offset, and 64-bit values cross lanes
// as two unsigned halves.  Every load and store is naturally aligned.  No LDS, no scratch.
#include "bam_record.hpp" // the word reads and the check of a record's head, shared with bai.hip

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_WAVES = BS_THREADS / 64;
constexpr uint32_t BS_GRANULE = 2048;                 // destination bytes of one wave
constexpr uint32_t BS_WORDS_PER_LANE = BS_GRANULE / 4 / 64;
static_assert(BS_GRANULE / KISS_HIP_BAM_RECORD_MIN + 2 + 1 <= 64, "the boundaries of the records of a granule fit one wave");
// control block of a call (u64 words); BS_NFIRST holds the largest ~r of a bad record r (the words start at 0)
enum { BS_BAD = 0, BS_NFIRST = 1, BS_UNPLACED = 2, BS_LONGEST = 3, BS_CTL_WORDS = 4 };

// One lane per record: the checks, the key.  size[] is not kept: the sizes are read again in sorted order.
__global__ __launch_bounds__(BS_THREADS) void k_bam_sort_key(const uint8_t *__restrict__ bam, uint64_t bam_bytes, const uint64_t *__restrict__ rec_index,
                                                           uint64_t records, uint32_t n_ref, int key_shift, uint64_t *__restrict__ key,
                                                           uint32_t *__restrict__ pos, unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    bool bad = false, unplaced = false;
    uint64_t size = 0;
    if (r < records) {
        const BsHead h = bs_head(bam, bam_bytes, rec_index, records, n_ref, r);
        bad = h.bad;
        uint64_t k = ~0ull;
        if (h.read) {
            size = h.size;
            unplaced = h.ref == -1;
            const uint64_t rk = unplaced ? (uint64_t)n_ref : (uint64_t)(uint32_t)h.ref;
            k = (rk << 32 | (uint64_t)(uint32_t)(h.pos + 1)) << key_shift;
        }
        key[r] = k;
        pos[r] = (uint32_t)r;
        if (bad) atomicMax(&ctl[BS_NFIRST], (unsigned long long)~r);
    }
    if (bad) size = 0, unplaced = false;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint64_t t = bs_lane64(size, (int)(lane_id() ^ (uint32_t)o));
        size = t > size ? t : size;
    }
    const unsigned long long B = __ballot(bad), U = __ballot(unplaced);
    if (lane_id() == 0) {
        if (B) atomicAdd(&ctl[BS_BAD], (unsigned long long)__popcll(B));
        if (U) atomicAdd(&ctl[BS_UNPLACED], (unsigned long long)__popcll(U));
        if (size > bs_ld64((const uint64_t *)ctl + BS_LONGEST)) atomicMax(&ctl[BS_LONGEST], (unsigned long long)size);
    }
}

// One lane per sorted slot: the bytes of the record that goes there (size[records] = 0 closes the array for the scan)
__global__ __launch_bounds__(BS_THREADS) void k_bam_sort_sizes(const uint64_t *__restrict__ rec_index, const uint32_t *__restrict__ sorted,
                                                             uint64_t records, uint64_t *__restrict__ size)
{
    const uint64_t s = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    if (s > records) return;
    uint64_t v = 0;
    if (s < records) {
        const uint64_t r = bs_ld32(sorted + s);
        v = bs_ld64(rec_index + r + 1) - bs_ld64(rec_index + r);
    }
    size[s] = v;
}

// the caller's copies of the sorted CSR and of the permutation (either may be null)
__global__ __launch_bounds__(BS_THREADS) void k_bam_sort_index(const uint64_t *__restrict__ sidx, const uint32_t *__restrict__ sorted, uint64_t records,
                                                             uint64_t *__restrict__ out_index, uint32_t *__restrict__ order)
{
    const uint64_t s = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    if (s > records) return;
    if (out_index) out_index[s] = bs_ld64(sidx + s);
    if (order && s < records) order[s] = bs_ld32(sorted + s);
}

// One wave per granule of the destination (the head of this file has the plan).  sidx: the sorted CSR, records + 1 entries,
// sidx[records] = total.
__global__ __launch_bounds__(BS_THREADS) void k_bam_gather(const uint8_t *__restrict__ bam, const uint64_t *__restrict__ rec_index,
                                                         const uint32_t *__restrict__ sorted, const uint64_t *__restrict__ sidx, uint64_t records,
                                                         uint64_t total, uint8_t *__restrict__ out)
{
    const uint32_t lane = lane_id();
    const uint64_t g = (uint64_t)blockIdx.x * BS_WAVES + (threadIdx.x >> 6);
    const uint32_t lead = (uint32_t)((uintptr_t)out & 3u); // the granules start `lead` bytes in front of out: on a word of its address
    // offsets into out, as signed values: the first granule starts at -lead
    const int64_t o_first = (int64_t)(g * BS_GRANULE) - (int64_t)lead;
    const int64_t o_lo = o_first < 0 ? 0 : o_first;
    const int64_t o_hi = o_first + (int64_t)BS_GRANULE < (int64_t)total ? o_first + (int64_t)BS_GRANULE : (int64_t)total;
    if (o_lo >= o_hi) return; // (uniform over the wave)

    // the last record s with sidx[s] <= o_lo: sidx[lo] <= o_lo < sidx[hi] throughout (sidx[0] = 0, sidx[records] = total > o_lo)
    uint64_t lo = 0, hi = records;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t p = lo + (uint64_t)(lane + 1) * step;
        const bool le = p < hi && bs_ld64(sidx + p) <= (uint64_t)o_lo;
        const uint64_t c = (uint64_t)__popcll(__ballot(le)); // (the probes ascend: the lanes that say yes are the first c)
        const uint64_t nlo = lo + c * step, nhi = lo + (c + 1) * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    // lane l: where record lo + l starts in the destination (st) and in the source (src); the lane behind the last record has the total
    const uint64_t k = lo + lane;
    uint64_t st = ~0ull >> 1, src = 0;
    if (k <= records) st = bs_ld64(sidx + k);
    if (k < records) src = bs_ld64(rec_index + bs_ld32(sorted + k));
    const int nrec = __popcll(__ballot(k < records && (int64_t)st < o_hi)); // the records that meet the granule: 1 .. 58
    // rel: the start of record lo + l as an offset into the granule, for the compares below (anything behind the granule: its end)
    const int64_t d = (int64_t)st - o_first;
    const int32_t rel = d > (int64_t)BS_GRANULE ? (int32_t)BS_GRANULE : (int32_t)d; // (lane 0 may start far in front: it is never compared)

    // which record holds the first byte of each of this lane's words
    int idx[BS_WORDS_PER_LANE];
#pragma unroll
    for (uint32_t t = 0; t < BS_WORDS_PER_LANE; t++) idx[t] = 0;
    for (int l = 1; l < nrec; l++) {
        const int32_t rl = __shfl(rel, l, 64);
#pragma unroll
        for (uint32_t t = 0; t < BS_WORDS_PER_LANE; t++) idx[t] += rl <= (int32_t)(4u * (lane + 64u * t)) ? 1 : 0;
    }
#pragma unroll
    for (uint32_t t = 0; t < BS_WORDS_PER_LANE; t++) {
        const int64_t o = o_first + (int64_t)(4u * (lane + 64u * t)); // the word's offset into out: its address is a multiple of 4
        // (every lane takes part in the exchanges, whatever it does with the answers)
        const uint64_t r_st = bs_lane64(st, idx[t]), r_end = bs_lane64(st, idx[t] + 1);
        const uint64_t r_src = bs_lane64(src, idx[t]), n_src = bs_lane64(src, idx[t] + 1);
        if (o >= o_hi || o + 4 <= o_lo) continue;
        if ((int64_t)r_st <= o && o + 4 <= (int64_t)r_end) { // the whole word is this record's (and inside the output: r_end <= total)
            const uint32_t v = bs_word_at(bam, r_src + ((uint64_t)o - r_st));
            *(uint32_t *)(out + o) = v;
        } else { // a word at either end of the output, or one that the next record shares (36 bytes or more: no third one)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int64_t ob = o + b;
                if (ob < o_lo || ob >= o_hi) continue;
                const bool mine = (uint64_t)ob < r_end;
                const uint64_t from = mine ? r_src + ((uint64_t)ob - r_st) : n_src + ((uint64_t)ob - r_end);
                out[ob] = bam[from];
            }
        }
    }
}

struct SortArgs {
    const uint8_t *bam;
    uint64_t bam_bytes;
    const uint64_t *rec_index;
    uint64_t records;
    uint32_t n_ref;
    uint8_t *out;
    uint64_t out_capacity;
    uint64_t *out_index;
    uint32_t *order;
};

// what needs no device; the totals go into the report whatever follows
int sort_args_check(const SortArgs &a, kiss_hip_bam_sort_report &rep)
{
    if (!a.rec_index || (a.bam_bytes && !a.bam) || (a.out_capacity && !a.out)) return KISS_HIP_E_INVALID;
    if (a.records == 0 && a.bam_bytes) return KISS_HIP_E_INVALID;
    rep.records = a.records;
    rep.bam_bytes = a.bam_bytes;
    if (a.out_capacity < a.bam_bytes) return KISS_HIP_E_INVALID; // (the totals are in the report)
    if (a.records > 0xFFFFFFFFull || a.bam_bytes > (1ull << 62)) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int sort_steps(kiss_hip_ctx *ctx, const SortArgs &a, kiss_hip_bam_sort_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t n = a.records;
    if (n == 0) { // out_index[0] = 0
        if (a.out_index) KTRY(kiss_zero_u32(ctx, a.out_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    // one call: its records are sorted in the ctx's LMS key arrays and their sizes scanned in its scratch
    if (n > ctx->m_cap || (n + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    const int key_bits = fm_bits((uint64_t)a.n_ref + 1, 32) + 32; // rk is 0 .. n_ref, pos + 1 is 0 .. 2^31
    const int key_shift = 64 - (key_bits + 7) / 8 * 8;            // the sort takes whole bytes from the top of the key
    FmCtl<BS_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_BAM_SORT_CTL));
    DevBuf index;
    KTRY(index.take(ctx, FM_SLOT_BAM_SORT_INDEX, (n + 1) * 8));
    uint64_t *const sidx = (uint64_t *)index.p; // the sizes in sorted order, scanned in place
    unsigned long long *const h = ctl.h;
    const dim3 threads(BS_THREADS);
    ev.mark(0);
    KTRY(ctl.zero());
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_bam_sort_key, dim3(fm_grid(n, BS_THREADS)), threads, 0, ctx->stream, a.bam, a.bam_bytes, a.rec_index, n, a.n_ref, key_shift,
                           ctx->keyA, ctx->posA, ctl.d);
        KCHECK(hipGetLastError());
    }
    ev.mark(1);
    KTRY(ctl.fetch_sync());
    rep.ms_key = ev.ms(0, 1);
    if (h[BS_BAD]) {
        rep.bad = h[BS_BAD];
        rep.first_bad = ~h[BS_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    rep.unplaced = h[BS_UNPLACED];
    rep.longest = h[BS_LONGEST];
    RadixBufs rb = kiss_ctx_radix_bufs(ctx);
    int res = 0;
    KTRY(kiss_radix_sort(ctx, rb, n, key_shift, 0, &res));
    const uint32_t *const sorted = rb.pos[res];
    ev.mark(2);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_bam_sort_sizes, dim3(fm_grid(n + 1, BS_THREADS)), threads, 0, ctx->stream, a.rec_index, sorted, n, sidx);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, sidx, sidx, n + 1));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, a.bam_bytes);
        if (a.out_index || a.order)
            hipLaunchKernelGGL(k_bam_sort_index, dim3(fm_grid(n + 1, BS_THREADS)), threads, 0, ctx->stream, (const uint64_t *)sidx, sorted, n, a.out_index,
                               a.order);
        const uint64_t granules = div_up(a.bam_bytes + 3, BS_GRANULE); // (up to three bytes of lead in front of out)
        const uint64_t blocks = div_up(granules, BS_WAVES);
        if (blocks > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
        hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)blocks), threads, 0, ctx->stream, a.bam, a.rec_index, sorted, (const uint64_t *)sidx, n,
                           a.bam_bytes, a.out);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    rep.ms_sort = ev.ms(1, 2);
    rep.ms_copy = ev.ms(2, 3);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_bam_sort_dev(kiss_hip_ctx *ctx, const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                          uint32_t n_ref, uint8_t *out, uint64_t out_capacity, uint64_t *out_index, uint32_t *order,
                          kiss_hip_bam_sort_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_bam_sort_report rep{};
    if (report) *report = rep;
    const SortArgs a{bam, bam_bytes, rec_index, records, n_ref, out, out_capacity, out_index, order};
    int rc = sort_args_check(a, rep);
    if (report) *report = rep;
    if (rc) return rc;
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    rc = sort_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_bam_sort_host(const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                           uint8_t *out, uint64_t out_capacity, uint64_t *out_index, uint32_t *order,
                           kiss_hip_bam_sort_report *report, int device)
{
    kiss_hip_bam_sort_report rep{};
    const SortArgs a{bam, bam_bytes, rec_index, records, n_ref, out, out_capacity, out_index, order};
    const int rc0 = sort_args_check(a, rep);
    if (report) *report = rep;
    if (rc0) return rc0;
    if (records == 0) {
        if (out_index) out_index[0] = 0;
        return KISS_HIP_OK;
    }
    return kiss_one_shot_cached(device, fm_host_max_n(0, records + 1), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *dbam = st.up(bam, bam_bytes);
        const uint64_t *dri = st.up(rec_index, (records + 1) * 8);
        uint8_t *dout = st.room<uint8_t>(true, bam_bytes);
        uint64_t *doi = st.room<uint64_t>(out_index != nullptr, (records + 1) * 8);
        uint32_t *dord = st.room<uint32_t>(order != nullptr, records * 4);
        if (st.rc) return st.rc;
        const int rc = kiss_hip_bam_sort_dev(ctx, dbam, bam_bytes, dri, records, n_ref, dout, bam_bytes, doi, dord, report, nullptr);
        if (rc) return rc;
        st.down(out, dout, bam_bytes);
        if (out_index) st.down(out_index, doi, (records + 1) * 8);
        if (order) st.down(order, dord, records * 4);
        return st.rc;
    });
}

} // extern "C"
