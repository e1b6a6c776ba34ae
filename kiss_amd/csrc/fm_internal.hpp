// fm_internal.hpp -- what the translation units of the batch calls share: the FM-index ones (fm.hip: exact queries +
// construction; fm_mm.hip: the search with mismatches; fm8.hip: the byte alphabet; fm_seed.hip: maximal exact match seeds;
// fm_chain.hip: chains of seeds; fm_align.hip: banded alignment of the chains; fm_select.hip: the mappings of a read;
// fm_pair.hip: the mappings of two mates; fm_rescue.hip: the missing mate, two alignment sets merged) and reads.hip, the read
// files; general.hip takes the staging of its one-shot entry from here.  Device side: the device view of an index, the
// one-sector rank blocks and the LF arithmetic on them, the rank of the sampling bit-vector, the bounded locate walk of one
// row.  Host side, the frame around a _dev call: the pooled scratch buffers (DevBuf, slots named by FmSlot in
// kiss_internal.hpp), the events behind a report's times (FmEvents), the prologue and epilogue (fm_enter / fm_leave), the
// control words of a call with their host mirror (FmCtl), the small arithmetic (fm_up256, fm_bits, fm_grid, FmSlab).  And the
// frame around a _host call, which runs its _dev twin on a one-shot ctx (kiss_one_shot_own / kiss_one_shot_cached in
// kiss_internal.hpp): the checked copies (fm_h2d / fm_d2h), the arrays of the call on the device (FmStage: up, room, down),
// a DNA index uploaded through it (fm_upload_index), the ascending check of an index array and the size of the ctx
// (fm_host_max_n).
#pragma once
#include "kiss_internal.hpp"

struct FmiD {
    uint64_t N;
    uint32_t cnt[4];
    uint32_t pri;
    uint64_t bwt_bytes;
    const uint8_t *bwt;
    const uint32_t *occ1;
    const uint8_t *occ2;
    const uint32_t *sa;
    const uint64_t *b;
    const uint32_t *b_occ;
    const uint4 *blk; // interleaved rank blocks: [2 * j] = counts of A, C, G, T in bwt[0, 64 j), [2 * j + 1] = the 64 dibits
};

// one 32-byte block: counts before the block + the block's dibits
struct FmBlock {
    uint4 cnt;
    uint4 bw; // dibit t of the block at bits 2 (t % 16) of word t / 16
};
__device__ __forceinline__ FmBlock fm_block(const FmiD &f, uint64_t j)
{
    FmBlock b;
    b.cnt = f.blk[2 * j];
    b.bw = f.blk[2 * j + 1];
    return b;
}
// occ(c, i) for a row i of block j = i / 64 (the block already loaded): the same sum as compute_occ with the block start in
// the place of the 16-row chunk start -- counts before the block + matching dibits in [64 j, i) - the primary row's
// placeholder 'A' when it lies in that stretch
__device__ __forceinline__ uint32_t fm_occ_in(const FmiD &f, const FmBlock &b, uint32_t c, uint64_t i)
{
    const uint32_t r = (uint32_t)(i & 63u);
    const uint32_t pat = c * 0x55555555u;
    const uint32_t w[4] = {b.bw.x, b.bw.y, b.bw.z, b.bw.w};
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) {
        const uint32_t x = w[t] ^ pat;
        uint32_t m = ~(x | (x >> 1)) & 0x55555555u; // bit 2 u set <=> dibit u of this word == c
        const int left = (int)r - (int)(16 * t);     // rows of this word below i
        m = left >= 16 ? m : (left <= 0 ? 0u : (m & ((1u << (2 * left)) - 1u)));
        cnt += (uint32_t)__popc(m);
    }
    const uint32_t base = c == 0 ? b.cnt.x : (c == 1 ? b.cnt.y : (c == 2 ? b.cnt.z : b.cnt.w));
    const uint64_t start = i & ~63ull;
    const uint32_t pass_pri = (c == 0 && start <= f.pri && f.pri < i) ? 1u : 0u;
    return base + cnt - pass_pri;
}
__device__ __forceinline__ uint32_t fm_occ(const FmiD &f, uint32_t c, uint64_t i)
{
    return fm_occ_in(f, fm_block(f, i >> 6), c, i);
}
__device__ __forceinline__ uint64_t fm_lf(const FmiD &f, uint32_t c, uint64_t i) { return (uint64_t)f.cnt[c] + fm_occ(f, c, i); }
// both ends of a range: one block load when they fall into the same 64 rows (the usual case once the range is narrow)
__device__ __forceinline__ void fm_lf2(const FmiD &f, uint32_t c, uint64_t &beg, uint64_t &end)
{
    const uint64_t jb = beg >> 6, je = end >> 6;
    const FmBlock bb = fm_block(f, jb);
    const uint32_t ob = fm_occ_in(f, bb, c, beg);
    const uint32_t oe = je == jb ? fm_occ_in(f, bb, c, end) : fm_occ_in(f, fm_block(f, je), c, end);
    beg = (uint64_t)f.cnt[c] + ob;
    end = (uint64_t)f.cnt[c] + oe;
}

__device__ __forceinline__ uint32_t fm_bwt(const FmiD &f, uint64_t i)
{
    return ((uint32_t)f.bwt[i >> 2] >> (2 * (uint32_t)(i & 3))) & 3u;
}

// compute_b_occ, fm_index.hpp:189-208.  SA_INTV = 1 keeps no bit-vector (b == nullptr): every row is sampled and its
// rank is the row itself, so the walk below emits sa_[beg, end) at depth 0 -- get_offsets' span (:455-456)
// (the arrays alone: fm8.hip keeps the same bit-vector beside another kind of index)
__device__ __forceinline__ uint32_t fm_b_rank(const uint64_t *__restrict__ b, const uint32_t *__restrict__ b_occ, uint64_t i)
{
    if (!b) return (uint32_t)i;
    const uint64_t w = i >> 6;
    const uint32_t r = (uint32_t)(i & 63);
    uint32_t c = b_occ[w];
    if (r) c += (uint32_t)__popcll(b[w] & ((1ull << r) - 1ull));
    return c;
}
__device__ __forceinline__ uint32_t fm_b_occ(const FmiD &f, uint64_t i) { return fm_b_rank(f.b, f.b_occ, i); }

// The locate walk of one SA row: LF to a sampled row -- at most sa_intv - 1 steps and never from the primary row (its BWT
// symbol is a placeholder), so the walk is bounded whatever arrays it is handed.  false: no sampled row inside the bound (an
// index that was not built from an exact suffix array); position is then 0xFFFFFFFF.
__device__ __forceinline__ bool fm_locate_row(const FmiD &f, uint32_t sa_intv, uint64_t sa_entries, uint64_t row,
                                              uint32_t &position)
{
    position = 0xFFFFFFFFu;
    for (uint32_t step = 0; step < sa_intv && row < f.N; step++) {
        const bool sampled = !f.b || ((f.b[row >> 6] >> (row & 63u)) & 1ull);
        if (sampled) {
            const uint64_t r = fm_b_occ(f, row);
            if (r >= sa_entries) return false;
            position = f.sa[r] + step;
            return true;
        }
        if (row == f.pri || step + 1 == sa_intv) break;
        row = fm_lf(f, fm_bwt(f, row), row);
    }
    return false;
}

// the device view of the arrays of a kiss_hip_fmi_view (blk is filled in by the caller: kiss_fm_make_blocks)
static inline FmiD fm_view_of(const kiss_hip_fmi_view *fmi)
{
    FmiD f;
    f.N = fmi->n_sa;
    for (int c = 0; c < 4; c++) f.cnt[c] = fmi->cnt[c];
    f.pri = fmi->pri;
    f.bwt_bytes = (fmi->n_sa + 3) / 4;
    f.bwt = fmi->bwt;
    f.occ1 = fmi->occ1;
    f.occ2 = fmi->occ2;
    f.sa = fmi->sa;
    f.b = fmi->sa_intv == 1 ? nullptr : fmi->b;
    f.b_occ = fmi->b_occ;
    f.blk = nullptr;
    return f;
}

struct DevBuf {
    void *p = nullptr;
    bool pooled = false;
    ~DevBuf()
    {
        if (p && !pooled) (void)hipFree(p);
    }
    int alloc(kiss_hip_ctx *ctx, uint64_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) {
            ctx->last_hip_error = (int)e;
            p = nullptr;
            return KISS_HIP_E_NOMEM;
        }
        return KISS_HIP_OK;
    }
    // scratch of the batched query: kept in the ctx between calls (slot = fixed role), regrown when too small --
    // nine hipMalloc / hipFree pairs per batch cost as much as the kernels
    int take(kiss_hip_ctx *ctx, FmSlot slot, uint64_t bytes)
    {
        pooled = true;
        if (ctx->fm_pool_cap[slot] < bytes) {
            if (ctx->fm_pool[slot]) (void)hipFree(ctx->fm_pool[slot]);
            ctx->fm_pool[slot] = nullptr;
            ctx->fm_pool_cap[slot] = 0;
            const uint64_t want = bytes + bytes / 8 + 256;
            hipError_t e = hipMalloc(&ctx->fm_pool[slot], want);
            if (e != hipSuccess) {
                ctx->last_hip_error = (int)e;
                ctx->fm_pool[slot] = nullptr;
                return KISS_HIP_E_NOMEM;
            }
            ctx->fm_pool_cap[slot] = want;
        }
        p = ctx->fm_pool[slot];
        return KISS_HIP_OK;
    }
};

// the times of a report: six events kept in the ctx (one call at a time per ctx), recorded only for a caller that wants a
// report
struct FmEvents {
    kiss_hip_ctx *ctx;
    bool ok;
    int last = -1; // the last event recorded
    FmEvents(kiss_hip_ctx *c, bool wanted) : ctx(c), ok(wanted)
    {
        for (auto &x : ctx->fm_ev)
            if (ok && !x && hipEventCreate(&x) != hipSuccess) {
                x = nullptr;
                ok = false;
            }
    }
    void mark(int i)
    {
        if (ok && hipEventRecord(ctx->fm_ev[i], ctx->stream) == hipSuccess) last = i;
    }
    float ms(int a, int b)
    {
        float v = 0.f;
        if (!ok || hipEventElapsedTime(&v, ctx->fm_ev[a], ctx->fm_ev[b]) != hipSuccess) return 0.f;
        return v;
    }
};

// the frame of a _dev entry.  fm_enter: the device, the stream of the call, the work arrays.  fm_leave, whichever way the
// steps ended: the time up to the last step that was queued (ms_total: the report's field, or null) and no timer left open
// in the ctx.
static inline int fm_enter(kiss_hip_ctx *ctx, void *stream)
{
    KCHECK(hipSetDevice(ctx->device));
    ctx->stream = stream ? (hipStream_t)stream : ctx->own_stream;
    if (!ctx->deferred_free.empty()) kiss_drain_deferred(ctx);
    return kiss_workspace_ready(ctx);
}
static inline int fm_leave(kiss_hip_ctx *ctx, FmEvents &ev, int rc, float *ms_total)
{
    if (rc != KISS_HIP_OK) (void)hipStreamSynchronize(ctx->stream);
    if (ms_total && ev.last > 0) *ms_total = ev.ms(0, ev.last);
    ktimer_collect(ctx);
    return rc;
}

// the control words of a call: WORDS 64-bit counters in a pooled buffer (d) and their host mirror (h).  fetch() only queues
// the copy (the caller queues another one behind it and then synchronises, or lets kiss_radix_check do that);
// fetch_sync() also waits for it.
template <int WORDS>
struct FmCtl {
    kiss_hip_ctx *ctx = nullptr;
    DevBuf buf;
    unsigned long long *d = nullptr;
    unsigned long long h[WORDS] = {0};
    int take(kiss_hip_ctx *c, FmSlot slot)
    {
        ctx = c;
        KTRY(buf.take(ctx, slot, WORDS * 8));
        d = (unsigned long long *)buf.p;
        return KISS_HIP_OK;
    }
    int zero() { return kiss_zero_u32(ctx, d, WORDS * 2); }
    int fetch()
    {
        KCHECK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        return KISS_HIP_OK;
    }
    int fetch_sync()
    {
        KTRY(fetch());
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
};

static inline bool fm_sa_intv_ok(uint32_t sa_intv) { return sa_intv >= 1 && sa_intv <= KISS_HIP_FMI_MAX_SA_INTV; }
static inline unsigned fm_grid(uint64_t items, unsigned threads) { return (unsigned)div_up(items, threads); }
static inline uint64_t fm_up256(uint64_t bytes) { return (bytes + 255) & ~255ull; }
// bits that hold 0 .. count - 1: at least `least`, at most `cap`
static inline int fm_bits(uint64_t count, int cap = 63, int least = 1)
{
    int b = least;
    while (b < cap && (1ull << b) < count) b++;
    return b;
}
// the arrays of a call laid out in one pooled buffer: carve() gives the offset of the next one (256-byte aligned), size the
// bytes to take once all are carved
struct FmSlab {
    uint64_t size = 0;
    uint64_t carve(uint64_t bytes)
    {
        const uint64_t at = size;
        size += fm_up256(bytes);
        return at;
    }
};

// ---- the _host entries ----
// blocking copies that skip an empty array; a failure is recorded in the ctx
static inline int fm_copy(kiss_hip_ctx *ctx, void *dst, const void *src, uint64_t bytes, hipMemcpyKind kind)
{
    if (!bytes) return KISS_HIP_OK;
    const hipError_t e = hipMemcpy(dst, src, bytes, kind);
    if (e == hipSuccess) return KISS_HIP_OK;
    ctx->last_hip_error = (int)e;
    return KISS_HIP_E_HIP;
}
static inline int fm_h2d(kiss_hip_ctx *ctx, void *dst, const void *src, uint64_t bytes)
{
    return fm_copy(ctx, dst, src, bytes, hipMemcpyHostToDevice);
}
static inline int fm_d2h(kiss_hip_ctx *ctx, void *dst, const void *src, uint64_t bytes)
{
    return fm_copy(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
}

// The arrays of one _host call on the device.  up(): a host array allocated and copied (null stays null; an empty one is still
// a valid pointer); room(): an output allocated, when it is wanted; down(): a result copied back.  The buffers are freed with
// the stage.  rc keeps the first failure (no memory: KISS_HIP_E_NOMEM, a copy: KISS_HIP_E_HIP, the HIP code in the ctx) and
// everything after it does nothing, so an entry looks at rc once before its _dev call and once after its downloads.
struct FmStage {
    kiss_hip_ctx *ctx;
    int rc = KISS_HIP_OK;
    int used = 0;
    DevBuf buf[16];
    explicit FmStage(kiss_hip_ctx *c) : ctx(c) {}
    template <class T>
    T *room(bool wanted, uint64_t bytes, uint64_t spare = 0)
    {
        if (!wanted || rc) return nullptr;
        if (used == (int)(sizeof buf / sizeof buf[0])) {
            rc = KINTERNAL();
            return nullptr;
        }
        rc = buf[used].alloc(ctx, bytes + spare);
        return (T *)buf[used++].p;
    }
    template <class T>
    const T *up(const T *host, uint64_t bytes, uint64_t spare = 0)
    {
        T *d = room<T>(host != nullptr, bytes, spare);
        if (d) rc = fm_h2d(ctx, d, host, bytes);
        return rc ? nullptr : d;
    }
    void down(void *host, const void *dev, uint64_t bytes)
    {
        if (!rc) rc = fm_d2h(ctx, host, dev, bytes);
    }
};

// a host kiss_hip_fmi_view on the device: its six arrays (z: their sizes; bwt and b with 8 spare bytes behind them) and the
// view over the copies.  sa_intv == 1 keeps no bit-vector: b / b_occ are allocated, not copied, and null in the view.
static inline kiss_hip_fmi_view fm_upload_index(FmStage &st, const kiss_hip_fmi_view &h, const kiss_hip_fmi_sizes &z)
{
    const bool bits = h.sa_intv != 1;
    kiss_hip_fmi_view v = h;
    v.bwt = st.up(h.bwt, z.bwt_bytes, 8);
    v.occ1 = st.up(h.occ1, z.occ1_entries * 4);
    v.occ2 = st.up(h.occ2, z.occ2_bytes);
    v.sa = st.up(h.sa, z.sa_entries * 4);
    v.b = bits ? st.up(h.b, z.b_words * 8, 8) : nullptr;
    v.b_occ = bits ? st.up(h.b_occ, z.b_occ_entries * 4) : nullptr;
    if (!bits) (void)(st.room<uint64_t>(true, z.b_words * 8, 8), st.room<uint32_t>(true, z.b_occ_entries * 4));
    return v;
}

// idx[0 .. count] never decreases (strict: and no two neighbours are equal)
static inline bool fm_index_ascending(const uint64_t *idx, uint64_t count, bool strict)
{
    for (uint64_t i = 0; i < count; i++)
        if (idx[i + 1] < idx[i] || (strict && idx[i + 1] == idx[i])) return false;
    return true;
}
// max_n of the ctx of a one-shot call: at least `base` and four times whatever the call sorts in the ctx's LMS arrays or scans
// in its scratch (they hold about 0.32 max_n entries), inside [2^20, KISS_HIP_MAX_N]
static inline uint64_t fm_host_max_n(uint64_t base, uint64_t sorted0, uint64_t sorted1 = 0)
{
    uint64_t max_n = base;
    if (max_n < 4 * sorted0) max_n = 4 * sorted0;
    if (max_n < 4 * sorted1) max_n = 4 * sorted1;
    if (max_n < (1u << 20)) max_n = 1u << 20;
    if (max_n > KISS_HIP_MAX_N) max_n = KISS_HIP_MAX_N;
    return max_n;
}

// fm.hip: fills blk (nblocks = f.N / 64 + 1 blocks of 32 bytes) from the on-disk arrays of f on the ctx stream (k_fm_blocks)
int kiss_fm_make_blocks(kiss_hip_ctx *ctx, const FmiD &f, uint64_t nblocks, uint4 *blk);
// fm.hip: the part of a build that depends on the suffix array only (k_fm_bits / k_fm_sample), queued on the ctx stream.
// sa_intv == 1: d_sa = the whole SA (N entries), d_b / d_b_occ untouched; else the sampling bit-vector (ceil(N / 64) words),
// its rank directory (N / 64 + 1) and the SA values with SA[i] % sa_intv == 0 in row order.
int kiss_fm_sample_sa(kiss_hip_ctx *ctx, const uint32_t *d_SA, uint64_t N, uint32_t sa_intv, uint32_t *d_sa, uint64_t *d_b,
                      uint32_t *d_b_occ);
