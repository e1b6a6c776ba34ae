// fm_internal.hpp -- what the FM-index translation units share (fm.hip: exact queries + construction; fm_mm.hip: the
// search with mismatches; fm_seed.hip: maximal exact match seeds): the device view of an index, the one-sector rank blocks
// and the LF arithmetic on them, the rank of the sampling bit-vector, the bounded locate walk of one row, the pooled
// scratch buffers of a batch and the events behind a report's times.
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
    int take(kiss_hip_ctx *ctx, int slot, uint64_t bytes)
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
        for (auto &x : ctx->fm_mm_ev)
            if (ok && !x && hipEventCreate(&x) != hipSuccess) {
                x = nullptr;
                ok = false;
            }
    }
    void mark(int i)
    {
        if (ok && hipEventRecord(ctx->fm_mm_ev[i], ctx->stream) == hipSuccess) last = i;
    }
    float ms(int a, int b)
    {
        float v = 0.f;
        if (!ok || hipEventElapsedTime(&v, ctx->fm_mm_ev[a], ctx->fm_mm_ev[b]) != hipSuccess) return 0.f;
        return v;
    }
};

// fm.hip: fills blk (nblocks = f.N / 64 + 1 blocks of 32 bytes) from the on-disk arrays of f on the ctx stream (k_fm_blocks)
int kiss_fm_make_blocks(kiss_hip_ctx *ctx, const FmiD &f, uint64_t nblocks, uint4 *blk);
// fm.hip: the part of a build that depends on the suffix array only (k_fm_bits / k_fm_sample), queued on the ctx stream.
// sa_intv == 1: d_sa = the whole SA (N entries), d_b / d_b_occ untouched; else the sampling bit-vector (ceil(N / 64) words),
// its rank directory (N / 64 + 1) and the SA values with SA[i] % sa_intv == 0 in row order.
int kiss_fm_sample_sa(kiss_hip_ctx *ctx, const uint32_t *d_SA, uint64_t N, uint32_t sa_intv, uint32_t *d_sa, uint64_t *d_b,
                      uint32_t *d_b_occ);
