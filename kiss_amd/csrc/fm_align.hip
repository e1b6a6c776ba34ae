// fm_align.hip -- FM-index: the chains of a read aligned to the text, banded, affine gaps (kiss_hip_fmi_align_*).
//
// The reference has no such function; the definition is in include/kiss_hip.h and restated in tests/fm_align_model.py.  The
// input is what kiss_hip_fmi_chain_dev wrote plus the reads and the text.  No index is read.
//
//   prep  : ONE LANE PER CHAIN finds its virtual read by search in chain_index, works out the band and writes the number of
//           DP cells L * B (0 for a band that is too wide); the library's u64 scan gives every chain its stretch of the
//           traceback store, one byte per cell; the host looks at the total once (the cell limit).
//   dp    : ONE WAVE PER CHAIN, lane = diagonal, bands wider than 64 in chunks of 64 lanes, rows swept in ascending i.  The
//           diagonal predecessor and the row above (H, F of row i - 1) are kept per diagonal in LDS and updated in place; E,
//           the only value that runs along a row, is a max-plus prefix scan over the lanes of T = max(0, Hd + s, F): E(k) =
//           max over k' < k of T(k') + k' e, minus o + k e, carried from chunk to chunk.  Exact because gap_open >= 0: a gap
//           that extends a gap never beats the gap opened where the first one was.  The read is loaded 64 rows at a time, one
//           base per lane, and handed out by readlane; the text window of those 64 rows (B + 63 bytes) goes to LDS in one
//           coalesced sweep of byte loads.  Nothing is gathered per cell.  The direction byte of a cell (2 bits source, E
//           opened, F opened, column matched) is stored once, coalesced along the row.  The best cell is a wave reduction of
//           (score, i, diagonal) under the tie rule.
//   trace : ONE LANE PER CHAIN walks the direction bytes back from the best cell and writes the record (into scratch: the
//           caller's arrays are untouched until the capacities are known to suffice) and the number of op runs; a second
//           scan, one look at the totals from the host, and the emit kernel copies the records and walks once more for the
//           ops, written from the last one down.
// All score arithmetic is signed 32-bit; -inf is AL_NEG, clamped wherever a value derived from it is stored.
#include "fm_internal.hpp"

#include <vector>

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_WAVES = AL_THREADS / 64;
constexpr int AL_MAXB = (int)KISS_HIP_ALIGN_MAX_BAND;
constexpr int AL_NEG = -(1 << 30);

// direction byte of a cell
enum { AL_SRC = 3, AL_STOP = 0, AL_DIAG = 1, AL_FROM_E = 2, AL_FROM_F = 3, AL_EOPEN = 4, AL_FOPEN = 8, AL_MATCH = 16 };

// control block of a call (u64 words)
enum { AL_BAD = 0, AL_C0 = 1, AL_C1 = 2, AL_MAXL = 3, AL_WIDE = 4, AL_MAXBAND = 5, AL_BEST = 6, AL_CTL_WORDS = 8 };

struct AlignP {
    int match, mismatch, open, ext;
    uint32_t band;
};

struct Band {
    long long dlo;
    unsigned long long B; // (below 2^34)
};
__host__ __device__ inline Band band_of(const kiss_hip_chain &c, uint32_t band)
{
    const long long d0 = (long long)c.tbeg - (long long)c.rbeg, d1 = (long long)c.tend - (long long)c.rend;
    const long long lo = (d0 < d1 ? d0 : d1) - (long long)band, hi = (d0 < d1 ? d1 : d0) + (long long)band;
    Band b;
    b.dlo = lo;
    b.B = (unsigned long long)(hi - lo + 1);
    return b;
}

// a chain_index that decreases, a read_index that does not ascend; the two ends of chain_index and the longest read
__global__ __launch_bounds__(AL_THREADS) void k_align_head(const uint64_t *__restrict__ chain_index, uint64_t V,
                                                          const uint64_t *__restrict__ read_index, uint64_t Q,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (g == 0) {
        ctl[AL_C0] = chain_index[0];
        ctl[AL_C1] = chain_index[V];
    }
    bool bad = g < V && chain_index[g + 1] < chain_index[g];
    unsigned long long len = 0;
    if (g < Q) {
        const uint64_t a = read_index[g], b = read_index[g + 1];
        if (b <= a) bad = true; // (a zero-length read too)
        else len = b - a;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(len, s, 64);
        len = o > len ? o : len;
    }
    if (__ballot(bad) && lane_id() == 0) ctl[AL_BAD] = 1;
    if (len && lane_id() == 0) atomicMax(&ctl[AL_MAXL], len);
}

// one lane per chain a: its virtual read (the last v with chain_index[v] <= c0 + a: reads without chains own empty
// segments), its cells; lane C closes the array for the scan
__global__ __launch_bounds__(AL_THREADS) void k_align_prep(const kiss_hip_chain *__restrict__ chains,
                                                          const uint64_t *__restrict__ chain_index, uint64_t V, uint64_t c0,
                                                          uint64_t C, const uint64_t *__restrict__ read_index, int both,
                                                          uint32_t band, uint32_t *__restrict__ vof, uint64_t *__restrict__ cells,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint64_t a = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    bool wide = false;
    unsigned long long mb = 0;
    if (a < C) {
        uint64_t lo = 0, hi = V;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (chain_index[mid] <= c0 + a) lo = mid;
            else hi = mid;
        }
        const uint64_t q = both ? lo >> 1 : lo;
        const uint64_t L = read_index[q + 1] - read_index[q];
        const Band b = band_of(chains[c0 + a], band);
        wide = b.B > (unsigned long long)AL_MAXB;
        vof[a] = (uint32_t)lo;
        cells[a] = wide ? 0ull : L * b.B;
        mb = wide ? 0ull : b.B;
    } else if (a == C) {
        cells[a] = 0;
    }
    const unsigned long long nw = (unsigned long long)__popcll(__ballot(wide));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(mb, s, 64);
        mb = o > mb ? o : mb;
    }
    if (lane_id() == 0) {
        if (nw) atomicAdd(&ctl[AL_WIDE], nw);
        if (mb) atomicMax(&ctl[AL_MAXBAND], mb);
    }
}

// LDS traffic between the lanes of ONE wave: the compiler must not move LDS accesses across this point, and the accesses
// before it have finished (a wave's LDS instructions run in order; nothing waits for another wave)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One wave per chain.  best[a] = (score, i, diagonal k) of the best cell, score 0: none.
__global__ __launch_bounds__(AL_THREADS) void k_align_dp(const uint8_t *__restrict__ text, uint64_t n,
                                                        const uint8_t *__restrict__ reads, const uint64_t *__restrict__ read_index,
                                                        int both, const kiss_hip_chain *__restrict__ chains, uint64_t c0, uint64_t C,
                                                        const uint32_t *__restrict__ vof, const uint64_t *__restrict__ cell_off,
                                                        AlignP P, uint8_t *__restrict__ store, uint32_t *__restrict__ best)
{
    __shared__ int s_h[AL_WAVES][AL_MAXB + 4]; // H of the row above, per diagonal; AL_NEG: no such cell
    __shared__ int s_f[AL_WAVES][AL_MAXB + 4]; // F of the row above
    __shared__ uint8_t s_t[AL_WAVES][AL_MAXB + 64]; // text under the 64 rows of a group: [row in group + diagonal]
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    const uint64_t a = (uint64_t)blockIdx.x * AL_WAVES + w;
    if (a >= C) return;
    const uint64_t cells = cell_off[a + 1] - cell_off[a];
    if (cells == 0) return; // too wide
    const uint32_t v = vof[a];
    const uint64_t q = both ? v >> 1 : v;
    const bool rev = both && (v & 1u);
    const uint64_t r0 = read_index[q];
    const uint32_t L = (uint32_t)(read_index[q + 1] - r0);
    const Band bd = band_of(chains[c0 + a], P.band);
    const int B = (int)bd.B;
    const long long dlo = bd.dlo;
    uint8_t *__restrict__ dirs = store + cell_off[a];
    int *hp = s_h[w], *fp = s_f[w];
    uint8_t *tw = s_t[w];
    for (int k = (int)lane; k <= B; k += 64) { // (entry B: what lane B - 1 reads as its right neighbour)
        hp[k] = AL_NEG;
        fp[k] = AL_NEG;
    }
    const int oe = P.open + P.ext;
    int bh = 0;
    uint32_t bi = 0, bk = 0;
    for (uint32_t i0 = 1; i0 <= L; i0 += 64) {
        const uint32_t rows = L - i0 + 1 < 64u ? L - i0 + 1 : 64u;
        // j of diagonal 0 in row i0; the group covers j0 .. j0 + rows - 1 + B - 1
        const long long j0 = (long long)i0 + dlo;
        if (j0 + (long long)(rows - 1) + (long long)(B - 1) < 1) continue; // still left of the text
        if (j0 > (long long)n) break;                                       // right of it, for good
        uint32_t rc = 4;
        if (lane < rows) {
            const uint32_t at = i0 - 1 + lane;
            const uint32_t c = rev ? reads[r0 + (L - 1 - at)] : reads[r0 + at];
            rc = c > 3u ? 4u : (rev ? 3u - c : c);
        }
        wave_lds_sync(); // (the rows of the last group have read their text)
        for (int x = (int)lane; x < B + 63; x += 64) {
            const long long p = j0 - 1 + x; // text position of column j0 + x
            tw[x] = (p >= 0 && p < (long long)n) ? text[p] : (uint8_t)0xFF;
        }
        wave_lds_sync();
        for (uint32_t r = 0; r < rows; r++) {
            const uint32_t i = i0 + r;
            const long long jk0 = j0 + r; // j of diagonal 0 in this row
            const long long kmin64 = jk0 >= 1 ? 0 : 1 - jk0, kmax64 = (long long)n - jk0 < (long long)(B - 1) ? (long long)n - jk0 : (long long)(B - 1);
            if (kmin64 > kmax64) {
                if (jk0 < 1) continue; // not yet in the text
                break;                 // past it (the group loop ends with the next j0)
            }
            const int kmin = (int)kmin64, kmax = (int)kmax64;
            const int x = (int)__builtin_amdgcn_readlane((int)rc, (int)r);
            int carry = AL_NEG, hleft = AL_NEG; // prefix of T + k e over the chunks before; H of the lane before the chunk
            uint8_t *drow = dirs + (uint64_t)(i - 1) * (uint64_t)B;
            for (int cb = kmin & ~63; cb <= kmax; cb += 64) {
                const int k = cb + (int)lane;
                const bool valid = k >= kmin && k <= kmax;
                const int kk = k < B ? k : B; // (lanes past the band read entry B and write nothing)
                const int hd = hp[kk], hup = hp[kk + (k < B ? 1 : 0)], fup = fp[kk + (k < B ? 1 : 0)];
                const int y = tw[r + (k < B ? k : 0)];
                wave_lds_sync();
                const int s = (x == y && x <= 3) ? P.match : (x > 3 ? -1 : -P.mismatch);
                int F = hup - oe > fup - P.ext ? hup - oe : fup - P.ext;
                F = F < AL_NEG ? AL_NEG : F;
                const int dg = (hd > 0 ? hd : 0) + s;
                int T = dg > F ? dg : F;
                T = T > 0 ? T : 0;
                // inclusive max-scan of T + k e over the lanes
                const int ke = (k - cb) * P.ext; // (relative to the chunk: the carry is rebased below)
                int u = valid ? T + ke : AL_NEG;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(u, d, 64);
                    if ((int)lane >= d) u = o > u ? o : u;
                }
                int pre = __shfl_up(u, 1, 64);
                if (lane == 0) pre = AL_NEG;
                pre = carry > pre ? carry : pre;
                int E = pre - P.open - ke;
                E = E < AL_NEG ? AL_NEG : E;
                const int H = valid ? (T > E ? T : E) : AL_NEG;
                int hl = __shfl_up(H, 1, 64);
                if (lane == 0) hl = hleft;
                if (valid) {
                    int dir = H == 0 ? AL_STOP : (H == dg ? AL_DIAG : (H == E ? AL_FROM_E : AL_FROM_F));
                    if (E == hl - oe) dir |= AL_EOPEN;
                    if (F == hup - oe) dir |= AL_FOPEN;
                    if (s > 0) dir |= AL_MATCH;
                    drow[k] = (uint8_t)dir;
                    if (H > bh) { // (rows ascend, and so do the chunks of a row: the first of equals stays)
                        bh = H;
                        bi = i;
                        bk = (uint32_t)k;
                    }
                }
                if (k < B) {
                    hp[k] = H;
                    fp[k] = valid ? F : AL_NEG;
                }
                // the next chunk: its k e starts 64 e further on
                const int last = __shfl(u, 63, 64);
                carry = (carry > last ? carry : last) - 64 * P.ext;
                carry = carry < AL_NEG ? AL_NEG : carry;
                hleft = __shfl(H, 63, 64);
                wave_lds_sync();
            }
        }
    }
    // the best cell: the largest H, then the smallest i, then the smallest diagonal (= the smallest j in that row)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int oh = __shfl_xor(bh, s, 64);
        const uint32_t oi = __shfl_xor(bi, s, 64), ok = __shfl_xor(bk, s, 64);
        if (oh > bh || (oh == bh && (oi < bi || (oi == bi && ok < bk)))) {
            bh = oh;
            bi = oi;
            bk = ok;
        }
    }
    if (lane == 0) {
        best[3 * a] = (uint32_t)bh;
        best[3 * a + 1] = bi;
        best[3 * a + 2] = bk;
    }
}

// the walk back from the best cell of a chain: f(op, len) for every maximal run, from the LAST run to the first; returns the
// cell the path starts behind (i, j) and counts into rec.  Every step lowers i or j, so the walk ends.
template <typename Fn>
__device__ __forceinline__ void align_walk(const uint8_t *__restrict__ dirs, int B, long long dlo, uint32_t bi, uint32_t bk,
                                           kiss_hip_aln &rec, Fn f)
{
    long long i = bi, j = (long long)bi + dlo + (long long)bk;
    int k = (int)bk;
    rec.rend = (uint32_t)i;
    rec.tend = (uint32_t)j;
    int state = 0; // 0: H, 1: E, 2: F
    int op = -1;
    uint32_t run = 0;
    const auto emit = [&](int o) {
        if (o == op) {
            run++;
            return;
        }
        if (op >= 0) f(op, run);
        if (o == 1 || o == 2) rec.gaps++;
        op = o;
        run = 1;
    };
    while (i > 0 && j > 0 && k >= 0 && k < B) {
        const int d = dirs[(uint64_t)(i - 1) * (uint64_t)B + (uint64_t)k];
        if (state == 0) {
            const int src = d & AL_SRC;
            if (src == AL_STOP) break;
            if (src == AL_DIAG) {
                emit(0);
                if (d & AL_MATCH) rec.matches++;
                else rec.mismatches++;
                i--;
                j--;
                continue;
            }
            state = src == AL_FROM_E ? 1 : 2;
        }
        if (state == 1) {
            emit(2);
            rec.del++;
            if (d & AL_EOPEN) state = 0;
            j--;
            k--;
        } else {
            emit(1);
            rec.ins++;
            if (d & AL_FOPEN) state = 0;
            i--;
            k++;
        }
    }
    if (op >= 0) f(op, run);
    rec.rbeg = (uint32_t)i;
    rec.tbeg = (uint32_t)j;
}

// one lane per chain: the record (into scratch) and the number of op runs; lane C closes the array for the scan
__global__ __launch_bounds__(AL_THREADS) void k_align_trace(const kiss_hip_chain *__restrict__ chains, uint64_t c0, uint64_t C,
                                                           const uint64_t *__restrict__ cell_off, uint32_t band,
                                                           const uint8_t *__restrict__ store, const uint32_t *__restrict__ best,
                                                           kiss_hip_aln *__restrict__ recs, uint64_t *__restrict__ nops,
                                                           unsigned long long *__restrict__ ctl)
{
    const uint64_t a = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    unsigned long long sc = 0;
    if (a < C) {
        const Band bd = band_of(chains[c0 + a], band);
        kiss_hip_aln rec{};
        rec.band = bd.B > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bd.B;
        uint64_t ops = 0;
        if (bd.B > (unsigned long long)AL_MAXB) {
            rec.flags = KISS_HIP_ALN_BAND_TOO_WIDE;
        } else if (cell_off[a + 1] > cell_off[a] && best[3 * a]) {
            rec.score = best[3 * a];
            align_walk(store + cell_off[a], (int)bd.B, bd.dlo, best[3 * a + 1], best[3 * a + 2], rec, [&](int, uint32_t) { ops++; });
            sc = rec.score;
        }
        recs[a] = rec;
        nops[a] = ops;
    } else if (a == C) {
        nops[a] = 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(sc, s, 64);
        sc = o > sc ? o : sc;
    }
    if (sc && lane_id() == 0) atomicMax(&ctl[AL_BEST], sc);
}

// one lane per chain: the record to the caller, cigar_index, and the ops from the last one down; lane C closes cigar_index
__global__ __launch_bounds__(AL_THREADS) void k_align_emit(const kiss_hip_chain *__restrict__ chains, uint64_t c0, uint64_t C,
                                                          const uint64_t *__restrict__ cell_off, uint32_t band,
                                                          const uint8_t *__restrict__ store, const uint32_t *__restrict__ best,
                                                          const kiss_hip_aln *__restrict__ recs, const uint64_t *__restrict__ op_off,
                                                          kiss_hip_aln *__restrict__ alns, uint32_t *__restrict__ cigar,
                                                          uint64_t *__restrict__ cigar_index)
{
    const uint64_t a = (uint64_t)blockIdx.x * AL_THREADS + threadIdx.x;
    if (a > C) return;
    if (cigar_index) cigar_index[a] = op_off[a];
    if (a == C) return;
    const kiss_hip_aln rec = recs[a];
    alns[a] = rec;
    if (!cigar || !rec.score) return;
    const Band bd = band_of(chains[c0 + a], band);
    uint64_t at = op_off[a + 1];
    const uint64_t first = op_off[a];
    kiss_hip_aln again{};
    align_walk(store + cell_off[a], (int)bd.B, bd.dlo, best[3 * a + 1], best[3 * a + 2], again, [&](int op, uint32_t len) {
        if (at > first) cigar[--at] = (len << 4) | (uint32_t)op;
    });
}

int align_steps(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                int both, uint64_t V, const kiss_hip_chain *chains, const uint64_t *chain_index, const AlignP &P, kiss_hip_aln *alns,
                uint64_t aln_capacity, uint32_t *cigar, uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_align_report *rep,
                FmEvents &ev)
{
    if (n > KISS_HIP_MAX_N || V > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    kiss_opts_refresh(ctx);
    DevBuf slab, st;
    FmCtl<AL_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_ALIGN_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_align_head, dim3(fm_grid(V + 1, AL_THREADS)), dim3(AL_THREADS), 0, ctx->stream, chain_index, V, read_index, Q, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[AL_BAD]) return KISS_HIP_E_INVALID; // chain_index or read_index decreases, or a read of length 0
    const uint64_t c0 = h[AL_C0], C = h[AL_C1] - c0;
    if (rep) rep->chains = C;
    if (h[AL_MAXL] * (uint64_t)P.match >= (1ull << 30)) return KISS_HIP_E_UNSUPPORTED;
    if (C >= 0xFFFFFFFFull || (C + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    if (C == 0) {
        if (cigar_index) KTRY(kiss_zero_u32(ctx, cigar_index, 2));
        ev.mark(1);
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    // the per-chain arrays of the call, one slab
    FmSlab lay;
    const uint64_t o_cells = lay.carve((C + 1) * 8), o_nops = lay.carve((C + 1) * 8), o_recs = lay.carve(C * sizeof(kiss_hip_aln)),
                   o_best = lay.carve(C * 12), o_vof = lay.carve(C * 4);
    KTRY(slab.take(ctx, FM_SLOT_ALIGN_SLAB, lay.size));
    char *sb = (char *)slab.p;
    uint64_t *cells = (uint64_t *)(sb + o_cells), *nops = (uint64_t *)(sb + o_nops);
    kiss_hip_aln *recs = (kiss_hip_aln *)(sb + o_recs);
    uint32_t *best = (uint32_t *)(sb + o_best), *vof = (uint32_t *)(sb + o_vof);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_align_prep, dim3(fm_grid(C + 1, AL_THREADS)), dim3(AL_THREADS), 0, ctx->stream, chains, chain_index, V, c0, C,
                           read_index, both, P.band, vof, cells, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, cells, cells, C + 1));
    uint64_t total_cells = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total_cells, cells + C, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) {
        rep->too_wide = h[AL_WIDE];
        rep->aligned = C - h[AL_WIDE];
        rep->cells = total_cells;
        rep->max_band = (uint32_t)h[AL_MAXBAND];
    }
    // (the total is in the report: split the batch)
    if (total_cells > (uint64_t)KISS_HIP_ALIGN_CELLS_PER_N * ctx->max_n) return KISS_HIP_E_UNSUPPORTED;
    KTRY(st.take(ctx, FM_SLOT_ALIGN_TRACE, total_cells));
    uint8_t *store = (uint8_t *)st.p;
    ev.mark(1);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, total_cells);
        hipLaunchKernelGGL(k_align_dp, dim3((unsigned)div_up(C, AL_WAVES)), dim3(AL_THREADS), 0, ctx->stream, text, n, reads, read_index,
                           both, chains, c0, C, (const uint32_t *)vof, (const uint64_t *)cells, P, store, best);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_align_trace, dim3(fm_grid(C + 1, AL_THREADS)), dim3(AL_THREADS), 0, ctx->stream, chains, c0, C, (const uint64_t *)cells,
                           P.band, (const uint8_t *)store, (const uint32_t *)best, recs, nops, d_ctl);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    KTRY(kiss_scan_u64(ctx, nops, nops, C + 1));
    uint64_t total_ops = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total_ops, nops + C, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) {
        rep->cigar_ops = total_ops;
        rep->best_score = (uint32_t)h[AL_BEST];
        rep->ms_dp = ev.ms(1, 2);
        rep->ms_trace = ev.ms(2, 3);
    }
    // (the totals are in the report: the caller's second call)
    if (aln_capacity < C || (cigar && cigar_capacity < total_ops)) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, C);
        hipLaunchKernelGGL(k_align_emit, dim3(fm_grid(C + 1, AL_THREADS)), dim3(AL_THREADS), 0, ctx->stream, chains, c0, C, (const uint64_t *)cells,
                           P.band, (const uint8_t *)store, (const uint32_t *)best, (const kiss_hip_aln *)recs, (const uint64_t *)nops,
                           alns, cigar, cigar_index);
        KCHECK(hipGetLastError());
    }
    ev.mark(4);
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (rep) rep->ms_emit = ev.ms(3, 4); // the scan, one look at the totals from the host, the records and the ops
    return KISS_HIP_OK;
}

int align_args_check(const uint8_t *text, const uint8_t *reads, const uint64_t *read_index, const kiss_hip_chain *chains,
                     const uint64_t *chain_index, const kiss_hip_align_params *params, const kiss_hip_aln *alns, const uint32_t *cigar,
                     const uint64_t *cigar_index, uint64_t cigar_capacity)
{
    const bool any = cigar || cigar_index, all = cigar && cigar_index;
    if (!text || !reads || !read_index || !chains || !chain_index || !params || !alns || any != all || (!any && cigar_capacity))
        return KISS_HIP_E_INVALID;
    if (params->match < 1 || params->match > 65535u || params->mismatch > 65535u || params->gap_open > 65535u ||
        params->gap_extend > 65535u || params->band > 0x7FFFFFFFu)
        return KISS_HIP_E_INVALID;
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_align_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index,
                           uint64_t Q, int both_strands, const kiss_hip_chain *chains, const uint64_t *chain_index,
                           const kiss_hip_align_params *params, kiss_hip_aln *alns, uint64_t aln_capacity, uint32_t *cigar,
                           uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_align_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (report) {
        *report = kiss_hip_align_report{};
        report->V = V;
    }
    KTRY(align_args_check(text, reads, read_index, chains, chain_index, params, alns, cigar, cigar_index, cigar_capacity));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if (V == 0) { // cigar_index[0] = 0
        if (cigar_index) KTRY(kiss_zero_u32(ctx, cigar_index, 2));
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    AlignP P;
    P.match = (int)params->match;
    P.mismatch = (int)params->mismatch;
    P.open = (int)params->gap_open;
    P.ext = (int)params->gap_extend;
    P.band = params->band;
    FmEvents ev(ctx, report != nullptr);
    const int rc = align_steps(ctx, text, n, reads, read_index, Q, both_strands ? 1 : 0, V, chains, chain_index, P, alns, aln_capacity,
                               cigar, cigar_index, cigar_capacity, report, ev);
    return fm_leave(ctx, ev, rc, report ? &report->ms_total : nullptr);
}

int kiss_hip_fmi_align_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                            int both_strands, const kiss_hip_chain *chains, const uint64_t *chain_index,
                            const kiss_hip_align_params *params, kiss_hip_aln *alns, uint64_t aln_capacity, uint32_t *cigar,
                            uint64_t *cigar_index, uint64_t cigar_capacity, kiss_hip_align_report *report, int device)
{
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (report) {
        *report = kiss_hip_align_report{};
        report->V = V;
    }
    KTRY(align_args_check(text, reads, read_index, chains, chain_index, params, alns, cigar, cigar_index, cigar_capacity));
    if (!fm_index_ascending(read_index, Q, true) || !fm_index_ascending(chain_index, V, false)) return KISS_HIP_E_INVALID;
    const uint64_t nchains = chain_index[V], nbases = read_index[Q]; // (the arrays are uploaded from their first entry)
    // the cells of the call decide the size of the context (KISS_HIP_ALIGN_CELLS_PER_N cells per base of max_n); no
    // alignment has more ops than 2 L + 1
    uint64_t cells = 0, max_ops = 0;
    for (uint64_t v = 0; v < V; v++) {
        const uint64_t q = both_strands ? v >> 1 : v, L = read_index[q + 1] - read_index[q];
        for (uint64_t c = chain_index[v]; c < chain_index[v + 1]; c++) {
            const Band b = band_of(chains[c], params->band);
            if (b.B <= (unsigned long long)AL_MAXB) {
                cells += L * b.B;
                max_ops += 2 * L + 1;
            }
        }
    }
    const uint64_t C = nchains - chain_index[0];
    return kiss_one_shot_cached(device, fm_host_max_n(cells / KISS_HIP_ALIGN_CELLS_PER_N + 1, C + 1, V + 1), [&](kiss_hip_ctx *ctx) -> int {
        const bool all = cigar != nullptr;
        const uint64_t acap = aln_capacity < C ? aln_capacity : C, ocap = cigar_capacity < max_ops ? cigar_capacity : max_ops;
        FmStage st(ctx);
        const uint8_t *dtext = st.up(text, n);
        const uint8_t *dreads = st.up(reads, nbases);
        const uint64_t *dridx = st.up(read_index, (Q + 1) * 8);
        const kiss_hip_chain *dchains = st.up(chains, nchains * sizeof(kiss_hip_chain));
        const uint64_t *dcidx = st.up(chain_index, (V + 1) * 8);
        kiss_hip_aln *dalns = st.room<kiss_hip_aln>(true, acap * sizeof(kiss_hip_aln));
        uint32_t *dcig = st.room<uint32_t>(all, ocap * 4);
        uint64_t *doidx = st.room<uint64_t>(all, (C + 1) * 8);
        if (st.rc) return st.rc;
        kiss_hip_align_report r{};
        const int rc = kiss_hip_fmi_align_dev(ctx, dtext, n, dreads, dridx, Q, both_strands ? 1 : 0, dchains, dcidx, params, dalns, acap, dcig,
                                              doidx, all ? ocap : 0, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(alns, dalns, C * sizeof(kiss_hip_aln));
        if (all) st.down(cigar_index, doidx, (C + 1) * 8);
        if (all) st.down(cigar, dcig, r.cigar_ops * 4);
        return st.rc;
    });
}

} // extern "C"
