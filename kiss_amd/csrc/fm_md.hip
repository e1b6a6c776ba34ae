// fm_md.hip -- FM-index: the MD:Z strings of alignments, written on the GPU (kiss_hip_fmi_md_*).
//
// The reference has no such function; the definition is in include/kiss_hip_md.h and restated in tests/fm_md_model.py.  The
// call reads what the align (or merge) call and the select call wrote, and the text and the reads they were made from.
//
//   head  : one kernel checks chain_index and read_index and fetches the ends of chain_index (C); a second one, once C is
//           known, checks cigar_index.
//   count : ONE WAVE PER ITEM (a wave takes items h, h + waves, ...).  The wave finds the virtual read of the alignment by
//           bisection of chain_index, holds the record against the read and the text and the op list against the record (lanes
//           over the ops, 64 at a time, sums by wave reduction), then goes through the ops in order with lanes over the columns
//           of the current op, 64 per step.  Per step the lanes that END A RUN (a mismatch) are found by ballot; a lane's run is
//           the distance to the previous set bit or, for the first one, the wave-uniform carry plus its lane; its bytes are
//           digits(run) + 1; a prefix sum over the wave places them.  A step without a mismatch is one ballot and an add.
//           A D op needs no prefix sum: only its first base carries a number.  run and the offset go from step to step in
//           wave-uniform registers.
//   scan  : the library's u64 scan over the items + 1 sizes; the host looks at the total once (capacity).
//   emit  : the same walk again, now writing (plain byte stores), and md_index / md_counts.
// No LDS, no scratch: the state of a walk is a handful of registers.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_md.h"

#include <vector>

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = MD_THREADS / 64;
constexpr unsigned MD_MAX_BLOCKS = 8192;

// control block of a call (u64 words)
enum { MD_BADIN = 0, MD_C0 = 1, MD_C1 = 2, MD_BAD = 3, MD_MISM = 4, MD_DEL = 5, MD_LONGEST = 6, MD_CTL_WORDS = 8 };

// Every load of a field or an index entry starts at a multiple of its own size, as in fm_pair.hip: relaxed
// loads and stores of wavefront scope, which the compiler does not merge into wider ones.
__device__ __forceinline__ uint32_t md_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t md_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void md_st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

__device__ __forceinline__ uint64_t md_wave_sum64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// the sum of v over the lanes below this one; total: over the wave
__device__ __forceinline__ uint32_t md_wave_excl32(uint32_t v, uint32_t &total)
{
    const uint32_t lane = lane_id();
    uint32_t s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(s, o, 64);
        if (lane >= (uint32_t)o) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

__device__ __forceinline__ uint32_t md_digits(uint32_t x)
{
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
           (x >= 100000000u) + (x >= 1000000000u);
}
// x in decimal, d = md_digits(x) bytes
__device__ __forceinline__ void md_put_number(uint8_t *p, uint32_t x, uint32_t d)
{
    for (uint32_t k = d; k-- > 0;) {
        p[k] = (uint8_t)('0' + x % 10u);
        x /= 10u;
    }
}
__device__ __forceinline__ uint8_t md_letter(uint32_t c) { return c == 0 ? 'A' : (c == 1 ? 'C' : (c == 2 ? 'G' : (c == 3 ? 'T' : 'N'))); }

// a chain_index that decreases, a read_index that does not ascend (a zero-length read too); the ends of chain_index
__global__ __launch_bounds__(MD_THREADS) void k_md_head(const uint64_t *__restrict__ chain_index, uint64_t V, const uint64_t *__restrict__ read_index,
                                                       uint64_t Q, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (g == 0) {
        ctl[MD_C0] = md_ld64(chain_index);
        ctl[MD_C1] = md_ld64(chain_index + V);
    }
    bool bad = g < V && md_ld64(chain_index + g + 1) < md_ld64(chain_index + g);
    if (g < Q && md_ld64(read_index + g + 1) <= md_ld64(read_index + g)) bad = true;
    if (__ballot(bad) && lane_id() == 0) ctl[MD_BADIN] = 1;
}
// a cigar_index that decreases
__global__ __launch_bounds__(MD_THREADS) void k_md_check_ops(const uint64_t *__restrict__ cigar_index, uint64_t C, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    const bool bad = g < C && md_ld64(cigar_index + g + 1) < md_ld64(cigar_index + g);
    if (__ballot(bad) && lane_id() == 0) ctl[MD_BADIN] = 1;
}

struct MdIn {
    const uint8_t *text;
    uint64_t n;
    const uint8_t *reads;
    const uint64_t *read_index;
    int both;
    const kiss_hip_aln *alns;
    const uint64_t *chain_index;
    uint64_t V, c0, C;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const kiss_hip_hit *hits;
    uint64_t items;
};

// what a wave knows of its item once it is opened; every field is the same in all lanes
struct MdItem {
    uint64_t rb, L; // where the read starts in reads, its length
    uint64_t o0, nops;
    uint32_t rbeg, tbeg;
    bool rev;
};
enum { MD_WALK = 0, MD_EMPTY = 1, MD_ISBAD = 2 };

// The item held against the definition.  CHECK false (the emit pass, for an item whose string is not empty): the fields alone.
template <bool CHECK>
__device__ __forceinline__ int md_open(const MdIn &in, uint64_t h, MdItem &it)
{
    const uint32_t lane = lane_id();
    const uint64_t a = in.hits ? (uint64_t)md_ld32(&in.hits[h].aln) : h;
    if (a >= in.C) return MD_ISBAD;
    const uint64_t x = md_ld64(in.cigar_index + a), y = md_ld64(in.cigar_index + a + 1);
    it.o0 = x;
    it.nops = y > x ? y - x : 0; // (an index that decreases fails the call: k_md_check_ops)
    if (it.nops == 0) return MD_EMPTY;
    // the largest v with chain_index[v] <= c0 + a (chain_index[V] > c0 + a: a < C)
    const uint64_t at = in.c0 + a;
    uint64_t lo = 0, hi = in.V;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (md_ld64(in.chain_index + mid) <= at) lo = mid;
        else hi = mid;
    }
    const uint64_t q = in.both ? lo >> 1 : lo;
    it.rev = in.both && (lo & 1ull);
    it.rb = md_ld64(in.read_index + q);
    it.L = md_ld64(in.read_index + q + 1) - it.rb;
    const uint32_t *rec = &in.alns[a].score;
    const uint32_t rbeg = md_ld32(rec + 2), rend = md_ld32(rec + 3), tbeg = md_ld32(rec + 4), tend = md_ld32(rec + 5);
    it.rbeg = rbeg;
    it.tbeg = tbeg;
    if (!CHECK) return MD_WALK;
    if ((uint64_t)rend > it.L || (uint64_t)tend > in.n || rbeg > rend || tbeg > tend) return MD_ISBAD;
    uint64_t sum_r = 0, sum_t = 0;
    bool bad_op = false;
    for (uint64_t kb = 0; kb < it.nops; kb += 64) {
        if (kb + lane < it.nops) {
            const uint32_t w = md_ld32(in.cigar + it.o0 + kb + lane);
            const uint32_t op = w & 15u;
            const uint64_t len = w >> 4;
            bad_op = bad_op || op > 2u || len == 0;
            if (op == 0 || op == 1) sum_r += len;
            if (op == 0 || op == 2) sum_t += len;
        }
    }
    if (__ballot(bad_op)) return MD_ISBAD;
    if (md_wave_sum64(sum_r) != (uint64_t)(rend - rbeg) || md_wave_sum64(sum_t) != (uint64_t)(tend - tbeg)) return MD_ISBAD;
    return MD_WALK;
}

// The walk of an item that md_open<true> let through: i stays inside [rbeg, rend) of a read of L bases, j inside [tbeg, tend)
// of the text, and EMIT writes exactly the bytes EMIT false counted.  -> the bytes of the string; mism / del: its counts.
template <bool EMIT>
__device__ __forceinline__ uint64_t md_walk(const MdIn &in, const MdItem &it, uint8_t *out, uint32_t &mism, uint32_t &del)
{
    const uint32_t lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint8_t *const rd = in.reads + it.rb;
    uint64_t i = it.rbeg, j = it.tbeg, off = 0;
    uint32_t run = 0;
    mism = del = 0;
    for (uint64_t kb = 0; kb < it.nops; kb += 64) {
        const uint32_t mine = kb + lane < it.nops ? md_ld32(in.cigar + it.o0 + kb + lane) : 0u;
        const uint32_t here = it.nops - kb < 64 ? (uint32_t)(it.nops - kb) : 64u;
        for (uint32_t kk = 0; kk < here; kk++) {
            const uint32_t w = __builtin_amdgcn_readfirstlane(__shfl(mine, (int)kk, 64));
            const uint32_t op = w & 15u, len = w >> 4;
            if (op == 1u) { // an insertion does not end a run
                i += len;
                continue;
            }
            if (op == 2u) { // only the first base carries the number and the '^'
                const uint32_t d = md_digits(run);
                if (EMIT) {
                    if (lane == 0) {
                        md_put_number(out + off, run, d);
                        out[off + d] = '^';
                    }
                    for (uint32_t c = lane; c < len; c += 64) out[off + d + 1 + c] = md_letter(in.text[j + c]);
                }
                off += (uint64_t)d + 1 + len;
                run = 0;
                j += len;
                del += len;
                continue;
            }
            for (uint32_t c0 = 0; c0 < len; c0 += 64) {
                const uint32_t cnt = len - c0 < 64 ? len - c0 : 64u;
                uint32_t tj = 0;
                bool ends = false;
                if (lane < cnt) {
                    const uint64_t ri = i + c0 + lane;
                    uint32_t r = it.rev ? rd[it.L - 1 - ri] : rd[ri];
                    if (it.rev && r <= 3u) r = 3u - r;
                    tj = in.text[j + c0 + lane];
                    ends = !(r <= 3u && r == tj);
                }
                const unsigned long long E = __ballot(ends);
                if (!E) {
                    run += cnt;
                    continue;
                }
                const unsigned long long m = E & below;
                const uint32_t my_run = m ? lane - (63u - (uint32_t)__builtin_clzll(m)) - 1u : run + lane;
                const uint32_t d = md_digits(my_run);
                uint32_t total;
                const uint32_t ex = md_wave_excl32(ends ? d + 1u : 0u, total);
                if (EMIT && ends) {
                    md_put_number(out + off + ex, my_run, d);
                    out[off + ex + d] = md_letter(tj);
                }
                off += total;
                mism += (uint32_t)__popcll(E);
                run = cnt - 1u - (63u - (uint32_t)__builtin_clzll(E));
            }
            i += len;
            j += len;
        }
    }
    const uint32_t d = md_digits(run);
    if (EMIT && lane == 0) md_put_number(out + off, run, d);
    return off + d;
}

// size[h] = the bytes of item h (size[items] = 0 closes the array for the scan); the report's counts
__global__ __launch_bounds__(MD_THREADS) void k_md_count(MdIn in, uint64_t *__restrict__ size, unsigned long long *__restrict__ ctl)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) size[in.items] = 0;
    const uint64_t waves = (uint64_t)gridDim.x * MD_WAVES;
    unsigned long long a_bad = 0, a_mism = 0, a_del = 0, a_longest = 0;
    for (uint64_t h = (uint64_t)blockIdx.x * MD_WAVES + (threadIdx.x >> 6); h < in.items; h += waves) {
        MdItem it;
        const int what = md_open<true>(in, h, it);
        uint64_t bytes = 0;
        if (what == MD_WALK) {
            uint32_t mism, del;
            bytes = md_walk<false>(in, it, nullptr, mism, del);
            a_mism += mism;
            a_del += del;
            a_longest = a_longest > bytes ? a_longest : bytes;
        } else if (what == MD_ISBAD) {
            a_bad++;
        }
        if (lane_id() == 0) size[h] = bytes;
    }
    if (lane_id() == 0) {
        if (a_bad) atomicAdd(&ctl[MD_BAD], a_bad);
        if (a_mism) atomicAdd(&ctl[MD_MISM], a_mism);
        if (a_del) atomicAdd(&ctl[MD_DEL], a_del);
        if (a_longest) atomicMax(&ctl[MD_LONGEST], a_longest);
    }
}

// offs: the scanned sizes, offs[items] <= the capacity of md (the host has looked).  An item whose string is empty is bad or
// has no ops; every other one went through md_open<true> in the count pass.
__global__ __launch_bounds__(MD_THREADS) void k_md_emit(MdIn in, const uint64_t *__restrict__ offs, uint8_t *md, uint64_t *__restrict__ md_index,
                                                       uint32_t *__restrict__ md_counts)
{
    for (uint64_t g = (uint64_t)blockIdx.x * MD_THREADS + threadIdx.x; g <= in.items; g += (uint64_t)gridDim.x * MD_THREADS)
        md_index[g] = md_ld64(offs + g);
    const uint64_t waves = (uint64_t)gridDim.x * MD_WAVES;
    for (uint64_t h = (uint64_t)blockIdx.x * MD_WAVES + (threadIdx.x >> 6); h < in.items; h += waves) {
        const uint64_t at = md_ld64(offs + h), end = md_ld64(offs + h + 1);
        uint32_t mism = 0, del = 0;
        MdItem it;
        if (end > at && md_open<false>(in, h, it) == MD_WALK) (void)md_walk<true>(in, it, md + at, mism, del);
        if (md_counts && lane_id() == 0) {
            md_st32(md_counts + 2 * h, mism);
            md_st32(md_counts + 2 * h + 1, del);
        }
    }
}

struct MdArgs {
    const uint8_t *text;
    uint64_t n;
    const uint8_t *reads;
    const uint64_t *read_index;
    uint64_t Q;
    int both;
    const kiss_hip_aln *alns;
    const uint64_t *chain_index;
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const kiss_hip_hit *hits;
    uint64_t H;
    uint8_t *md;
    uint64_t *md_index;
    uint32_t *md_counts;
    uint64_t md_capacity;
};

int md_args_check(const MdArgs &a)
{
    if (!a.text || !a.reads || !a.read_index || !a.alns || !a.chain_index || !a.cigar || !a.cigar_index || !a.md_index) return KISS_HIP_E_INVALID;
    if (a.md_capacity && !a.md) return KISS_HIP_E_INVALID;
    if (a.n > KISS_HIP_MAX_N || a.Q >= (1ull << 31) || (a.both && 2 * a.Q >= (1ull << 31))) return KISS_HIP_E_UNSUPPORTED;
    if (a.hits && a.H > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int md_zero_items(kiss_hip_ctx *ctx, uint64_t *md_index)
{
    KTRY(kiss_zero_u32(ctx, md_index, 2));
    KCHECK(hipStreamSynchronize(ctx->stream));
    return KISS_HIP_OK;
}

int md_steps(kiss_hip_ctx *ctx, const MdArgs &a, kiss_hip_md_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t V = a.both ? 2 * a.Q : a.Q;
    FmCtl<MD_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_MD_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    const dim3 threads(MD_THREADS);
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_md_head, dim3(fm_grid((V > a.Q ? V : a.Q) + 1, MD_THREADS)), threads, 0, ctx->stream, a.chain_index, V, a.read_index, a.Q,
                       d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[MD_BADIN]) return KISS_HIP_E_INVALID; // an index out of order, a read of length 0
    const uint64_t C = h[MD_C1] - h[MD_C0];
    const uint64_t items = a.hits ? a.H : C;
    rep.items = items;
    if (items > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (items == 0) return md_zero_items(ctx, a.md_index);
    if ((items + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    DevBuf slab;
    KTRY(slab.take(ctx, FM_SLOT_MD_SLAB, (items + 1) * 8));
    uint64_t *const size = (uint64_t *)slab.p; // (scanned in place)
    const MdIn in{a.text, a.n, a.reads, a.read_index, a.both, a.alns, a.chain_index, V, h[MD_C0], C, a.cigar, a.cigar_index, a.hits, items};
    const uint64_t blocks = div_up(items, MD_WAVES);
    const dim3 grid((unsigned)(blocks < MD_MAX_BLOCKS ? blocks : MD_MAX_BLOCKS));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, items);
        if (C) hipLaunchKernelGGL(k_md_check_ops, dim3(fm_grid(C, MD_THREADS)), threads, 0, ctx->stream, a.cigar_index, C, d_ctl);
        hipLaunchKernelGGL(k_md_count, grid, threads, 0, ctx->stream, in, size, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, size, size, items + 1));
    uint64_t total = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total, size + items, 8, hipMemcpyDeviceToHost, ctx->stream));
    ev.mark(1);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_count = ev.ms(0, 1);
    if (h[MD_BADIN]) return KISS_HIP_E_INVALID; // a cigar index decreases
    rep.bad = h[MD_BAD];
    rep.md_bytes = total;
    rep.mismatch_columns = h[MD_MISM];
    rep.deleted_bases = h[MD_DEL];
    rep.longest = h[MD_LONGEST];
    // (the totals are in the report: the caller's second call)
    if (a.md_capacity < total) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, items);
        hipLaunchKernelGGL(k_md_emit, grid, threads, 0, ctx->stream, in, (const uint64_t *)size, a.md, a.md_index, a.md_counts);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_emit = ev.ms(1, 2);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_md_dev(kiss_hip_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q,
                        int both_strands, const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar,
                        const uint64_t *cigar_index, const kiss_hip_hit *hits, uint64_t H, uint8_t *md, uint64_t *md_index,
                        uint32_t *md_counts, uint64_t md_capacity, kiss_hip_md_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_md_report rep{};
    if (report) *report = rep;
    const MdArgs a{text, n, reads, read_index, Q, both_strands ? 1 : 0, alns, chain_index, cigar, cigar_index, hits, hits ? H : 0, md, md_index,
                   md_counts, md_capacity};
    KTRY(md_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    int rc = md_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_fmi_md_host(const uint8_t *text, uint64_t n, const uint8_t *reads, const uint64_t *read_index, uint64_t Q, int both_strands,
                         const kiss_hip_aln *alns, const uint64_t *chain_index, const uint32_t *cigar, const uint64_t *cigar_index,
                         const kiss_hip_hit *hits, uint64_t H, uint8_t *md, uint64_t *md_index, uint32_t *md_counts, uint64_t md_capacity,
                         kiss_hip_md_report *report, int device)
{
    if (report) *report = kiss_hip_md_report{};
    const MdArgs a{text, n, reads, read_index, Q, both_strands ? 1 : 0, alns, chain_index, cigar, cigar_index, hits, hits ? H : 0, md, md_index,
                   md_counts, md_capacity};
    KTRY(md_args_check(a));
    const uint64_t V = both_strands ? 2 * Q : Q;
    if (!fm_index_ascending(read_index, Q, true) || !fm_index_ascending(chain_index, V, false)) return KISS_HIP_E_INVALID;
    const uint64_t C = chain_index[V] - chain_index[0];
    if (!fm_index_ascending(cigar_index, C, false)) return KISS_HIP_E_INVALID;
    const uint64_t items = hits ? H : C;
    if (report) report->items = items;
    if (items > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (items == 0) {
        md_index[0] = 0;
        return KISS_HIP_OK;
    }
    // (the ops are uploaded from the first one the alignments use, their index from 0)
    std::vector<uint64_t> oi(C + 1);
    for (uint64_t i = 0; i <= C; i++) oi[i] = cigar_index[i] - cigar_index[0];
    return kiss_one_shot_cached(device, fm_host_max_n(0, items + 1), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *dtext = st.up(text, n), *dreads = st.up(reads, read_index[Q]);
        const uint64_t *dridx = st.up(read_index, (Q + 1) * 8), *dcidx = st.up(chain_index, (V + 1) * 8);
        const kiss_hip_aln *dalns = st.up(alns, C * sizeof(kiss_hip_aln));
        const uint32_t *dcig = st.up(cigar + cigar_index[0], oi[C] * 4);
        const uint64_t *doidx = st.up(oi.data(), (C + 1) * 8);
        const kiss_hip_hit *dhits = st.up(hits, H * sizeof(kiss_hip_hit));
        uint64_t *dmidx = st.room<uint64_t>(true, (items + 1) * 8);
        uint32_t *dcnt = st.room<uint32_t>(md_counts != nullptr, items * 8);
        if (st.rc) return st.rc;
        // the sizing call first: the room on the device is the total, whatever capacity the caller names
        kiss_hip_md_report r{};
        int rc = kiss_hip_fmi_md_dev(ctx, dtext, n, dreads, dridx, Q, both_strands, dalns, dcidx, dcig, doidx, dhits, H, nullptr, dmidx, dcnt, 0, &r,
                                     nullptr);
        uint8_t *dmd = nullptr;
        if (rc == KISS_HIP_E_INVALID && r.md_bytes && r.md_bytes <= md_capacity) {
            dmd = st.room<uint8_t>(true, r.md_bytes);
            if (st.rc) return st.rc;
            rc = kiss_hip_fmi_md_dev(ctx, dtext, n, dreads, dridx, Q, both_strands, dalns, dcidx, dcig, doidx, dhits, H, dmd, dmidx, dcnt, r.md_bytes,
                                     &r, nullptr);
        }
        if (report) *report = r;
        if (rc) return rc;
        st.down(md, dmd, r.md_bytes);
        st.down(md_index, dmidx, (items + 1) * 8);
        if (md_counts) st.down(md_counts, dcnt, items * 8);
        return st.rc;
    });
}

} // extern "C"
