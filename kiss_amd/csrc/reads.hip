// reads.hip -- files of reads (one per line, or FASTQ) -> base codes, qualities, read index and name spans, parsed on the GPU
// (kiss_hip_reads_parse_*), and two parsed batches interleaved into the mates of pairs (kiss_hip_reads_interleave_*).
//
// The reference has no such function; the definition is in include/kiss_hip_reads.h and restated in tests/reads_model.py.  The
// LINES format is kiss_cli::read_file (host/cli_format.hpp) bit for bit.  The host only moves raw bytes.
//
// A TILE is 4096 bytes of the file, cut at multiples of 4096 of the ADDRESS rounded down to 16 (h = address & 15 bytes of the
// first tile lie in front of the file): a lane owns 16 consecutive bytes that start at a multiple of 16, and fetches them with one
// 16-byte load where all 16 are bytes of the file, byte by byte in the group at either end.
//
//   lines : k_rd_count     per tile: the '\n's                                              -> scan over the tiles
//           k_rd_lines     the line starts compacted by newline rank: lstart[r + 1] = the byte behind '\n' number r
//   reads : LINES  k_rd_line_flags  one lane per line: is it a read                         -> scan: the read of a line
//                  k_rd_line_reads  one lane per line: the length and the line of its read  -> u64 scan: where the reads start
//           FASTQ  k_rd_last_kept   the last line that is not empty
//                  k_rd_records     one lane per record: the four lines held against the form, the length -> u64 scan
//           (the host looks at the totals: bad records, capacities; nothing of the caller's has been written so far)
//   copy  : k_rd_copy      PARALLEL OVER THE BYTES of the file: a lane knows the line its first byte lies in from the scanned
//                          counts, and for every line it walks through which read it is and where that read starts; a byte of a
//                          sequence line is translated, one of a quality line copied, to where it belongs.  A read of 300 000
//                          bases is the work of 18 750 lanes.
//           k_rd_finish    one lane per read: read_index, the span of the name
//   part  : kiss_hip_reads_parse_part_* (kiss_hip_reads_part.h): the lines passes over a chunk, the records its
//           complete lines hold, the boundary picked (FASTQ: line start 4 * records; LINES: k_rd_cut_line), then the passes
//           above over the prefix
#include "fm_internal.hpp"
#include "../../include/kiss_hip_reads_part.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_PER = 16;
constexpr int RD_TILE = RD_THREADS * RD_PER; // 4096 bytes per workgroup

// control block of a call (u64 words)
enum { RD_FIRST = 0, RD_LAST = 1, RD_NL = 2, RD_READS = 3, RD_BASES = 4, RD_KEPT = 5, RD_BAD = 6, RD_FIRST_BAD = 7, RD_EMPTY = 8, RD_FIRST_EMPTY = 9,
       RD_NOBASE = 10, IL_BAD = 11, IL_TOTAL_A = 12, IL_TOTAL_B = 13, RD_CUT = 14, RD_CTL_WORDS = 16 };

// Every load of an index or table entry starts at a multiple of its own size: relaxed loads of wavefront scope, as in
// fm_pair.hip -- ordinary global_load_dword / _dwordx2 that the compiler does not merge with their neighbours (lstart[k] and
// lstart[k + 1], idx[q] and idx[q + 1]) into one wider load at an address that is only 4- or 8-byte aligned.
__device__ __forceinline__ uint32_t rd_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t rd_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__global__ void k_rd_ctl_init(unsigned long long *__restrict__ ctl)
{
    if (threadIdx.x < RD_CTL_WORDS) ctl[threadIdx.x] = (threadIdx.x == RD_FIRST_BAD || threadIdx.x == RD_FIRST_EMPTY) ? ~0ull : 0ull;
}

// the 16 bytes of a lane: file offsets i0 .. i0 + 15 (i0 may be negative in the first group), `valid` = which of them are bytes of
// the file.  One 16-byte load only where raw + i0 is a multiple of 16 by construction and all 16 are inside.
struct Bytes16 {
    uint32_t w[4];
    uint32_t valid;
    __device__ __forceinline__ uint32_t at(int e) const { return (w[e >> 2] >> (8 * (e & 3))) & 0xFFu; }
};
__device__ __forceinline__ Bytes16 rd_load16(const uint8_t *__restrict__ raw, uint64_t bytes, long long i0)
{
    Bytes16 b;
    if (i0 >= 0 && (uint64_t)i0 + RD_PER <= bytes) {
        const uint4 q = *reinterpret_cast<const uint4 *>(raw + i0);
        b.w[0] = q.x, b.w[1] = q.y, b.w[2] = q.z, b.w[3] = q.w;
        b.valid = 0xFFFFu;
        return b;
    }
    b.w[0] = b.w[1] = b.w[2] = b.w[3] = 0;
    b.valid = 0;
#pragma unroll
    for (int e = 0; e < RD_PER; e++) {
        const long long i = i0 + e;
        if (i >= 0 && (uint64_t)i < bytes) {
            b.w[e >> 2] |= (uint32_t)raw[i] << (8 * (e & 3));
            b.valid |= 1u << e;
        }
    }
    return b;
}
__device__ __forceinline__ uint32_t rd_newlines(const Bytes16 &b)
{
    uint32_t n = 0;
#pragma unroll
    for (int e = 0; e < RD_PER; e++) n += ((b.valid >> e) & 1u) && b.at(e) == '\n';
    return n;
}
// the file offset of the first byte of lane `threadIdx.x` of tile `blockIdx.x`; h = address of raw & 15
__device__ __forceinline__ long long rd_lane_offset(uint32_t h)
{
    return (long long)((uint64_t)blockIdx.x * RD_TILE + (uint64_t)threadIdx.x * RD_PER) - (long long)h;
}

__device__ __forceinline__ uint32_t rd_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// exclusive prefix of v over the lanes of a workgroup
__device__ __forceinline__ uint32_t rd_block_excl(uint32_t v, uint32_t *ws)
{
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if ((int)lane_id() >= d) inc += o;
    }
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t ex = inc - v;
    for (int w = 0; w < wave; w++) ex += ws[w];
    __syncthreads();
    return ex;
}

// per tile: the '\n's; tile `tiles` (one workgroup more than there are tiles): 0, so that the scan's last entry is the total.
// The first and the last byte of the file go to the control block.
__global__ __launch_bounds__(RD_THREADS) void k_rd_count(const uint8_t *__restrict__ raw, uint64_t bytes, uint32_t h, uint32_t *__restrict__ tile_nl,
                                                        unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t ws[RD_THREADS / 64];
    const long long i0 = rd_lane_offset(h);
    const Bytes16 b = rd_load16(raw, bytes, i0);
    const uint32_t nl = rd_wave_sum(rd_newlines(b));
    if (lane_id() == 0) ws[threadIdx.x >> 6] = nl;
#pragma unroll
    for (int e = 0; e < RD_PER; e++) {
        if (i0 + e == 0) ctl[RD_FIRST] = b.at(e);
        if ((uint64_t)(i0 + e) + 1 == bytes) ctl[RD_LAST] = b.at(e);
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_nl[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void k_rd_pick32(const uint32_t *__restrict__ src, uint64_t at, unsigned long long *__restrict__ ctl, int word)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) ctl[word] = src[at];
}
__global__ void k_rd_pick64(const uint64_t *__restrict__ src, uint64_t at, unsigned long long *__restrict__ ctl, int word)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) ctl[word] = src[at];
}

// lstart[0] = 0, lstart[r + 1] = the byte behind newline number r; a last piece without '\n' ends as if one stood at `bytes`:
// lstart[lines] = bytes + 1.  So line k is [lstart[k], lstart[k + 1] - 1) whatever ends it.
__global__ __launch_bounds__(RD_THREADS) void k_rd_lines(const uint8_t *__restrict__ raw, uint64_t bytes, uint32_t h, const uint32_t *__restrict__ nl_ex,
                                                        uint64_t lines, int open_end, uint32_t *__restrict__ lstart)
{
    __shared__ uint32_t ws[RD_THREADS / 64];
    const long long i0 = rd_lane_offset(h);
    const Bytes16 b = rd_load16(raw, bytes, i0);
    uint64_t rank = (uint64_t)nl_ex[blockIdx.x] + rd_block_excl(rd_newlines(b), ws);
#pragma unroll
    for (int e = 0; e < RD_PER; e++)
        if (((b.valid >> e) & 1u) && b.at(e) == '\n') {
            rank++;
            if (rank <= lines) lstart[rank] = (uint32_t)(i0 + e + 1); // (rank <= lines by construction: the bound costs nothing)
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lstart[0] = 0;
        if (open_end) lstart[lines] = (uint32_t)(bytes + 1);
    }
}

// line k after the '\r' strip: [beg, end)
struct Line {
    uint32_t beg, end;
    __device__ __forceinline__ bool empty() const { return end == beg; }
};
__device__ __forceinline__ Line rd_line(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart, uint64_t k)
{
    Line l;
    l.beg = rd_ld32(lstart + k);
    l.end = rd_ld32(lstart + k + 1) - 1u;
    if (l.end > l.beg && raw[l.end - 1] == '\r') l.end--;
    return l;
}
// the name behind the first byte of a header line: up to the first space, tab or line end
__device__ __forceinline__ uint32_t rd_name_len(const uint8_t *__restrict__ raw, const Line &l)
{
    uint32_t j = l.beg + 1;
    while (j < l.end && raw[j] != ' ' && raw[j] != '\t') j++;
    return j - (l.beg + 1);
}

// LINES: flag[k] = line k is a read (flag[lines] = 0: the scan's last entry is the number of reads)
__global__ __launch_bounds__(RD_THREADS) void k_rd_line_flags(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart, uint64_t lines,
                                                             uint32_t *__restrict__ flag)
{
    const uint64_t k = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (k > lines) return;
    uint32_t f = 0;
    if (k < lines) {
        const Line l = rd_line(raw, lstart, k);
        f = !l.empty() && raw[l.beg] != '>';
    }
    flag[k] = f;
}
// LINES: rank = the scanned flags; the read of a line gets its length and its line
__global__ __launch_bounds__(RD_THREADS) void k_rd_line_reads(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart, uint64_t lines,
                                                             const uint32_t *__restrict__ rank, uint64_t reads, uint64_t *__restrict__ len,
                                                             uint32_t *__restrict__ line_of)
{
    const uint64_t k = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (k == 0) len[reads] = 0;
    if (k >= lines) return;
    const uint32_t q = rd_ld32(rank + k);
    if (rd_ld32(rank + k + 1) == q || q >= reads) return;
    const Line l = rd_line(raw, lstart, k);
    len[q] = l.end - l.beg;
    line_of[q] = (uint32_t)k;
}

// LINES, the cut of a chunk: the byte behind read line number `records` >= 1 (rank = the scanned flags)
__global__ __launch_bounds__(RD_THREADS) void k_rd_cut_line(const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ rank, uint64_t lines,
                                                           uint64_t records, unsigned long long *__restrict__ ctl)
{
    const uint64_t k = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (k >= lines) return;
    if ((uint64_t)rd_ld32(rank + k) + 1 == records && (uint64_t)rd_ld32(rank + k + 1) == records) ctl[RD_CUT] = rd_ld32(lstart + k + 1);
}

// FASTQ: the number of lines up to the last one that is not empty
__global__ __launch_bounds__(RD_THREADS) void k_rd_last_kept(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart, uint64_t lines,
                                                            unsigned long long *__restrict__ ctl)
{
    const uint64_t k = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    const bool kept = k < lines && !rd_line(raw, lstart, k).empty();
    const unsigned long long m = __ballot(kept);
    if (m && lane_id() == 63u - (uint32_t)__builtin_clzll(m)) atomicMax(&ctl[RD_KEPT], (unsigned long long)(k + 1));
}
// FASTQ: record r = lines 4 r .. 4 r + 3 of the `kept` first lines
__global__ __launch_bounds__(RD_THREADS) void k_rd_records(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart, uint64_t kept,
                                                          uint64_t records, uint64_t *__restrict__ len, unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (r == 0) len[records] = 0;
    if (r >= records) return;
    uint32_t kind = 0;
    uint64_t L = 0;
    if (4 * r + 4 > kept) {
        kind = KISS_HIP_READS_BAD_TRUNCATED;
    } else {
        const Line name = rd_line(raw, lstart, 4 * r), seq = rd_line(raw, lstart, 4 * r + 1), plus = rd_line(raw, lstart, 4 * r + 2),
                   qual = rd_line(raw, lstart, 4 * r + 3);
        L = seq.end - seq.beg;
        if (name.empty() || raw[name.beg] != '@') kind = KISS_HIP_READS_BAD_NO_AT;
        else if (plus.empty() || raw[plus.beg] != '+') kind = KISS_HIP_READS_BAD_NO_PLUS;
        else if (qual.end - qual.beg != seq.end - seq.beg) kind = KISS_HIP_READS_BAD_LENGTHS;
    }
    len[r] = kind ? 0 : L;
    if (kind) {
        atomicAdd(&ctl[RD_BAD], 1ull);
        atomicMin(&ctl[RD_FIRST_BAD], (unsigned long long)(r * 8 + kind));
    } else if (L == 0) {
        atomicAdd(&ctl[RD_EMPTY], 1ull);
        atomicMin(&ctl[RD_FIRST_EMPTY], (unsigned long long)r);
    }
}

__device__ __forceinline__ uint32_t rd_code(uint32_t c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4; // no base
    }
}

// what a lane knows of the line it walks through: where it starts, where its bytes go (out == nullptr: nowhere), how many of them
struct Dest {
    uint8_t *out;
    uint64_t len;
    uint32_t beg;
    bool translate;
};
template <bool FASTQ>
__device__ __forceinline__ Dest rd_dest(uint64_t k, uint64_t used_lines, const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ rank,
                                        const uint64_t *__restrict__ idx, uint64_t reads, uint8_t *codes, uint8_t *qual)
{
    Dest d{nullptr, 0, 0, true};
    if (k >= used_lines) return d;
    uint64_t q;
    if (FASTQ) {
        if (!(k & 1ull)) return d; // the '@' and the '+' line
        q = k >> 2;
        d.translate = !(k & 2ull);
        if (!d.translate && !qual) return d;
    } else {
        q = rd_ld32(rank + k);
        if (rd_ld32(rank + k + 1) == q) return d;
    }
    if (q >= reads) return d;
    const uint64_t at = rd_ld64(idx + q);
    d.len = rd_ld64(idx + q + 1) - at;
    d.beg = rd_ld32(lstart + k);
    d.out = (d.translate ? codes : qual) + at;
    return d;
}

// the copy pass: every byte of a sequence line translated to its place in codes, every byte of a quality line copied to its
// place in qual.  idx[reads] <= the capacity of both (the host has looked), off < len keeps a store inside its read.
template <bool FASTQ>
__global__ __launch_bounds__(RD_THREADS) void k_rd_copy(const uint8_t *__restrict__ raw, uint64_t bytes, uint32_t h, const uint32_t *__restrict__ nl_ex,
                                                       uint64_t used_lines, const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ rank,
                                                       const uint64_t *__restrict__ idx, uint64_t reads, uint8_t *codes, uint8_t *qual,
                                                       unsigned long long *__restrict__ ctl)
{
    __shared__ uint32_t ws[RD_THREADS / 64];
    const long long i0 = rd_lane_offset(h);
    const Bytes16 b = rd_load16(raw, bytes, i0);
    uint64_t k = (uint64_t)nl_ex[blockIdx.x] + rd_block_excl(rd_newlines(b), ws);
    uint32_t no_base = 0;
    if (b.valid) {
        Dest d = rd_dest<FASTQ>(k, used_lines, lstart, rank, idx, reads, codes, qual);
#pragma unroll
        for (int e = 0; e < RD_PER; e++) {
            if (!((b.valid >> e) & 1u)) continue;
            const uint32_t c = b.at(e);
            if (c == '\n') {
                k++;
                d = rd_dest<FASTQ>(k, used_lines, lstart, rank, idx, reads, codes, qual);
                continue;
            }
            if (!d.out) continue;
            const uint64_t off = (uint64_t)(i0 + e) - d.beg;
            if (off >= d.len) continue; // (the '\r' of the line end)
            if (d.translate) {
                const uint32_t code = rd_code(c);
                d.out[off] = (uint8_t)code;
                no_base += code == 4u;
            } else {
                d.out[off] = (uint8_t)c;
            }
        }
    }
    no_base = rd_wave_sum(no_base);
    if (no_base && lane_id() == 0) atomicAdd(&ctl[RD_NOBASE], (unsigned long long)no_base);
}

// one lane per read (and one more): read_index, the span of the name
template <bool FASTQ>
__global__ __launch_bounds__(RD_THREADS) void k_rd_finish(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ lstart,
                                                         const uint32_t *__restrict__ line_of, const uint64_t *__restrict__ idx, uint64_t reads,
                                                         uint64_t *__restrict__ read_index, uint64_t *__restrict__ name_off,
                                                         uint32_t *__restrict__ name_len)
{
    const uint64_t q = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (q > reads) return;
    read_index[q] = rd_ld64(idx + q);
    if (q == reads || !name_off) return;
    uint64_t off = 0;
    uint32_t n = 0;
    const uint64_t k = FASTQ ? 4 * q + 1 : line_of[q]; // the line of the read: its header is the line in front of it
    if (k > 0) {
        const Line l = rd_line(raw, lstart, k - 1);
        if (!l.empty() && raw[l.beg] == (FASTQ ? '@' : '>')) {
            off = (uint64_t)l.beg + 1;
            n = rd_name_len(raw, l);
        }
    }
    name_off[q] = off;
    name_len[q] = n;
}

int pick32(kiss_hip_ctx *ctx, const uint32_t *src, uint64_t at, unsigned long long *ctl, int word)
{
    hipLaunchKernelGGL(k_rd_pick32, dim3(1), dim3(64), 0, ctx->stream, src, at, ctl, word);
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}
int pick64(kiss_hip_ctx *ctx, const uint64_t *src, uint64_t at, unsigned long long *ctl, int word)
{
    hipLaunchKernelGGL(k_rd_pick64, dim3(1), dim3(64), 0, ctx->stream, src, at, ctl, word);
    KCHECK(hipGetLastError());
    return KISS_HIP_OK;
}

struct ParseArgs {
    const uint8_t *raw;
    uint64_t bytes;
    int format;
    uint8_t *codes, *qual;
    uint64_t bases_capacity;
    uint64_t *read_index, *name_off;
    uint32_t *name_len;
    uint64_t reads_capacity;
    kiss_hip_reads_report *report;
    bool no_drop = false; // FASTQ: the prefix of a chunk, every line of it a line of a record (kiss_hip_reads_part.h)
};

int parse_steps(kiss_hip_ctx *ctx, const ParseArgs &a, kiss_hip_reads_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint8_t *raw = a.raw;
    const uint64_t bytes = a.bytes;
    const uint32_t h = (uint32_t)((uintptr_t)raw & 15u);
    const uint64_t tiles = div_up(bytes + h, RD_TILE);
    const dim3 threads(RD_THREADS);
    FmCtl<RD_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_READS_CTL));
    unsigned long long *const d_ctl = ctl.d, *const hc = ctl.h;
    DevBuf tile_buf, line_buf, index_buf;
    KTRY(tile_buf.take(ctx, FM_SLOT_READS_TILES, (tiles + 1) * 4));
    uint32_t *const nl_ex = (uint32_t *)tile_buf.p; // (the counts, scanned in place)

    // ---- lines
    ev.mark(0);
    hipLaunchKernelGGL(k_rd_ctl_init, dim3(1), dim3(64), 0, ctx->stream, d_ctl);
    {
        KTimer t(ctx, KISS_HIP_K_PACK, bytes);
        hipLaunchKernelGGL(k_rd_count, dim3((unsigned)(tiles + 1)), threads, 0, ctx->stream, raw, bytes, h, nl_ex, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u32(ctx, nl_ex, nl_ex, tiles + 1));
    KTRY(pick32(ctx, nl_ex, tiles, d_ctl, RD_NL));
    KTRY(ctl.fetch_sync());
    const int open_end = hc[RD_LAST] != (unsigned long long)'\n';
    const uint64_t lines = hc[RD_NL] + (uint64_t)open_end;
    const bool fastq = a.format == KISS_HIP_READS_FASTQ || (a.format == KISS_HIP_READS_AUTO && hc[RD_FIRST] == (unsigned long long)'@');
    rep.format = fastq ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_LINES;
    rep.has_qual = fastq ? 1u : 0u;
    rep.lines = lines;
    if (lines > bytes) return KINTERNAL();
    FmSlab lay;
    const uint64_t o_lstart = lay.carve((lines + 1) * 4), o_rank = lay.carve((lines + 1) * 4);
    KTRY(line_buf.take(ctx, FM_SLOT_READS_LINES, lay.size));
    uint32_t *const lstart = (uint32_t *)((char *)line_buf.p + o_lstart), *const rank = (uint32_t *)((char *)line_buf.p + o_rank);
    {
        KTimer t(ctx, KISS_HIP_K_PACK, bytes);
        hipLaunchKernelGGL(k_rd_lines, dim3((unsigned)tiles), threads, 0, ctx->stream, raw, bytes, h, nl_ex, lines, open_end, lstart);
        KCHECK(hipGetLastError());
    }
    ev.mark(1);

    // ---- reads
    uint64_t reads = 0, used_lines = lines;
    if (fastq && a.no_drop) {
        if (lines % 4) return KINTERNAL();
        reads = lines / 4;
    } else if (fastq) {
        if (lines) hipLaunchKernelGGL(k_rd_last_kept, dim3(fm_grid(lines, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, lines, d_ctl);
        KCHECK(hipGetLastError());
        KTRY(ctl.fetch_sync());
        used_lines = hc[RD_KEPT];
        if (used_lines > lines) return KINTERNAL();
        reads = div_up(used_lines, 4);
    } else {
        hipLaunchKernelGGL(k_rd_line_flags, dim3(fm_grid(lines + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, lines, rank);
        KCHECK(hipGetLastError());
        KTRY(kiss_scan_u32(ctx, rank, rank, lines + 1));
        KTRY(pick32(ctx, rank, lines, d_ctl, RD_READS));
        KTRY(ctl.fetch_sync());
        reads = hc[RD_READS];
        if (reads > lines) return KINTERNAL();
    }
    FmSlab ilay;
    const uint64_t o_idx = ilay.carve((reads + 1) * 8), o_line_of = ilay.carve((reads + 1) * 4);
    KTRY(index_buf.take(ctx, FM_SLOT_READS_INDEX, ilay.size));
    uint64_t *const idx = (uint64_t *)((char *)index_buf.p + o_idx); // (the lengths, scanned in place)
    uint32_t *const line_of = (uint32_t *)((char *)index_buf.p + o_line_of);
    if (fastq)
        hipLaunchKernelGGL(k_rd_records, dim3(fm_grid(reads + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, used_lines, reads, idx, d_ctl);
    else
        hipLaunchKernelGGL(k_rd_line_reads, dim3(fm_grid(lines + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, lines, rank, reads, idx, line_of);
    KCHECK(hipGetLastError());
    KTRY(kiss_scan_u64(ctx, idx, idx, reads + 1));
    KTRY(pick64(ctx, idx, reads, d_ctl, RD_BASES));
    ev.mark(2);
    KTRY(ctl.fetch_sync());
    rep.ms_lines = ev.ms(0, 1);
    rep.ms_reads = ev.ms(1, 2);
    if (hc[RD_BAD]) { // the outputs are untouched
        rep.bad_records = hc[RD_BAD];
        rep.first_bad = hc[RD_FIRST_BAD] >> 3;
        rep.first_bad_kind = (uint32_t)(hc[RD_FIRST_BAD] & 7u);
        return KISS_HIP_E_INVALID;
    }
    const uint64_t bases = hc[RD_BASES];
    rep.reads = reads;
    rep.bases = bases;
    rep.empty_reads = hc[RD_EMPTY];
    rep.first_empty = hc[RD_FIRST_EMPTY];
    if (bases > bytes) return KINTERNAL();
    if (reads > a.reads_capacity || bases > a.bases_capacity) return KISS_HIP_E_INVALID; // size, then fill

    // ---- copy
    {
        KTimer t(ctx, KISS_HIP_K_PACK, bytes);
        uint8_t *const qual = fastq ? a.qual : nullptr;
        if (bases && fastq)
            hipLaunchKernelGGL((k_rd_copy<true>), dim3((unsigned)tiles), threads, 0, ctx->stream, raw, bytes, h, nl_ex, used_lines, lstart, rank, idx,
                               reads, a.codes, qual, d_ctl);
        else if (bases)
            hipLaunchKernelGGL((k_rd_copy<false>), dim3((unsigned)tiles), threads, 0, ctx->stream, raw, bytes, h, nl_ex, used_lines, lstart, rank, idx,
                               reads, a.codes, qual, d_ctl);
        if (fastq)
            hipLaunchKernelGGL((k_rd_finish<true>), dim3(fm_grid(reads + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, line_of, idx, reads,
                               a.read_index, a.name_off, a.name_len);
        else
            hipLaunchKernelGGL((k_rd_finish<false>), dim3(fm_grid(reads + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, line_of, idx, reads,
                               a.read_index, a.name_off, a.name_len);
        KCHECK(hipGetLastError());
    }
    ev.mark(3);
    KTRY(ctl.fetch_sync());
    rep.no_base = hc[RD_NOBASE];
    rep.ms_copy = ev.ms(2, 3);
    return KISS_HIP_OK;
}

int parse_args_check(const ParseArgs &a)
{
    if (!a.read_index || (a.bytes && !a.raw)) return KISS_HIP_E_INVALID;
    if (a.format != KISS_HIP_READS_AUTO && a.format != KISS_HIP_READS_LINES && a.format != KISS_HIP_READS_FASTQ) return KISS_HIP_E_INVALID;
    if ((a.name_off == nullptr) != (a.name_len == nullptr)) return KISS_HIP_E_INVALID;
    if (a.bases_capacity && !a.codes) return KISS_HIP_E_INVALID;
    if (a.bytes > KISS_HIP_READS_MAX_BYTES) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}
kiss_hip_reads_report empty_report(int format)
{
    kiss_hip_reads_report r{};
    r.format = format == KISS_HIP_READS_FASTQ ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_LINES;
    r.has_qual = r.format == KISS_HIP_READS_FASTQ ? 1u : 0u;
    r.first_empty = r.first_bad = KISS_HIP_READS_NONE;
    return r;
}

// ---- the first whole records of a chunk (kiss_hip_reads_part.h) ----------------------------------------------------------------
// The cut runs the line passes of the parse over the chunk, counts the records its complete lines hold and picks the byte behind
// the last one it takes; the parse then runs on that prefix as on a file of its own (no_drop: without looking for empty lines at
// its end).  The line passes run twice over the prefix so; DESIGN.md 4.20 has what that costs.
struct Cut {
    bool fastq = false, whole = false; // whole: the end of the file and every record taken -- the prefix is parsed as a file is
    uint64_t complete = 0, records = 0, used = 0;
};

int cut_steps(kiss_hip_ctx *ctx, const uint8_t *raw, uint64_t bytes, int format, bool final, uint64_t max_records, Cut &cut)
{
    kiss_opts_refresh(ctx);
    const uint32_t h = (uint32_t)((uintptr_t)raw & 15u);
    const uint64_t tiles = div_up(bytes + h, RD_TILE);
    const dim3 threads(RD_THREADS);
    FmCtl<RD_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_READS_CTL));
    unsigned long long *const d_ctl = ctl.d, *const hc = ctl.h;
    DevBuf tile_buf, line_buf;
    KTRY(tile_buf.take(ctx, FM_SLOT_READS_TILES, (tiles + 1) * 4));
    uint32_t *const nl_ex = (uint32_t *)tile_buf.p;
    hipLaunchKernelGGL(k_rd_ctl_init, dim3(1), dim3(64), 0, ctx->stream, d_ctl);
    {
        KTimer t(ctx, KISS_HIP_K_PACK, bytes);
        hipLaunchKernelGGL(k_rd_count, dim3((unsigned)(tiles + 1)), threads, 0, ctx->stream, raw, bytes, h, nl_ex, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u32(ctx, nl_ex, nl_ex, tiles + 1));
    KTRY(pick32(ctx, nl_ex, tiles, d_ctl, RD_NL));
    KTRY(ctl.fetch_sync());
    // the complete lines: a last piece without '\n' is one only at the end of the file
    const int open_end = final && hc[RD_LAST] != (unsigned long long)'\n';
    const uint64_t lines = hc[RD_NL] + (uint64_t)open_end;
    cut.fastq = format == KISS_HIP_READS_FASTQ || (format == KISS_HIP_READS_AUTO && hc[RD_FIRST] == (unsigned long long)'@');
    if (lines > bytes) return KINTERNAL();
    FmSlab lay;
    const uint64_t o_lstart = lay.carve((lines + 1) * 4), o_rank = lay.carve((lines + 1) * 4);
    KTRY(line_buf.take(ctx, FM_SLOT_READS_LINES, lay.size));
    uint32_t *const lstart = (uint32_t *)((char *)line_buf.p + o_lstart), *const rank = (uint32_t *)((char *)line_buf.p + o_rank);
    {
        KTimer t(ctx, KISS_HIP_K_PACK, bytes);
        hipLaunchKernelGGL(k_rd_lines, dim3((unsigned)tiles), threads, 0, ctx->stream, raw, bytes, h, nl_ex, lines, open_end, lstart);
        KCHECK(hipGetLastError());
    }
    if (cut.fastq) {
        if (lines) hipLaunchKernelGGL(k_rd_last_kept, dim3(fm_grid(lines, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, lines, d_ctl);
        KCHECK(hipGetLastError());
        KTRY(ctl.fetch_sync());
        const uint64_t kept = hc[RD_KEPT];
        if (kept > lines) return KINTERNAL();
        cut.complete = final ? div_up(kept, 4) : kept / 4;
    } else {
        hipLaunchKernelGGL(k_rd_line_flags, dim3(fm_grid(lines + 1, RD_THREADS)), threads, 0, ctx->stream, raw, lstart, lines, rank);
        KCHECK(hipGetLastError());
        KTRY(kiss_scan_u32(ctx, rank, rank, lines + 1));
        KTRY(pick32(ctx, rank, lines, d_ctl, RD_READS));
        KTRY(ctl.fetch_sync());
        cut.complete = hc[RD_READS];
        if (cut.complete > lines) return KINTERNAL();
    }
    cut.records = max_records && max_records < cut.complete ? max_records : cut.complete;
    cut.whole = final && cut.records == cut.complete;
    cut.used = cut.whole ? bytes : 0;
    if (cut.whole || !cut.records) return KISS_HIP_OK;
    // the byte behind the '\n' of the last line taken (it has one: it is not the last line of the file's end, or not final)
    if (cut.fastq) {
        if (4 * cut.records > lines) return KINTERNAL();
        KTRY(pick32(ctx, lstart, 4 * cut.records, d_ctl, RD_CUT));
    } else {
        hipLaunchKernelGGL(k_rd_cut_line, dim3(fm_grid(lines, RD_THREADS)), threads, 0, ctx->stream, lstart, rank, lines, cut.records, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(ctl.fetch_sync());
    cut.used = hc[RD_CUT];
    if (cut.used == 0 || cut.used > bytes) return KINTERNAL();
    return KISS_HIP_OK;
}

// ---- interleave ------------------------------------------------------------------------------------------------------------
// an index that does not start at 0 or decreases; the totals
__global__ __launch_bounds__(RD_THREADS) void k_il_check(const uint64_t *__restrict__ ia, const uint64_t *__restrict__ ib, uint64_t P,
                                                        unsigned long long *__restrict__ ctl)
{
    const uint64_t p = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    bool bad = false;
    if (p == 0) {
        ctl[IL_TOTAL_A] = rd_ld64(ia + P);
        ctl[IL_TOTAL_B] = rd_ld64(ib + P);
        bad = rd_ld64(ia) != 0 || rd_ld64(ib) != 0;
    }
    if (p < P) bad = bad || rd_ld64(ia + p + 1) < rd_ld64(ia + p) || rd_ld64(ib + p + 1) < rd_ld64(ib + p);
    if (__ballot(bad) && lane_id() == 0) ctl[IL_BAD] = 1;
}
// read 2 p starts where p reads of either batch end, read 2 p + 1 one read of the first batch further
__global__ __launch_bounds__(RD_THREADS) void k_il_index(const uint64_t *__restrict__ ia, const uint64_t *__restrict__ ib, uint64_t P,
                                                        uint64_t *__restrict__ out)
{
    const uint64_t r = (uint64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (r <= 2 * P) out[r] = rd_ld64(ia + ((r + 1) >> 1)) + rd_ld64(ib + (r >> 1));
}
// a lane takes 16 bases of the output: the read of the first one by bisection of the new index, the others by walking on
__global__ __launch_bounds__(RD_THREADS) void k_il_copy(const uint8_t *__restrict__ ca, const uint64_t *__restrict__ ia, const uint8_t *__restrict__ qa,
                                                       const uint8_t *__restrict__ cb, const uint64_t *__restrict__ ib, const uint8_t *__restrict__ qb,
                                                       uint64_t P, const uint64_t *__restrict__ oidx, uint64_t total, uint8_t *__restrict__ codes,
                                                       uint8_t *__restrict__ qual)
{
    const uint64_t j0 = ((uint64_t)blockIdx.x * RD_THREADS + threadIdx.x) * RD_PER;
    if (j0 >= total) return;
    uint64_t lo = 0, hi = 2 * P; // the last read r with oidx[r] <= j0 (oidx[2 P] = total > j0)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rd_ld64(oidx + mid) <= j0) lo = mid;
        else hi = mid;
    }
    uint64_t r = lo, beg = rd_ld64(oidx + r), end = rd_ld64(oidx + r + 1);
    for (int e = 0; e < RD_PER; e++) {
        const uint64_t j = j0 + e;
        if (j >= total) break;
        while (j >= end) { // (ends below 2 P: j < total)
            r++;
            beg = end;
            end = rd_ld64(oidx + r + 1);
        }
        const uint64_t s = ((r & 1ull) ? rd_ld64(ib + (r >> 1)) : rd_ld64(ia + (r >> 1))) + (j - beg);
        codes[j] = (r & 1ull) ? cb[s] : ca[s];
        if (qual) qual[j] = (r & 1ull) ? qb[s] : qa[s];
    }
}

struct InterleaveArgs {
    const uint8_t *codes_a;
    const uint64_t *index_a;
    const uint8_t *qual_a;
    uint64_t P_a;
    const uint8_t *codes_b;
    const uint64_t *index_b;
    const uint8_t *qual_b;
    uint64_t P_b;
    uint8_t *codes;
    uint64_t *read_index;
    uint8_t *qual;
    uint64_t bases_capacity, *bases_out;
};

int interleave_args_check(const InterleaveArgs &a)
{
    if (!a.index_a || !a.index_b || !a.read_index) return KISS_HIP_E_INVALID;
    if (a.P_a != a.P_b) return KISS_HIP_E_INVALID;
    const int quals = (a.qual_a ? 1 : 0) + (a.qual_b ? 1 : 0) + (a.qual ? 1 : 0);
    if (quals != 0 && quals != 3) return KISS_HIP_E_INVALID;
    if (a.P_a >= (1ull << 31)) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int interleave_steps(kiss_hip_ctx *ctx, const InterleaveArgs &a)
{
    kiss_opts_refresh(ctx);
    const uint64_t P = a.P_a;
    FmCtl<RD_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_READS_CTL));
    const dim3 threads(RD_THREADS);
    hipLaunchKernelGGL(k_rd_ctl_init, dim3(1), dim3(64), 0, ctx->stream, ctl.d);
    hipLaunchKernelGGL(k_il_check, dim3(fm_grid(P + 1, RD_THREADS)), threads, 0, ctx->stream, a.index_a, a.index_b, P, ctl.d);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (ctl.h[IL_BAD]) return KISS_HIP_E_INVALID;
    const uint64_t total_a = ctl.h[IL_TOTAL_A], total_b = ctl.h[IL_TOTAL_B], total = total_a + total_b;
    if (a.bases_out) *a.bases_out = total;
    if (total > a.bases_capacity || (total && !a.codes) || (total_a && !a.codes_a) || (total_b && !a.codes_b)) return KISS_HIP_E_INVALID;
    KTimer t(ctx, KISS_HIP_K_PACK, total);
    hipLaunchKernelGGL(k_il_index, dim3(fm_grid(2 * P + 1, RD_THREADS)), threads, 0, ctx->stream, a.index_a, a.index_b, P, a.read_index);
    if (total)
        hipLaunchKernelGGL(k_il_copy, dim3(fm_grid(div_up(total, RD_PER), RD_THREADS)), threads, 0, ctx->stream, a.codes_a, a.index_a, a.qual_a,
                           a.codes_b, a.index_b, a.qual_b, P, a.read_index, total, a.codes, a.qual);
    KCHECK(hipGetLastError());
    KCHECK(hipStreamSynchronize(ctx->stream));
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_reads_parse_dev(kiss_hip_ctx *ctx, const uint8_t *d_raw, uint64_t bytes, int format, uint8_t *d_codes, uint8_t *d_qual,
                             uint64_t bases_capacity, uint64_t *d_read_index, uint64_t *d_name_off, uint32_t *d_name_len, uint64_t reads_capacity,
                             kiss_hip_reads_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_reads_report rep = empty_report(format);
    if (report) *report = rep;
    const ParseArgs a{d_raw, bytes, format, d_codes, d_qual, bases_capacity, d_read_index, d_name_off, d_name_len, reads_capacity, report};
    KTRY(parse_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if ((bytes + 2) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    FmEvents ev(ctx, report != nullptr);
    int rc;
    if (bytes == 0) { // no line, no read: the one entry of the index
        rc = kiss_zero_u32(ctx, d_read_index, 2);
        if (rc == KISS_HIP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = KISS_HIP_E_HIP;
    } else {
        rc = parse_steps(ctx, a, rep, ev);
    }
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_reads_parse_host(const uint8_t *raw, uint64_t bytes, int format, uint8_t *codes, uint8_t *qual, uint64_t bases_capacity,
                              uint64_t *read_index, uint64_t *name_off, uint32_t *name_len, uint64_t reads_capacity, kiss_hip_reads_report *report,
                              int device)
{
    if (report) *report = empty_report(format);
    KTRY(parse_args_check(ParseArgs{raw, bytes, format, codes, qual, bases_capacity, read_index, name_off, name_len, reads_capacity, report}));
    return kiss_one_shot_cached(device, fm_host_max_n(0, bytes + 2), [&](kiss_hip_ctx *ctx) -> int {
        const bool names = name_off != nullptr;
        FmStage st(ctx);
        const uint8_t *draw = st.up(raw, bytes);
        uint8_t *dcodes = st.room<uint8_t>(true, bases_capacity);
        uint8_t *dqual = st.room<uint8_t>(qual != nullptr, bases_capacity);
        uint64_t *didx = st.room<uint64_t>(true, (reads_capacity + 1) * 8);
        uint64_t *dnoff = st.room<uint64_t>(names, reads_capacity * 8);
        uint32_t *dnlen = st.room<uint32_t>(names, reads_capacity * 4);
        if (st.rc) return st.rc;
        kiss_hip_reads_report r{};
        const int rc = kiss_hip_reads_parse_dev(ctx, draw, bytes, format, dcodes, dqual, bases_capacity, didx, dnoff, dnlen, reads_capacity, &r,
                                                nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(codes, dcodes, r.bases);
        if (qual && r.has_qual) st.down(qual, dqual, r.bases);
        st.down(read_index, didx, (r.reads + 1) * 8);
        if (names) st.down(name_off, dnoff, r.reads * 8);
        if (names) st.down(name_len, dnlen, r.reads * 4);
        return st.rc;
    });
}

int kiss_hip_reads_parse_part_dev(kiss_hip_ctx *ctx, const uint8_t *d_raw, uint64_t bytes, int format, int final, uint64_t max_records,
                                  uint8_t *d_codes, uint8_t *d_qual, uint64_t bases_capacity, uint64_t *d_read_index, uint64_t *d_name_off,
                                  uint32_t *d_name_len, uint64_t reads_capacity, kiss_hip_reads_part_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx);
    kiss_hip_reads_part_report rep{};
    rep.parsed = empty_report(format);
    if (report) *report = rep;
    ParseArgs a{d_raw, bytes, format, d_codes, d_qual, bases_capacity, d_read_index, d_name_off, d_name_len, reads_capacity, &rep.parsed};
    KTRY(parse_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    if ((bytes + 2) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    FmEvents ev(ctx, report != nullptr);
    Cut cut;
    float ms_cut = 0.f;
    bool parsed = false;
    int rc = KISS_HIP_OK;
    if (bytes) {
        ev.mark(4);
        rc = cut_steps(ctx, d_raw, bytes, format, final != 0, max_records, cut);
        ev.mark(5);
    }
    if (rc == KISS_HIP_OK) {
        if (bytes) rep.parsed = empty_report(cut.fastq ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_LINES);
        rep.records_complete = cut.complete;
        rep.records = cut.records;
        rep.bytes_used = cut.used;
        a.bytes = cut.used;
        a.format = (int)rep.parsed.format;
        a.no_drop = !cut.whole;
        if (cut.used == 0) { // no line, no read: the one entry of the index
            rc = kiss_zero_u32(ctx, d_read_index, 2);
            if (rc == KISS_HIP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = KISS_HIP_E_HIP;
        } else {
            parsed = true;
            rc = parse_steps(ctx, a, rep.parsed, ev);
        }
        if (bytes) ms_cut = ev.ms(4, 5);
    }
    rc = fm_leave(ctx, ev, rc, parsed ? &rep.parsed.ms_total : nullptr); // (events 0 .. 3 are the parse's)
    rep.parsed.ms_total += ms_cut;
    rep.parsed.ms_lines += ms_cut;
    if (report) *report = rep;
    return rc;
}

int kiss_hip_reads_parse_part_host(const uint8_t *raw, uint64_t bytes, int format, int final, uint64_t max_records, uint8_t *codes,
                                   uint8_t *qual, uint64_t bases_capacity, uint64_t *read_index, uint64_t *name_off, uint32_t *name_len,
                                   uint64_t reads_capacity, kiss_hip_reads_part_report *report, int device)
{
    if (report) {
        *report = kiss_hip_reads_part_report{};
        report->parsed = empty_report(format);
    }
    KTRY(parse_args_check(ParseArgs{raw, bytes, format, codes, qual, bases_capacity, read_index, name_off, name_len, reads_capacity, nullptr}));
    return kiss_one_shot_cached(device, fm_host_max_n(0, bytes + 2), [&](kiss_hip_ctx *ctx) -> int {
        const bool names = name_off != nullptr;
        FmStage st(ctx);
        const uint8_t *draw = st.up(raw, bytes);
        uint8_t *dcodes = st.room<uint8_t>(true, bases_capacity);
        uint8_t *dqual = st.room<uint8_t>(qual != nullptr, bases_capacity);
        uint64_t *didx = st.room<uint64_t>(true, (reads_capacity + 1) * 8);
        uint64_t *dnoff = st.room<uint64_t>(names, reads_capacity * 8);
        uint32_t *dnlen = st.room<uint32_t>(names, reads_capacity * 4);
        if (st.rc) return st.rc;
        kiss_hip_reads_part_report r{};
        const int rc = kiss_hip_reads_parse_part_dev(ctx, draw, bytes, format, final, max_records, dcodes, dqual, bases_capacity, didx, dnoff,
                                                     dnlen, reads_capacity, &r, nullptr);
        if (report) *report = r;
        if (rc) return rc;
        st.down(codes, dcodes, r.parsed.bases);
        if (qual && r.parsed.has_qual) st.down(qual, dqual, r.parsed.bases);
        st.down(read_index, didx, (r.parsed.reads + 1) * 8);
        if (names) st.down(name_off, dnoff, r.parsed.reads * 8);
        if (names) st.down(name_len, dnlen, r.parsed.reads * 4);
        return st.rc;
    });
}

int kiss_hip_reads_interleave_dev(kiss_hip_ctx *ctx, const uint8_t *codes_a, const uint64_t *index_a, const uint8_t *qual_a, uint64_t P_a,
                                  const uint8_t *codes_b, const uint64_t *index_b, const uint8_t *qual_b, uint64_t P_b, uint8_t *codes,
                                  uint64_t *read_index, uint8_t *qual, uint64_t bases_capacity, uint64_t *bases_out, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx);
    if (bases_out) *bases_out = 0;
    const InterleaveArgs a{codes_a, index_a, qual_a, P_a, codes_b, index_b, qual_b, P_b, codes, read_index, qual, bases_capacity, bases_out};
    KTRY(interleave_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, false);
    return fm_leave(ctx, ev, interleave_steps(ctx, a), nullptr);
}

int kiss_hip_reads_interleave_host(const uint8_t *codes_a, const uint64_t *index_a, const uint8_t *qual_a, uint64_t P_a, const uint8_t *codes_b,
                                   const uint64_t *index_b, const uint8_t *qual_b, uint64_t P_b, uint8_t *codes, uint64_t *read_index, uint8_t *qual,
                                   uint64_t bases_capacity, uint64_t *bases_out, int device)
{
    if (bases_out) *bases_out = 0;
    KTRY(interleave_args_check(
        InterleaveArgs{codes_a, index_a, qual_a, P_a, codes_b, index_b, qual_b, P_b, codes, read_index, qual, bases_capacity, bases_out}));
    if (index_a[0] != 0 || index_b[0] != 0 || !fm_index_ascending(index_a, P_a, false) || !fm_index_ascending(index_b, P_b, false))
        return KISS_HIP_E_INVALID;
    return kiss_one_shot_cached(device, fm_host_max_n(0, 0), [&](kiss_hip_ctx *ctx) -> int {
        const uint64_t P = P_a, na = index_a[P], nb = index_b[P];
        FmStage st(ctx);
        const uint8_t *dca = st.up(codes_a, na), *dcb = st.up(codes_b, nb);
        const uint64_t *dia = st.up(index_a, (P + 1) * 8), *dib = st.up(index_b, (P + 1) * 8);
        const uint8_t *dqa = st.up(qual_a, na), *dqb = st.up(qual_b, nb); // (all three of the qualities, or none)
        uint8_t *dc = st.room<uint8_t>(true, bases_capacity);
        uint64_t *di = st.room<uint64_t>(true, (2 * P + 1) * 8);
        uint8_t *dq = st.room<uint8_t>(qual != nullptr, bases_capacity);
        if (st.rc) return st.rc;
        uint64_t total = 0;
        const int rc = kiss_hip_reads_interleave_dev(ctx, dca, dia, dqa, P, dcb, dib, dqb, P, dc, di, dq, bases_capacity, &total, nullptr);
        if (bases_out) *bases_out = total;
        if (rc) return rc;
        st.down(codes, dc, total);
        if (qual) st.down(qual, dq, total);
        st.down(read_index, di, (2 * P + 1) * 8);
        return st.rc;
    });
}

} // extern "C"
