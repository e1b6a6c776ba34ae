// fm_sam.hip -- FM-index: the alignment lines of the SAM output, written on the GPU (kiss_hip_fmi_sam_*).
//
// The reference has no such function; the definition is in include/kiss_hip_sam.h and restated in tests/fm_sam_model.py.  The
// call reads what the parse, align / merge, select, pair and MD calls left on the device.
//
//   head  : one kernel checks read_index, hit_index and ref_name_index and fetches H = hit_index[Q]; a second one, once H is
//           known, checks cigar_index and md_index.
//   count : ONE LANE PER READ holds the read against the definition (BAD reads) and counts its lines.  The library's u64 scan
//           gives read_line; the host looks at bad and at the total once.
//   size  : ONE WAVE PER LINE (a wave takes lines w, w + waves, ...).  The wave finds the read of its line by bisection of
//           read_line, describes the line (SamLine: every field the same in all lanes) and lays it out: the line is 25 PIECES
//           in order, piece p held by lane p -- a short one (a literal, a number, a literal: tabs, numbers, tags) or a long one
//           (QNAME, RNAME, the ops, RNEXT, SEQ, QUAL, MD) of known length -- and one prefix sum over the lanes places them all.
//           A second scan gives line_index; the host looks at the total once (capacity).
//   emit  : the same function again with the writing sink: every lane writes its short piece, then the lanes together write the
//           long ones (lanes over the bytes and the ops).
// Sizing and writing a line are ONE function (sam_line) over a sink, so that the two cannot disagree.  No LDS, no scratch.
//
// What a line IS -- which reads are BAD, the lines of a read, the hit, FLAG, MAPQ, place, TLEN and tags of one line -- stands in
// fm_sam_line.hpp, which fm_bam.hip includes too: one SAM line is one BAM record.
//
// ADDRESSING.  Every address is a kernel-argument base pointer plus a 64-bit offset.  No pointer and no 64-bit offset goes
// through a cross-lane operation as one value: sam_lane64 / sam_up64 (fm_sam_line.hpp) move the two halves.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_sam.h"

#include <vector>

namespace {

#include "fm_sam_line.hpp" // the input, the loads, the cross-lane moves, the BAD rule and the description of a line

// the decimal digits of x (every number of a line is at most 2^32)
__device__ __forceinline__ uint32_t sam_digits(uint64_t x)
{
    return 1u + (x >= 10ull) + (x >= 100ull) + (x >= 1000ull) + (x >= 10000ull) + (x >= 100000ull) + (x >= 1000000ull) + (x >= 10000000ull) +
           (x >= 100000000ull) + (x >= 1000000000ull) + (x >= 10000000000ull);
}

// One lane per read: BAD or not, and its lines.  nl[q] = the lines of read q (nl[Q] = 0 closes the array for the scan).  Only
// the read's own hits, the alignments and records they name once those exist, and its pair are read.
__global__ __launch_bounds__(SAM_THREADS) void k_sam_count(SamIn in, uint64_t *__restrict__ nl, unsigned long long *__restrict__ ctl)
{
    const uint64_t q = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x;
    if (q == 0) nl[in.Q] = 0;
    bool bad = false, unmapped = false;
    if (q < in.Q) {
        uint64_t lines;
        const uint32_t f = sam_read_check(in, q, lines);
        bad = f & SAM_READ_BAD;
        unmapped = f & SAM_READ_UNMAPPED;
        nl[q] = lines;
        if (bad) atomicMax(&ctl[SAM_NFIRST], (unsigned long long)~q);
    }
    const unsigned long long B = __ballot(bad), U = __ballot(unmapped);
    if (lane_id() == 0) {
        if (B) atomicAdd(&ctl[SAM_BAD], (unsigned long long)__popcll(B));
        if (U) atomicAdd(&ctl[SAM_UNMAPPED], (unsigned long long)__popcll(U));
    }
}

// a short piece: a literal of up to 8 bytes (packed, first byte lowest), a number, a literal
struct SamPiece {
    uint64_t pre = 0, suf = 0, num = 0;
    uint32_t plen = 0, slen = 0;
    bool has_num = false, neg = false;
};
template <int N>
__device__ __forceinline__ constexpr uint64_t sam_pack(const char (&s)[N])
{
    static_assert(N - 1 <= 8, "a literal of a piece has at most 8 bytes");
    uint64_t v = 0;
    for (int k = 0; k < N - 1; k++) v |= (uint64_t)(uint8_t)s[k] << (8 * k);
    return v;
}
#define SAM_PRE(pc, s) ((pc).pre = sam_pack(s), (pc).plen = (uint32_t)sizeof(s) - 1u)
#define SAM_SUF(pc, s) ((pc).suf = sam_pack(s), (pc).slen = (uint32_t)sizeof(s) - 1u)
__device__ __forceinline__ void sam_num(SamPiece &pc, uint64_t x, bool neg = false)
{
    pc.has_num = true;
    pc.num = x;
    pc.neg = neg;
}
__device__ __forceinline__ uint32_t sam_piece_bytes(const SamPiece &pc)
{
    return pc.plen + (pc.has_num ? (pc.neg ? 1u : 0u) + sam_digits(pc.num) : 0u) + pc.slen;
}
__device__ __forceinline__ uint8_t sam_base(uint32_t c, bool rev)
{
    if (c > 3u) return 'N';
    if (rev) c = 3u - c;
    return c == 0 ? 'A' : (c == 1 ? 'C' : (c == 2 ? 'G' : 'T'));
}
__device__ __forceinline__ uint8_t sam_op(uint32_t op) { return op == 0 ? 'M' : (op == 1 ? 'I' : (op == 2 ? 'D' : '?')); }

// The ops of an alignment as <len><letter>, lanes over the ops, 64 per step -> their bytes.  WRITE: to out[at ..).
template <bool WRITE>
__device__ __forceinline__ uint64_t sam_ops(const SamIn &in, uint64_t o0, uint64_t nops, uint8_t *out, uint64_t at)
{
    const uint32_t lane = lane_id();
    uint64_t done = 0;
    for (uint64_t kb = 0; kb < nops; kb += 64) {
        const bool have = kb + lane < nops;
        const uint32_t w = have ? sam_ld32(in.cigar + (o0 + kb + lane)) : 0u;
        uint32_t len = w >> 4;
        const uint32_t d = sam_digits(len);
        uint32_t total;
        const uint32_t ex = sam_wave_excl32(have ? d + 1u : 0u, total);
        if (WRITE && have) {
            const uint64_t to = at + done + ex;
            for (uint32_t k = d; k-- > 0;) {
                out[to + k] = (uint8_t)('0' + len % 10u);
                len /= 10u;
            }
            out[to + d] = sam_op(w & 15u);
        }
        done += total;
    }
    return done;
}

// the sink that only sizes
struct SamCount {
    __device__ __forceinline__ void piece(uint64_t, const SamPiece &) const {}
    __device__ __forceinline__ void bytes(uint64_t, const uint8_t *, uint64_t, uint64_t) const {}
    __device__ __forceinline__ void seq(uint64_t, const uint8_t *, uint64_t, uint64_t, bool) const {}
    __device__ __forceinline__ void qual(uint64_t, const uint8_t *, uint64_t, uint64_t, bool) const {}
    __device__ __forceinline__ void ops(uint64_t, const SamIn &, uint64_t, uint64_t) const {}
};
// the sink that writes the line to sam[base ..): every `at` is an offset inside the line
struct SamWrite {
    uint8_t *sam;
    uint64_t base;
    // one lane, its own piece
    __device__ __forceinline__ void piece(uint64_t at, const SamPiece &pc) const
    {
        uint64_t to = base + at;
        for (uint32_t k = 0; k < pc.plen; k++) sam[to + k] = (uint8_t)(pc.pre >> (8 * k));
        to += pc.plen;
        if (pc.has_num) {
            if (pc.neg) sam[to++] = '-';
            const uint32_t d = sam_digits(pc.num);
            uint64_t x = pc.num;
            for (uint32_t k = d; k-- > 0;) {
                if (x <= 0xFFFFFFFFull) { // (a 64-bit division only for the one number that can be 2^32)
                    const uint32_t y = (uint32_t)x;
                    sam[to + k] = (uint8_t)('0' + y % 10u);
                    x = y / 10u;
                } else {
                    sam[to + k] = (uint8_t)('0' + (uint32_t)(x % 10ull));
                    x /= 10ull;
                }
            }
            to += d;
        }
        for (uint32_t k = 0; k < pc.slen; k++) sam[to + k] = (uint8_t)(pc.suf >> (8 * k));
    }
    // the wave, lanes over the bytes: src[from .. from + len) as they stand
    __device__ __forceinline__ void bytes(uint64_t at, const uint8_t *src, uint64_t from, uint64_t len) const
    {
        for (uint64_t k = lane_id(); k < len; k += 64) sam[base + at + k] = src[from + k];
    }
    __device__ __forceinline__ void seq(uint64_t at, const uint8_t *reads, uint64_t rb, uint64_t L, bool rev) const
    {
        for (uint64_t k = lane_id(); k < L; k += 64) sam[base + at + k] = sam_base(reads[rb + (rev ? L - 1 - k : k)], rev);
    }
    __device__ __forceinline__ void qual(uint64_t at, const uint8_t *qual, uint64_t rb, uint64_t L, bool rev) const
    {
        for (uint64_t k = lane_id(); k < L; k += 64) sam[base + at + k] = qual[rb + (rev ? L - 1 - k : k)];
    }
    __device__ __forceinline__ void ops(uint64_t at, const SamIn &in, uint64_t o0, uint64_t nops) const
    {
        (void)sam_ops<true>(in, o0, nops, sam, base + at);
    }
};

// the lanes of the pieces
enum {
    PC_QNAME = 0, PC_FLAG, PC_RNAME_TAB, PC_RNAME, PC_POS, PC_MAPQ, PC_CLIP0, PC_OPS, PC_CLIP1, PC_RNEXT, PC_RNEXT_NAME, PC_PNEXT, PC_TLEN, PC_SEQ,
    PC_QUAL_TAB, PC_QUAL, PC_NM, PC_MD_TAG, PC_MD, PC_AS, PC_XS, PC_YS, PC_YT, PC_YR, PC_END
};

// THE line: laid out, and handed to the sink piece by piece -> its bytes.  (The counting sink and the writing sink go through
// the same layout, so a line is as long as it was sized.)
template <class Sink>
__device__ __forceinline__ uint64_t sam_line(const SamIn &in, const SamLine &d, const Sink &sink)
{
    const uint32_t lane = lane_id();
    const uint64_t name_len = sam_ld32(in.name_len + d.q);
    uint64_t rname0 = 0, rname_len = 0, rnext0 = 0, rnext_len = 0;
    if (d.has_ref) {
        rname0 = sam_ld64(in.ref_name_index + d.ref);
        rname_len = sam_ld64(in.ref_name_index + d.ref + 1) - rname0;
    }
    if (d.rnext == 2) {
        rnext0 = sam_ld64(in.ref_name_index + d.nref);
        rnext_len = sam_ld64(in.ref_name_index + d.nref + 1) - rnext0;
    }
    const uint64_t ops_bytes = d.mapped ? sam_ops<false>(in, d.o0, d.nops, nullptr, 0) : 0;
    SamPiece pc;
    uint64_t big = 0; // the bytes of a long piece
    if (lane == PC_QNAME) big = name_len;
    if (lane == PC_FLAG) (SAM_PRE(pc, "\t"), sam_num(pc, d.flag));
    if (lane == PC_RNAME_TAB) {
        if (d.has_ref) SAM_PRE(pc, "\t");
        else SAM_PRE(pc, "\t*");
    }
    if (lane == PC_RNAME) big = rname_len;
    if (lane == PC_POS) (SAM_PRE(pc, "\t"), sam_num(pc, d.pos));
    if (lane == PC_MAPQ) (SAM_PRE(pc, "\t"), sam_num(pc, d.mapq));
    if (lane == PC_CLIP0) {
        if (!d.mapped) SAM_PRE(pc, "\t*");
        else {
            SAM_PRE(pc, "\t");
            if (d.rbeg) (sam_num(pc, d.rbeg), SAM_SUF(pc, "S"));
        }
    }
    if (lane == PC_OPS) big = ops_bytes;
    if (lane == PC_CLIP1) {
        if (d.mapped && d.L > (uint64_t)d.rend) (sam_num(pc, d.L - d.rend), SAM_SUF(pc, "S\t"));
        else SAM_PRE(pc, "\t");
    }
    if (lane == PC_RNEXT) {
        if (d.rnext == 0) SAM_PRE(pc, "*");
        if (d.rnext == 1) SAM_PRE(pc, "=");
    }
    if (lane == PC_RNEXT_NAME) big = rnext_len;
    if (lane == PC_PNEXT) (SAM_PRE(pc, "\t"), sam_num(pc, d.pnext));
    if (lane == PC_TLEN) (SAM_PRE(pc, "\t"), sam_num(pc, d.tlen, d.tneg), SAM_SUF(pc, "\t"));
    if (lane == PC_SEQ) big = d.L;
    if (lane == PC_QUAL_TAB) {
        if (in.qual) SAM_PRE(pc, "\t");
        else SAM_PRE(pc, "\t*");
    }
    if (lane == PC_QUAL) big = in.qual ? d.L : 0;
    if (d.mapped) {
        if (lane == PC_NM) (SAM_PRE(pc, "\tNM:i:"), sam_num(pc, d.nm));
        if (lane == PC_MD_TAG && d.has_md) SAM_PRE(pc, "\tMD:Z:");
        if (lane == PC_MD) big = d.mdl;
        if (lane == PC_AS) (SAM_PRE(pc, "\tAS:i:"), sam_num(pc, d.as));
        if (lane == PC_XS && d.has_xs) (SAM_PRE(pc, "\tXS:i:"), sam_num(pc, d.xs));
        if (lane == PC_YS && d.has_ys) (SAM_PRE(pc, "\tYS:i:"), sam_num(pc, d.ys));
        if (lane == PC_YT && d.yt) SAM_PRE(pc, "\tYT:Z:CP");
        if (lane == PC_YR && d.yr) SAM_PRE(pc, "\tYR:i:1");
    }
    if (lane == PC_END) SAM_PRE(pc, "\n");
    const uint32_t small = sam_piece_bytes(pc);
    uint64_t total;
    const uint64_t at = sam_wave_excl64((uint64_t)small + big, total);
    if (small) sink.piece(at, pc);
    sink.bytes(sam_lane64(at, PC_QNAME), in.names, sam_ld64(in.name_off + d.q), name_len);
    sink.bytes(sam_lane64(at, PC_RNAME), in.ref_names, rname0, rname_len);
    if (d.mapped) sink.ops(sam_lane64(at, PC_OPS), in, d.o0, d.nops);
    sink.bytes(sam_lane64(at, PC_RNEXT_NAME), in.ref_names, rnext0, rnext_len);
    sink.seq(sam_lane64(at, PC_SEQ), in.reads, d.rb, d.L, d.rev);
    if (in.qual) sink.qual(sam_lane64(at, PC_QUAL), in.qual, d.rb, d.L, d.rev);
    if (d.has_md) sink.bytes(sam_lane64(at, PC_MD), in.md, d.md0, d.mdl);
    return total;
}

// size[line] = the bytes of the line (size[lines] = 0 closes the array for the scan); the longest one
__global__ __launch_bounds__(SAM_THREADS) void k_sam_size(SamIn in, const uint64_t *__restrict__ read_line, uint64_t *__restrict__ size,
                                                        unsigned long long *__restrict__ ctl)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) size[in.lines] = 0;
    const uint64_t waves = (uint64_t)gridDim.x * SAM_WAVES;
    unsigned long long longest = 0;
    for (uint64_t line = (uint64_t)blockIdx.x * SAM_WAVES + (threadIdx.x >> 6); line < in.lines; line += waves) {
        SamLine d;
        sam_describe(in, read_line, line, d);
        const uint64_t bytes = sam_line(in, d, SamCount{});
        if (lane_id() == 0) size[line] = bytes;
        longest = longest > bytes ? longest : bytes;
    }
    if (lane_id() == 0 && longest) atomicMax(&ctl[SAM_LONGEST], longest);
}

// offs: the scanned sizes, offs[lines] <= the capacity of sam (the host has looked); read_line_out and line_index too
__global__ __launch_bounds__(SAM_THREADS) void k_sam_emit(SamIn in, const uint64_t *__restrict__ read_line, const uint64_t *__restrict__ offs,
                                                        uint8_t *sam, uint64_t *__restrict__ line_index, uint64_t *__restrict__ read_line_out)
{
    const uint64_t step = (uint64_t)gridDim.x * SAM_THREADS;
    for (uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x; g <= in.Q; g += step) read_line_out[g] = sam_ld64(read_line + g);
    if (line_index)
        for (uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x; g <= in.lines; g += step) line_index[g] = sam_ld64(offs + g);
    const uint64_t waves = (uint64_t)gridDim.x * SAM_WAVES;
    for (uint64_t line = (uint64_t)blockIdx.x * SAM_WAVES + (threadIdx.x >> 6); line < in.lines; line += waves) {
        SamLine d;
        sam_describe(in, read_line, line, d);
        (void)sam_line(in, d, SamWrite{sam, sam_ld64(offs + line)});
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SamArgs {
    const kiss_hip_sam_input *in;
    uint8_t *sam;
    uint64_t sam_capacity;
    uint64_t *line_index;
    uint64_t line_capacity;
    uint64_t *read_line;
};

int sam_args_check(const SamArgs &a)
{
    const kiss_hip_sam_input *in = a.in;
    if (!in || !a.read_line) return KISS_HIP_E_INVALID;
    if (!in->reads || !in->read_index || !in->names || !in->name_off || !in->name_len || !in->alns || !in->cigar || !in->cigar_index || !in->hits ||
        !in->hit_index)
        return KISS_HIP_E_INVALID;
    if (in->md && !in->md_index) return KISS_HIP_E_INVALID;
    if (in->R && (!in->ref_names || !in->ref_name_index || !in->bounds)) return KISS_HIP_E_INVALID;
    if (a.sam_capacity && !a.sam) return KISS_HIP_E_INVALID;
    if (in->pairs && (in->Q & 1ull)) return KISS_HIP_E_INVALID;
    if (in->Q >= (1ull << 31) || in->C > 0xFFFFFFFFull || in->R > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int sam_zero_reads(kiss_hip_ctx *ctx, const SamArgs &a)
{
    KTRY(kiss_zero_u32(ctx, a.read_line, 2));
    if (a.line_index) KTRY(kiss_zero_u32(ctx, a.line_index, 2));
    KCHECK(hipStreamSynchronize(ctx->stream));
    return KISS_HIP_OK;
}

int sam_steps(kiss_hip_ctx *ctx, const SamArgs &a, kiss_hip_sam_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const kiss_hip_sam_input &u = *a.in;
    const uint64_t Q = u.Q;
    if (Q == 0) return sam_zero_reads(ctx, a);
    FmCtl<SAM_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_SAM_CTL));
    unsigned long long *const d_ctl = ctl.d, *const h = ctl.h;
    const dim3 threads(SAM_THREADS);
    ev.mark(0);
    KTRY(ctl.zero());
    hipLaunchKernelGGL(k_sam_head, dim3(fm_grid((Q > u.R ? Q : u.R) + 1, SAM_THREADS)), threads, 0, ctx->stream, u.read_index, u.hit_index, Q,
                       u.ref_name_index, u.R, d_ctl);
    KCHECK(hipGetLastError());
    KTRY(ctl.fetch_sync());
    if (h[SAM_BADIN]) return KISS_HIP_E_INVALID; // an index out of order, a read of length 0
    const uint64_t H = h[SAM_H];
    if (H > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if ((Q + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED; // more than the ctx can scan
    DevBuf per_read;
    KTRY(per_read.take(ctx, FM_SLOT_SAM_READS, (Q + 1) * 8));
    uint64_t *const rl = (uint64_t *)per_read.p; // (scanned in place)
    SamIn in{u.reads, u.read_index, u.qual, u.names, u.name_off, u.name_len, (const uint32_t *)u.alns, u.cigar, u.cigar_index,
             (const uint32_t *)u.hits, u.hit_index, (const uint32_t *)u.pairs, u.source, u.md, u.md_index, u.ref_names, u.ref_name_index, u.bounds,
             Q, u.C, u.R, u.first_alns, H, 0};
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, Q);
        const uint64_t most = u.C > H ? u.C : H;
        if (most)
            hipLaunchKernelGGL(k_sam_check, dim3(fm_grid(most, SAM_THREADS)), threads, 0, ctx->stream, u.cigar_index, u.C, u.md ? u.md_index : nullptr, H,
                               d_ctl);
        hipLaunchKernelGGL(k_sam_count, dim3(fm_grid(Q, SAM_THREADS)), threads, 0, ctx->stream, in, rl, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, rl, rl, Q + 1));
    uint64_t lines = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&lines, rl + Q, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (h[SAM_BADIN]) return KISS_HIP_E_INVALID; // a cigar or md index decreases
    if (h[SAM_BAD]) {
        rep.bad = h[SAM_BAD];
        rep.first_bad = ~h[SAM_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    rep.lines = lines;
    rep.unmapped_lines = h[SAM_UNMAPPED];
    if (lines > 0xFFFFFFFFull || (lines + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    DevBuf per_line;
    KTRY(per_line.take(ctx, FM_SLOT_SAM_LINES, (lines + 1) * 8));
    uint64_t *const size = (uint64_t *)per_line.p; // (scanned in place)
    in.lines = lines;
    const uint64_t blocks = div_up(lines, SAM_WAVES);
    const dim3 grid((unsigned)(blocks < SAM_MAX_BLOCKS ? blocks : SAM_MAX_BLOCKS));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, lines);
        hipLaunchKernelGGL(k_sam_size, grid, threads, 0, ctx->stream, in, (const uint64_t *)rl, size, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, size, size, lines + 1));
    uint64_t total = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total, size + lines, 8, hipMemcpyDeviceToHost, ctx->stream));
    ev.mark(1);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_count = ev.ms(0, 1);
    rep.sam_bytes = total;
    rep.longest = h[SAM_LONGEST];
    // (the totals are in the report: the caller's second call)
    if (a.sam_capacity < total || (a.line_index && a.line_capacity < lines)) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, lines);
        hipLaunchKernelGGL(k_sam_emit, grid, threads, 0, ctx->stream, in, (const uint64_t *)rl, (const uint64_t *)size, a.sam, a.line_index,
                           a.read_line);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_emit = ev.ms(1, 2);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_sam_dev(kiss_hip_ctx *ctx, const kiss_hip_sam_input *in, uint8_t *sam, uint64_t sam_capacity, uint64_t *line_index,
                         uint64_t line_capacity, uint64_t *read_line, kiss_hip_sam_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_sam_report rep{};
    if (report) *report = rep;
    const SamArgs a{in, sam, sam_capacity, line_index, line_capacity, read_line};
    KTRY(sam_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    int rc = sam_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_fmi_sam_host(const kiss_hip_sam_input *in, uint8_t *sam, uint64_t sam_capacity, uint64_t *line_index, uint64_t line_capacity,
                          uint64_t *read_line, kiss_hip_sam_report *report, int device)
{
    if (report) *report = kiss_hip_sam_report{};
    const SamArgs a{in, sam, sam_capacity, line_index, line_capacity, read_line};
    KTRY(sam_args_check(a));
    const kiss_hip_sam_input &u = *in;
    const uint64_t Q = u.Q, C = u.C, R = u.R;
    if (Q == 0) {
        read_line[0] = 0;
        if (line_index) line_index[0] = 0;
        return KISS_HIP_OK;
    }
    if (!fm_index_ascending(u.read_index, Q, true) || !fm_index_ascending(u.hit_index, Q, false) || !fm_index_ascending(u.cigar_index, C, false) ||
        (R && !fm_index_ascending(u.ref_name_index, R, false)))
        return KISS_HIP_E_INVALID;
    const uint64_t H = u.hit_index[Q];
    if (H > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (u.md && !fm_index_ascending(u.md_index, H, false)) return KISS_HIP_E_INVALID;
    uint64_t name_bytes = 0;
    for (uint64_t q = 0; q < Q; q++)
        if (name_bytes < u.name_off[q] + u.name_len[q]) name_bytes = u.name_off[q] + u.name_len[q];
    const uint64_t bases = u.read_index[Q];
    // (a line per hit at the most, and one per read: the scans of the call fit a ctx of this size)
    return kiss_one_shot_cached(device, fm_host_max_n(0, Q + H + 1), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx), st2(ctx);
        kiss_hip_sam_input d = u;
        d.reads = st.up(u.reads, bases);
        d.read_index = st.up(u.read_index, (Q + 1) * 8);
        d.qual = st.up(u.qual, bases);
        d.names = st.up(u.names, name_bytes);
        d.name_off = st.up(u.name_off, Q * 8);
        d.name_len = st.up(u.name_len, Q * 4);
        d.alns = st.up(u.alns, C * sizeof(kiss_hip_aln));
        d.cigar = st.up(u.cigar, u.cigar_index[C] * 4);
        d.cigar_index = st.up(u.cigar_index, (C + 1) * 8);
        d.hits = st.up(u.hits, H * sizeof(kiss_hip_hit));
        d.hit_index = st.up(u.hit_index, (Q + 1) * 8);
        d.pairs = st.up(u.pairs, Q / 2 * sizeof(kiss_hip_pair));
        d.source = st.up(u.source, C * 4);
        d.md = st.up(u.md, u.md ? u.md_index[H] : 0);
        d.md_index = st.up(u.md ? u.md_index : nullptr, (H + 1) * 8);
        if (st.rc) return st.rc;
        d.ref_names = R ? st2.up(u.ref_names, u.ref_name_index[R]) : nullptr;
        d.ref_name_index = R ? st2.up(u.ref_name_index, (R + 1) * 8) : nullptr;
        d.bounds = R ? st2.up(u.bounds, (R + 1) * 8) : nullptr;
        uint64_t *drl = st2.room<uint64_t>(true, (Q + 1) * 8);
        if (st2.rc) return st2.rc;
        // the sizing call first: the room on the device is the total, whatever capacity the caller names
        kiss_hip_sam_report r{};
        int rc = kiss_hip_fmi_sam_dev(ctx, &d, nullptr, 0, nullptr, 0, drl, &r, nullptr);
        uint8_t *dsam = nullptr;
        uint64_t *dli = nullptr;
        if (rc == KISS_HIP_E_INVALID && r.sam_bytes && r.sam_bytes <= sam_capacity && (!line_index || r.lines <= line_capacity)) {
            dsam = st2.room<uint8_t>(true, r.sam_bytes);
            dli = st2.room<uint64_t>(line_index != nullptr, (r.lines + 1) * 8);
            if (st2.rc) return st2.rc;
            rc = kiss_hip_fmi_sam_dev(ctx, &d, dsam, r.sam_bytes, dli, r.lines, drl, &r, nullptr);
        }
        if (report) *report = r;
        if (rc) return rc;
        st2.down(sam, dsam, r.sam_bytes);
        if (line_index) st2.down(line_index, dli, (r.lines + 1) * 8);
        st2.down(read_line, drl, (Q + 1) * 8);
        return st2.rc;
    });
}

} // extern "C"
