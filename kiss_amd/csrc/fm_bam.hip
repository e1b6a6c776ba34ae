// fm_bam.hip -- the BAM output written on the GPU: the alignment records of a batch (kiss_hip_fmi_bam_*) and the BGZF framing
// with the CRC-32 of every block (kiss_hip_bgzf_*).  The definition is in include/kiss_hip_bam.h and restated in
// tests/bam_model.py.
//
// THE RECORDS have the shape of fm_sam.hip, and what a line is -- which hit, FLAG, MAPQ, place, TLEN, tags -- comes from the same
// code (fm_sam_line.hpp: sam_read_check, sam_describe):
//   head  : k_sam_head / k_sam_check on the index arrays.
//   count : ONE LANE PER READ: BAD for SAM, or for BAM by its name, its length or a position; its records.  u64 scan: read_rec.
//   size  : ONE WAVE PER RECORD: the ops are walked once by the lanes (reflen for the bin, the op codes, the op count), then the
//           record is laid out as 25 PIECES in order, piece p held by lane p -- a short one (a word of the fixed part, a tag: up to
//           8 bytes in a register) or a long one (name, ops, SEQ, QUAL, MD) of known length -- and one prefix sum over the lanes
//           places them all.  A record that BAM cannot hold marks its read (a flag per read, so a read counts once).  u64 scan:
//           rec_index.
//   emit  : the same function with the writing sink.
// THE FRAMING: ONE WORKGROUP PER BLOCK (k_bgzf).  The payload is read once, as aligned words with bytes at both ends, into LDS at
// the byte phase of its address; from there it is copied out (aligned words of the destination, two LDS words funnelled into one)
// and checksummed: lane t takes the bytes [t * piece, (t + 1) * piece), piece = ceil(len / 256), and runs the byte-wise table CRC
// over them (the 256-entry table in LDS), starting from 0 -- lane 0 from 0xFFFFFFFF.  The register of lane t is then multiplied by
// x^(8 * bytes behind its piece) modulo the polynomial (crc_mul: 32 shift-and-add steps in registers; the powers x^(8 * 2^j) are
// compile-time constants), the products are XORed across the workgroup, and the complement is the CRC-32.
//
// ADDRESSING.  As fm_sam.hip: every address is a kernel-argument base pointer plus a 64-bit offset, no pointer crosses lanes,
// 64-bit values cross lanes as two unsigned halves (sam_lane64 / sam_up64).  No scratch.
#include "fm_internal.hpp"
#include "../../include/kiss_hip_bam.h"

namespace {

#include "fm_sam_line.hpp"

// (the scratch of a BAM call lives in the slots of the SAM call: a ctx runs one call at a time)
constexpr FmSlot BAM_SLOT_CTL = FM_SLOT_SAM_CTL, BAM_SLOT_READS = FM_SLOT_SAM_READS, BAM_SLOT_RECS = FM_SLOT_SAM_LINES;

// One lane per read.  nr[q] = the records of read q (nr[Q] = 0 closes the array for the scan).
__global__ __launch_bounds__(SAM_THREADS) void k_bam_count(SamIn in, uint64_t *__restrict__ nr, unsigned long long *__restrict__ ctl)
{
    const uint64_t q = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x;
    if (q == 0) nr[in.Q] = 0;
    bool bad = false, unmapped = false;
    if (q < in.Q) {
        uint64_t recs;
        const uint32_t f = sam_read_check(in, q, recs);
        bad = f & SAM_READ_BAD;
        unmapped = f & SAM_READ_UNMAPPED;
        const uint32_t nl = sam_ld32(in.name_len + q);
        if (nl == 0 || nl > 254u) bad = true;
        if (sam_ld64(in.read_index + q + 1) - sam_ld64(in.read_index + q) >= (1ull << 28)) bad = true;
        // POS - 1 of the read's own hits, and of the hit its pair chooses for the partner (PNEXT - 1), where they exist
        const uint64_t hb = sam_ld64(in.hit_index + q), he = sam_ld64(in.hit_index + q + 1);
        uint64_t other = SAM_NONE;
        if (in.pairs) other = sam_pair(in, q >> 1, (q & 1) ? P_HIT1 : P_HIT2);
        for (uint64_t h = hb; h <= he; h++) {
            uint64_t x = h;
            if (h == he) { // (the partner's last)
                if (other == SAM_NONE || other >= in.H) break;
                x = other;
            }
            const uint64_t a = sam_hit(in, x, H_ALN), ref = sam_hit(in, x, H_REF);
            if (a >= in.C || ref >= in.R) continue;
            const uint64_t tbeg = sam_aln(in, a, A_TBEG), b0 = sam_ld64(in.bounds + ref);
            if (tbeg >= b0 && tbeg - b0 >= (1ull << 31)) bad = true;
        }
        nr[q] = recs;
        if (bad) atomicMax(&ctl[SAM_NFIRST], (unsigned long long)~q);
    }
    const unsigned long long B = __ballot(bad), U = __ballot(unmapped);
    if (lane_id() == 0) {
        if (B) atomicAdd(&ctl[SAM_BAD], (unsigned long long)__popcll(B));
        if (U) atomicAdd(&ctl[SAM_UNMAPPED], (unsigned long long)__popcll(U));
    }
}

// ---- one record ------------------------------------------------------------------------------------------------------------
// The ops of an alignment walked by the lanes, 64 per step -> reflen (the M and D lengths), in every lane; bad_code: a code above 2
__device__ __forceinline__ uint64_t bam_walk_ops(const SamIn &in, uint64_t o0, uint64_t nops, bool &bad_code)
{
    uint64_t mine = 0;
    bool bad = false;
    for (uint64_t k = lane_id(); k < nops; k += 64) {
        const uint32_t w = sam_ld32(in.cigar + (o0 + k));
        const uint32_t op = w & 15u;
        if (op > 2u) bad = true;
        if (op == 0u || op == 2u) mine += (uint64_t)(w >> 4);
    }
    bad_code = __ballot(bad) != 0ull;
    uint64_t total;
    (void)sam_wave_excl64(mine, total);
    return total;
}

// reg2bin of the SAM specification on signed 64-bit values, [beg, end)
__device__ __forceinline__ uint32_t bam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}

// the nibble of base i of SEQ
__device__ __forceinline__ uint32_t bam_nibble(const uint8_t *reads, uint64_t rb, uint64_t L, uint64_t i, bool rev)
{
    const uint32_t c = reads[rb + (rev ? L - 1 - i : i)];
    if (c > 3u) return 15u;
    return 1u << (rev ? 3u - c : c);
}

// the sink that only sizes
struct BamCount {
    __device__ __forceinline__ void piece(uint64_t, uint64_t, uint32_t) const {}
    __device__ __forceinline__ void bytes(uint64_t, const uint8_t *, uint64_t, uint64_t) const {}
    __device__ __forceinline__ void ops(uint64_t, const SamIn &, uint64_t, uint64_t) const {}
    __device__ __forceinline__ void seq(uint64_t, const uint8_t *, uint64_t, uint64_t, bool) const {}
    __device__ __forceinline__ void qual(uint64_t, const uint8_t *, uint64_t, uint64_t, bool) const {}
};
// the sink that writes the record to bam[base ..): every `at` is an offset inside the record
struct BamWrite {
    uint8_t *bam;
    uint64_t base;
    // one lane, its own piece: the low len bytes of val, lowest first
    __device__ __forceinline__ void piece(uint64_t at, uint64_t val, uint32_t len) const
    {
        for (uint32_t k = 0; k < len; k++) bam[base + at + k] = (uint8_t)(val >> (8 * k));
    }
    // the wave, lanes over the bytes: src[from .. from + len) as they stand
    __device__ __forceinline__ void bytes(uint64_t at, const uint8_t *src, uint64_t from, uint64_t len) const
    {
        for (uint64_t k = lane_id(); k < len; k += 64) bam[base + at + k] = src[from + k];
    }
    __device__ __forceinline__ void ops(uint64_t at, const SamIn &in, uint64_t o0, uint64_t nops) const
    {
        for (uint64_t k = lane_id(); k < nops; k += 64) {
            const uint32_t w = sam_ld32(in.cigar + (o0 + k));
            const uint64_t to = base + at + 4 * k;
            bam[to] = (uint8_t)w;
            bam[to + 1] = (uint8_t)(w >> 8);
            bam[to + 2] = (uint8_t)(w >> 16);
            bam[to + 3] = (uint8_t)(w >> 24);
        }
    }
    __device__ __forceinline__ void seq(uint64_t at, const uint8_t *reads, uint64_t rb, uint64_t L, bool rev) const
    {
        const uint64_t nb = (L + 1) >> 1;
        for (uint64_t j = lane_id(); j < nb; j += 64) {
            const uint32_t hi = bam_nibble(reads, rb, L, 2 * j, rev);
            const uint32_t lo = 2 * j + 1 < L ? bam_nibble(reads, rb, L, 2 * j + 1, rev) : 0u;
            bam[base + at + j] = (uint8_t)(hi << 4 | lo);
        }
    }
    __device__ __forceinline__ void qual(uint64_t at, const uint8_t *qual, uint64_t rb, uint64_t L, bool rev) const
    {
        for (uint64_t k = lane_id(); k < L; k += 64)
            bam[base + at + k] = qual ? (uint8_t)(qual[rb + (rev ? L - 1 - k : k)] - 33u) : (uint8_t)0xFF;
    }
};

// the lanes of the pieces
enum {
    BP_SIZE = 0, BP_REF, BP_POS, BP_NAME_MAPQ_BIN, BP_NCIG_FLAG, BP_LSEQ, BP_NREF, BP_NPOS, BP_TLEN, BP_NAME, BP_NAME_NUL, BP_CLIP0, BP_OPS,
    BP_CLIP1, BP_SEQ, BP_QUAL, BP_NM, BP_MD_TAG, BP_MD, BP_MD_NUL, BP_AS, BP_XS, BP_YS, BP_YT, BP_YR
};
// a tag of type I: the two letters, 'I', the value
__device__ __forceinline__ uint64_t bam_tag_u32(char c0, char c1, uint32_t v)
{
    return (uint64_t)(uint8_t)c0 | (uint64_t)(uint8_t)c1 << 8 | (uint64_t)'I' << 16 | (uint64_t)v << 24;
}

// THE record: laid out, and handed to the sink piece by piece -> its bytes, block_size included.  reflen: of bam_walk_ops.
template <class Sink>
__device__ __forceinline__ uint64_t bam_record(const SamIn &in, const SamLine &d, uint64_t reflen, const Sink &sink)
{
    const uint32_t lane = lane_id();
    const uint64_t name_len = sam_ld32(in.name_len + d.q);
    const uint32_t clip0 = d.mapped ? d.rbeg : 0u;
    const uint64_t clip1 = d.mapped ? d.L - (uint64_t)d.rend : 0ull;
    const uint64_t ncig = d.mapped ? d.nops + (clip0 ? 1u : 0u) + (clip1 ? 1u : 0u) : 0ull;
    const int64_t pos0 = (int64_t)d.pos - 1; // (-1 without a place)
    const uint32_t bin = bam_reg2bin(pos0, pos0 + (int64_t)(d.mapped && reflen ? reflen : 1ull)) & 0xFFFFu;
    const uint32_t tl = d.tneg ? 0u - (uint32_t)d.tlen : (uint32_t)d.tlen;
    uint64_t val = 0, big = 0;
    uint32_t small = 0;
    if (lane <= BP_TLEN) small = 4;
    if (lane == BP_REF) val = d.has_ref ? (uint32_t)d.ref : 0xFFFFFFFFu;
    if (lane == BP_POS) val = (uint32_t)pos0;
    if (lane == BP_NAME_MAPQ_BIN) val = (((uint32_t)name_len + 1u) & 0xFFu) | (d.mapq & 0xFFu) << 8 | bin << 16;
    if (lane == BP_NCIG_FLAG) val = ((uint32_t)ncig & 0xFFFFu) | (d.flag & 0xFFFFu) << 16;
    if (lane == BP_LSEQ) val = (uint32_t)d.L;
    if (lane == BP_NREF) val = d.rnext ? (uint32_t)d.nref : 0xFFFFFFFFu;
    if (lane == BP_NPOS) val = (uint32_t)(d.pnext - 1ull);
    if (lane == BP_TLEN) val = tl;
    if (lane == BP_NAME) big = name_len;
    if (lane == BP_NAME_NUL) small = 1;
    if (lane == BP_CLIP0 && clip0) (val = (uint64_t)clip0 << 4 | 4u, small = 4);
    if (lane == BP_OPS && d.mapped) big = 4 * d.nops;
    if (lane == BP_CLIP1 && clip1) (val = (uint64_t)(uint32_t)(clip1 << 4 | 4u), small = 4);
    if (lane == BP_SEQ) big = (d.L + 1) >> 1;
    if (lane == BP_QUAL) big = d.L;
    if (d.mapped) {
        if (lane == BP_NM) (val = bam_tag_u32('N', 'M', d.nm), small = 7);
        if (d.has_md) {
            if (lane == BP_MD_TAG) (val = (uint64_t)'M' | (uint64_t)'D' << 8 | (uint64_t)'Z' << 16, small = 3);
            if (lane == BP_MD) big = d.mdl;
            if (lane == BP_MD_NUL) small = 1;
        }
        if (lane == BP_AS) (val = bam_tag_u32('A', 'S', d.as), small = 7);
        if (lane == BP_XS && d.has_xs) (val = bam_tag_u32('X', 'S', d.xs), small = 7);
        if (lane == BP_YS && d.has_ys) (val = bam_tag_u32('Y', 'S', d.ys), small = 7);
        if (lane == BP_YT && d.yt) (val = (uint64_t)'Y' | (uint64_t)'T' << 8 | (uint64_t)'Z' << 16 | (uint64_t)'C' << 24 | (uint64_t)'P' << 32, small = 6);
        if (lane == BP_YR && d.yr) (val = (uint64_t)'Y' | (uint64_t)'R' << 8 | (uint64_t)'C' << 16 | 1ull << 24, small = 4);
    }
    uint64_t total;
    const uint64_t at = sam_wave_excl64((uint64_t)small + big, total);
    if (lane == BP_SIZE) val = (uint32_t)(total - 4ull);
    if (small) sink.piece(at, val, small);
    sink.bytes(sam_lane64(at, BP_NAME), in.names, sam_ld64(in.name_off + d.q), name_len);
    if (d.mapped) sink.ops(sam_lane64(at, BP_OPS), in, d.o0, d.nops);
    sink.seq(sam_lane64(at, BP_SEQ), in.reads, d.rb, d.L, d.rev);
    sink.qual(sam_lane64(at, BP_QUAL), in.qual, d.rb, d.L, d.rev);
    if (d.mapped && d.has_md) sink.bytes(sam_lane64(at, BP_MD), in.md, d.md0, d.mdl);
    return total;
}

// The record number of a wave is the same in all its lanes, so the compiler would keep it, and the forty values that describe the
// record, in scalar registers beside the forty-eight of the input: more than a wave has, and it spills them.  Handing the number
// through a vector register (no instruction) puts the description into vector registers, of which there are plenty.
__device__ __forceinline__ uint64_t bam_in_vgprs(uint64_t v)
{
    uint32_t lo = (uint32_t)(v & 0xFFFFFFFFull), hi = (uint32_t)(v >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return sam_join(hi, lo);
}

// size[rec] = the bytes of the record (size[recs] = 0 closes the array for the scan); the longest one; the reads with a record
// that BAM cannot hold (flag: one u32 per read, zeroed).  One wave, one record, and no loop over records: what a loop would keep
// alive across its turns (the input's pointers, the masks) is what did not fit the scalar registers.
__global__ __launch_bounds__(SAM_THREADS) void k_bam_size(SamIn in, const uint64_t *__restrict__ read_rec, uint64_t *__restrict__ size,
                                                        uint32_t *__restrict__ flag, unsigned long long *__restrict__ ctl)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) size[in.lines] = 0;
    const uint64_t r = (uint64_t)blockIdx.x * SAM_WAVES + (threadIdx.x >> 6);
    if (r >= in.lines) return;
    const uint64_t rec = bam_in_vgprs(r);
    SamLine d;
    sam_describe(in, read_rec, rec, d);
    bool bad = false;
    uint64_t reflen = 0;
    if (d.mapped) {
        reflen = bam_walk_ops(in, d.o0, d.nops, bad);
        if (d.nops + (d.rbeg ? 1u : 0u) + (d.L > (uint64_t)d.rend ? 1u : 0u) > 65535ull) bad = true;
    }
    const uint64_t bytes = bam_record(in, d, reflen, BamCount{});
    if (bytes - 4ull >= (1ull << 31)) bad = true;
    if (lane_id() == 0) {
        size[rec] = bytes;
        if (bad) {
            if (atomicExch(flag + d.q, 1u) == 0u) atomicAdd(&ctl[SAM_BAD], 1ull);
            atomicMax(&ctl[SAM_NFIRST], (unsigned long long)~d.q);
        }
        // (the word only grows: a record no longer than what it holds now cannot change it)
        if (bytes > sam_ld64((const uint64_t *)ctl + SAM_LONGEST)) atomicMax(&ctl[SAM_LONGEST], (unsigned long long)bytes);
    }
}

// offs: the scanned sizes, offs[recs] <= the capacity of bam (the host has looked); read_rec_out and rec_index too
__global__ __launch_bounds__(SAM_THREADS) void k_bam_emit(SamIn in, const uint64_t *__restrict__ read_rec, const uint64_t *__restrict__ offs,
                                                        uint8_t *bam, uint64_t *__restrict__ rec_index, uint64_t *__restrict__ read_rec_out)
{
    const uint64_t step = (uint64_t)gridDim.x * SAM_THREADS;
    for (uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x; g <= in.Q; g += step) read_rec_out[g] = sam_ld64(read_rec + g);
    if (rec_index)
        for (uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x; g <= in.lines; g += step) rec_index[g] = sam_ld64(offs + g);
    const uint64_t r = (uint64_t)blockIdx.x * SAM_WAVES + (threadIdx.x >> 6);
    if (r >= in.lines) return;
    const uint64_t rec = bam_in_vgprs(r);
    SamLine d;
    sam_describe(in, read_rec, rec, d);
    bool bad_code;
    const uint64_t reflen = d.mapped ? bam_walk_ops(in, d.o0, d.nops, bad_code) : 0ull;
    (void)bam_record(in, d, reflen, BamWrite{bam, sam_ld64(offs + rec)});
}

// ---- BGZF ------------------------------------------------------------------------------------------------------------------
#include "bgzf_block.hpp"
constexpr unsigned BGZF_MAX_BLOCKS = 2048;

// One workgroup per block (a workgroup takes blocks b, b + gridDim.x, ...); the end-of-file block by workgroup 0.
__global__ __launch_bounds__(BGZF_THREADS) void k_bgzf(const uint8_t *__restrict__ data, uint64_t n, uint32_t bb, uint64_t blocks, int eof,
                                                      uint8_t *__restrict__ out)
{
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_pay[BGZF_PAY_WORDS];
    __shared__ uint32_t s_acc;
    const uint32_t t = threadIdx.x;
    s_tab[t] = crc_table_entry(t);
    if (eof && blockIdx.x == 0 && t < KISS_HIP_BGZF_EOF_BYTES) out[n + (uint64_t)KISS_HIP_BGZF_OVERHEAD * blocks + t] = bgzf_eof_byte(t);
    const uint8_t *const pb = (const uint8_t *)s_pay;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t src = b * (uint64_t)bb;
        const uint32_t len = (uint32_t)(n - src < (uint64_t)bb ? n - src : (uint64_t)bb);
        const uint64_t ob = b * ((uint64_t)bb + KISS_HIP_BGZF_OVERHEAD), dst = ob + 23u;
        if (t == 0) s_acc = 0;
        if (t < 23u) out[ob + t] = bgzf_head_byte(t, len);
        // the payload into LDS at the byte phase of its address: payload byte i is LDS byte sh + i
        const uint32_t sh = (uint32_t)(((uint64_t)(uintptr_t)data + src) & 3ull);
        {
            uint32_t head = (4u - sh) & 3u;
            head = head < len ? head : len;
            const uint32_t words = (len - head) >> 2;
            if (t < head) ((uint8_t *)s_pay)[sh + t] = data[src + t];
            const uint32_t *const gw = (const uint32_t *)(data + (src + head)); // (a multiple of 4)
            const uint32_t w0 = (sh + head) >> 2;
            for (uint32_t w = t; w < words; w += BGZF_THREADS) s_pay[w0 + w] = gw[w];
            const uint32_t done = head + 4u * words;
            if (t < len - done) ((uint8_t *)s_pay)[sh + done + t] = data[src + done + t];
        }
        __syncthreads();
        // out of LDS: aligned words of the destination, bytes at both ends
        {
            uint32_t head = (4u - (uint32_t)(((uint64_t)(uintptr_t)out + dst) & 3ull)) & 3u;
            head = head < len ? head : len;
            const uint32_t words = (len - head) >> 2;
            if (t < head) out[dst + t] = pb[sh + t];
            uint32_t *const ow = (uint32_t *)(out + (dst + head)); // (a multiple of 4)
            const uint32_t from = sh + head, r = 8u * (from & 3u);
            for (uint32_t w = t; w < words; w += BGZF_THREADS) {
                const uint32_t i = (from >> 2) + w;
                const uint32_t lo = s_pay[i];
                ow[w] = r ? (lo >> r) | (s_pay[i + 1] << (32u - r)) : lo;
            }
            const uint32_t done = head + 4u * words;
            if (t < len - done) out[dst + done + t] = pb[sh + done + t];
        }
        // the CRC: lane t over its piece, then times x^(8 * the bytes behind the piece)
        {
            const uint32_t c = crc_wave_of_pieces(s_tab, pb + sh, len, t);
            if ((t & 63u) == 0) atomicXor(&s_acc, c);
        }
        __syncthreads();
        if (t < 8u) {
            const uint32_t v = t < 4u ? ~s_acc : len;
            out[dst + len + t] = (uint8_t)(v >> (8u * (t & 3u)));
        }
        __syncthreads(); // (s_acc and the payload are the next block's)
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct BamArgs {
    const kiss_hip_sam_input *in;
    uint8_t *bam;
    uint64_t bam_capacity;
    uint64_t *rec_index;
    uint64_t rec_capacity;
    uint64_t *read_rec;
};

int bam_args_check(const BamArgs &a)
{
    const kiss_hip_sam_input *in = a.in;
    if (!in || !a.read_rec) return KISS_HIP_E_INVALID;
    if (!in->reads || !in->read_index || !in->names || !in->name_off || !in->name_len || !in->alns || !in->cigar || !in->cigar_index || !in->hits ||
        !in->hit_index)
        return KISS_HIP_E_INVALID;
    if (in->md && !in->md_index) return KISS_HIP_E_INVALID;
    if (!in->R || !in->ref_names || !in->ref_name_index || !in->bounds) return KISS_HIP_E_INVALID;
    if (a.bam_capacity && !a.bam) return KISS_HIP_E_INVALID;
    if (in->pairs && (in->Q & 1ull)) return KISS_HIP_E_INVALID;
    if (in->Q >= (1ull << 31) || in->C > 0xFFFFFFFFull || in->R > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int bam_zero_reads(kiss_hip_ctx *ctx, const BamArgs &a)
{
    KTRY(kiss_zero_u32(ctx, a.read_rec, 2));
    if (a.rec_index) KTRY(kiss_zero_u32(ctx, a.rec_index, 2));
    KCHECK(hipStreamSynchronize(ctx->stream));
    return KISS_HIP_OK;
}

int bam_steps(kiss_hip_ctx *ctx, const BamArgs &a, kiss_hip_bam_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const kiss_hip_sam_input &u = *a.in;
    const uint64_t Q = u.Q;
    if (Q == 0) return bam_zero_reads(ctx, a);
    FmCtl<SAM_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, BAM_SLOT_CTL));
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
    DevBuf per_read; // read_rec (scanned in place), then a flag per read
    KTRY(per_read.take(ctx, BAM_SLOT_READS, (Q + 1) * 8 + Q * 4));
    uint64_t *const rr = (uint64_t *)per_read.p;
    uint32_t *const flag = (uint32_t *)(rr + (Q + 1));
    SamIn in{u.reads, u.read_index, u.qual, u.names, u.name_off, u.name_len, (const uint32_t *)u.alns, u.cigar, u.cigar_index,
             (const uint32_t *)u.hits, u.hit_index, (const uint32_t *)u.pairs, u.source, u.md, u.md_index, u.ref_names, u.ref_name_index, u.bounds,
             Q, u.C, u.R, u.first_alns, H, 0};
    KTRY(kiss_zero_u32(ctx, flag, Q));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, Q);
        const uint64_t most = u.C > H ? u.C : H;
        if (most)
            hipLaunchKernelGGL(k_sam_check, dim3(fm_grid(most, SAM_THREADS)), threads, 0, ctx->stream, u.cigar_index, u.C, u.md ? u.md_index : nullptr, H,
                               d_ctl);
        hipLaunchKernelGGL(k_bam_count, dim3(fm_grid(Q, SAM_THREADS)), threads, 0, ctx->stream, in, rr, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, rr, rr, Q + 1));
    uint64_t recs = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&recs, rr + Q, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipStreamSynchronize(ctx->stream));
    if (h[SAM_BADIN]) return KISS_HIP_E_INVALID; // a cigar or md index decreases
    if (h[SAM_BAD]) {
        rep.bad = h[SAM_BAD];
        rep.first_bad = ~h[SAM_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    rep.records = recs;
    rep.unmapped_records = h[SAM_UNMAPPED];
    if (recs > 0xFFFFFFFFull || (recs + 1) / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    DevBuf per_rec;
    KTRY(per_rec.take(ctx, BAM_SLOT_RECS, (recs + 1) * 8));
    uint64_t *const size = (uint64_t *)per_rec.p; // (scanned in place)
    in.lines = recs;
    const dim3 grid((unsigned)div_up(recs, SAM_WAVES)); // (a wave per record; recs < 2^32)
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, recs);
        hipLaunchKernelGGL(k_bam_size, grid, threads, 0, ctx->stream, in, (const uint64_t *)rr, size, flag, d_ctl);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, size, size, recs + 1));
    uint64_t total = 0;
    KTRY(ctl.fetch());
    KCHECK(hipMemcpyAsync(&total, size + recs, 8, hipMemcpyDeviceToHost, ctx->stream));
    ev.mark(1);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_count = ev.ms(0, 1);
    if (h[SAM_BAD]) { // a record that BAM cannot hold
        rep.records = rep.unmapped_records = 0;
        rep.bad = h[SAM_BAD];
        rep.first_bad = ~h[SAM_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    rep.bam_bytes = total;
    rep.longest = h[SAM_LONGEST];
    // (the totals are in the report: the caller's second call)
    if (a.bam_capacity < total || (a.rec_index && a.rec_capacity < recs)) return KISS_HIP_E_INVALID;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, recs);
        hipLaunchKernelGGL(k_bam_emit, grid, threads, 0, ctx->stream, in, (const uint64_t *)rr, (const uint64_t *)size, a.bam, a.rec_index,
                           a.read_rec);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    KCHECK(hipStreamSynchronize(ctx->stream));
    rep.ms_emit = ev.ms(1, 2);
    return KISS_HIP_OK;
}

struct BgzfPlan {
    uint32_t bb;
    uint64_t blocks, out_bytes;
};
int bgzf_plan(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, const uint8_t *out, uint64_t out_capacity, BgzfPlan &p)
{
    p.bb = block_bytes ? block_bytes : KISS_HIP_BGZF_BLOCK_DEFAULT;
    if (p.bb > KISS_HIP_BGZF_BLOCK_MAX) return KISS_HIP_E_INVALID;
    if ((n && !data) || (out_capacity && !out)) return KISS_HIP_E_INVALID;
    if (n > (1ull << 62)) return KISS_HIP_E_UNSUPPORTED;
    p.blocks = div_up(n, (uint64_t)p.bb);
    p.out_bytes = n + (uint64_t)KISS_HIP_BGZF_OVERHEAD * p.blocks + (eof ? KISS_HIP_BGZF_EOF_BYTES : 0u);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_fmi_bam_dev(kiss_hip_ctx *ctx, const kiss_hip_sam_input *in, uint8_t *bam, uint64_t bam_capacity, uint64_t *rec_index,
                         uint64_t rec_capacity, uint64_t *read_rec, kiss_hip_bam_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_bam_report rep{};
    if (report) *report = rep;
    const BamArgs a{in, bam, bam_capacity, rec_index, rec_capacity, read_rec};
    KTRY(bam_args_check(a));
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    int rc = bam_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_fmi_bam_host(const kiss_hip_sam_input *in, uint8_t *bam, uint64_t bam_capacity, uint64_t *rec_index, uint64_t rec_capacity,
                          uint64_t *read_rec, kiss_hip_bam_report *report, int device)
{
    if (report) *report = kiss_hip_bam_report{};
    const BamArgs a{in, bam, bam_capacity, rec_index, rec_capacity, read_rec};
    KTRY(bam_args_check(a));
    const kiss_hip_sam_input &u = *in;
    const uint64_t Q = u.Q, C = u.C, R = u.R;
    if (Q == 0) {
        read_rec[0] = 0;
        if (rec_index) rec_index[0] = 0;
        return KISS_HIP_OK;
    }
    if (!fm_index_ascending(u.read_index, Q, true) || !fm_index_ascending(u.hit_index, Q, false) || !fm_index_ascending(u.cigar_index, C, false) ||
        !fm_index_ascending(u.ref_name_index, R, false))
        return KISS_HIP_E_INVALID;
    const uint64_t H = u.hit_index[Q];
    if (H > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    if (u.md && !fm_index_ascending(u.md_index, H, false)) return KISS_HIP_E_INVALID;
    uint64_t name_bytes = 0;
    for (uint64_t q = 0; q < Q; q++)
        if (name_bytes < u.name_off[q] + u.name_len[q]) name_bytes = u.name_off[q] + u.name_len[q];
    const uint64_t bases = u.read_index[Q];
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
        d.ref_names = st2.up(u.ref_names, u.ref_name_index[R]);
        d.ref_name_index = st2.up(u.ref_name_index, (R + 1) * 8);
        d.bounds = st2.up(u.bounds, (R + 1) * 8);
        uint64_t *drr = st2.room<uint64_t>(true, (Q + 1) * 8);
        if (st2.rc) return st2.rc;
        // the sizing call first: the room on the device is the total, whatever capacity the caller names
        kiss_hip_bam_report r{};
        int rc = kiss_hip_fmi_bam_dev(ctx, &d, nullptr, 0, nullptr, 0, drr, &r, nullptr);
        uint8_t *dbam = nullptr;
        uint64_t *dri = nullptr;
        if (rc == KISS_HIP_E_INVALID && r.bam_bytes && r.bam_bytes <= bam_capacity && (!rec_index || r.records <= rec_capacity)) {
            dbam = st2.room<uint8_t>(true, r.bam_bytes);
            dri = st2.room<uint64_t>(rec_index != nullptr, (r.records + 1) * 8);
            if (st2.rc) return st2.rc;
            rc = kiss_hip_fmi_bam_dev(ctx, &d, dbam, r.bam_bytes, dri, r.records, drr, &r, nullptr);
        }
        if (report) *report = r;
        if (rc) return rc;
        st2.down(bam, dbam, r.bam_bytes);
        if (rec_index) st2.down(rec_index, dri, (r.records + 1) * 8);
        st2.down(read_rec, drr, (Q + 1) * 8);
        return st2.rc;
    });
}

int kiss_hip_bgzf_dev(kiss_hip_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                      kiss_hip_bgzf_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx);
    kiss_hip_bgzf_report rep{};
    if (report) *report = rep;
    BgzfPlan p;
    KTRY(bgzf_plan(data, n, block_bytes, eof, out, out_capacity, p));
    if (!ctx) return KISS_HIP_E_INVALID;
    rep.blocks = p.blocks;
    rep.out_bytes = p.out_bytes;
    if (report) *report = rep;
    if (out_capacity < p.out_bytes) return KISS_HIP_E_INVALID; // (the totals are in the report)
    if (!p.out_bytes) return KISS_HIP_OK;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    kiss_opts_refresh(ctx);
    ev.mark(0);
    int rc = KISS_HIP_OK;
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        const uint64_t want = p.blocks ? p.blocks : 1;
        hipLaunchKernelGGL(k_bgzf, dim3((unsigned)(want < BGZF_MAX_BLOCKS ? want : BGZF_MAX_BLOCKS)), dim3(BGZF_THREADS), 0, ctx->stream, data, n, p.bb,
                           p.blocks, eof, out);
        if (hipGetLastError() != hipSuccess) rc = KISS_HIP_E_HIP;
    }
    ev.mark(1);
    if (rc == KISS_HIP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = KISS_HIP_E_HIP;
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_bgzf_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, int eof, uint8_t *out, uint64_t out_capacity,
                       kiss_hip_bgzf_report *report, int device)
{
    kiss_hip_bgzf_report rep{};
    if (report) *report = rep;
    BgzfPlan p;
    KTRY(bgzf_plan(data, n, block_bytes, eof, out, out_capacity, p));
    rep.blocks = p.blocks;
    rep.out_bytes = p.out_bytes;
    if (report) *report = rep;
    if (out_capacity < p.out_bytes) return KISS_HIP_E_INVALID;
    if (!p.out_bytes) return KISS_HIP_OK;
    return kiss_one_shot_cached(device, fm_host_max_n(0, 0), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *d = st.up(data, n);
        uint8_t *o = st.room<uint8_t>(true, p.out_bytes);
        if (st.rc) return st.rc;
        const int rc = kiss_hip_bgzf_dev(ctx, d, n, block_bytes, eof, o, p.out_bytes, report, nullptr);
        if (rc) return rc;
        st.down(out, o, p.out_bytes);
        return st.rc;
    });
}

} // extern "C"
