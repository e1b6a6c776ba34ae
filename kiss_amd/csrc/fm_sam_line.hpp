// fm_sam_line.hpp -- what the two writers of the mappings share (fm_sam.hip: SAM lines; fm_bam.hip: BAM records): the input on
// the device, the loads, the cross-lane moves of 64-bit values, the checks of the index arrays, the rule that says which reads
// are BAD and how many lines a read has (sam_read_check), and the description of one line (sam_describe: which hit, FLAG, MAPQ,
// place, TLEN, tags).  The rules are those of include/kiss_hip_sam.h and stand here ONCE: one SAM line is one BAM record.
// Included inside the unnamed namespace of a unit, after fm_internal.hpp and kiss_hip_sam.h.
//
// ADDRESSING.  Every address is a kernel-argument base pointer plus a 64-bit offset.  No pointer and no 64-bit offset goes
// through a cross-lane operation as one value: sam_lane64 / sam_up64 below move the two halves.
#pragma once

constexpr int SAM_THREADS = 256;
constexpr int SAM_WAVES = SAM_THREADS / 64;
constexpr unsigned SAM_MAX_BLOCKS = 8192;
constexpr uint32_t SAM_NONE = KISS_HIP_PAIR_NONE;

// control block of a call (u64 words).  SAM_NFIRST holds the largest ~q of a bad read q (the words start at 0).
enum { SAM_BADIN = 0, SAM_H = 1, SAM_BAD = 2, SAM_NFIRST = 3, SAM_UNMAPPED = 4, SAM_LONGEST = 5, SAM_CTL_WORDS = 8 };

// the fields of the records, as u32 offsets
enum { A_RBEG = 2, A_REND = 3, A_TBEG = 4, A_MISM = 7, A_INS = 8, A_DEL = 9, A_WORDS = 12 };
enum { H_ALN = 0, H_FLAGS = 1, H_MAPQ = 2, H_SCORE = 3, H_SUB = 4, H_REF = 7, H_WORDS = 8 };
enum { P_HIT1 = 0, P_HIT2 = 1, P_FLAGS = 2, P_TLEN = 3, P_MAPQ1 = 7, P_MAPQ2 = 8, P_WORDS = 10 };
static_assert(sizeof(kiss_hip_aln) == 4 * A_WORDS && sizeof(kiss_hip_hit) == 4 * H_WORDS && sizeof(kiss_hip_pair) == 4 * P_WORDS, "records");

// Every load of a field or an index entry starts at a multiple of its own size, as in fm_md.hip.
__device__ __forceinline__ uint32_t sam_ld32(const uint32_t *p)
{
    return __hip_atomic_load(const_cast<uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t sam_ld64(const uint64_t *p)
{
    return __hip_atomic_load(const_cast<uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// THE PITFALL these two exist for: the cross-lane builtins move 32 bits and __builtin_amdgcn_readfirstlane returns int, so a
// helper that widens their result to 64 bits extends the SIGN of the low half, and an offset or a pointer whose low half is
// 2^31 or more becomes a wild one -- or not, depending on where the allocator put the array.  A 64-bit value therefore crosses
// lanes as two uint32_t halves that are joined without a sign: (uint64_t)hi << 32 | (uint64_t)(uint32_t)lo.  Nothing else in
// the units that include this file moves a 64-bit value between lanes, and no pointer is moved at all.
__device__ __forceinline__ uint64_t sam_join(uint32_t hi, uint32_t lo) { return (uint64_t)hi << 32 | (uint64_t)(uint32_t)lo; }
// v of lane `from`, in every lane
__device__ __forceinline__ uint64_t sam_lane64(uint64_t v, int from)
{
    const uint32_t lo = (uint32_t)__shfl((unsigned int)(v & 0xFFFFFFFFull), from, 64);
    const uint32_t hi = (uint32_t)__shfl((unsigned int)(v >> 32), from, 64);
    return sam_join(hi, lo);
}
// v of the lane `by` below this one
__device__ __forceinline__ uint64_t sam_up64(uint64_t v, unsigned by)
{
    const uint32_t lo = (uint32_t)__shfl_up((unsigned int)(v & 0xFFFFFFFFull), by, 64);
    const uint32_t hi = (uint32_t)__shfl_up((unsigned int)(v >> 32), by, 64);
    return sam_join(hi, lo);
}
// the sum of v over the lanes below this one; total: over the wave
__device__ __forceinline__ uint64_t sam_wave_excl64(uint64_t v, uint64_t &total)
{
    const uint32_t lane = lane_id();
    uint64_t s = v;
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const uint64_t t = sam_up64(s, o);
        if (lane >= o) s += t;
    }
    total = sam_lane64(s, 63);
    return s - v;
}
__device__ __forceinline__ uint32_t sam_wave_excl32(uint32_t v, uint32_t &total)
{
    const uint32_t lane = lane_id();
    uint32_t s = v;
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

struct SamIn {
    const uint8_t *reads;
    const uint64_t *read_index;
    const uint8_t *qual;
    const uint8_t *names;
    const uint64_t *name_off;
    const uint32_t *name_len;
    const uint32_t *alns; // (the records as u32 words: read field by field)
    const uint32_t *cigar;
    const uint64_t *cigar_index;
    const uint32_t *hits;
    const uint64_t *hit_index;
    const uint32_t *pairs;
    const uint32_t *source;
    const uint8_t *md;
    const uint64_t *md_index;
    const uint8_t *ref_names;
    const uint64_t *ref_name_index;
    const uint64_t *bounds;
    uint64_t Q, C, R, first_alns, H, lines;
};

__device__ __forceinline__ uint32_t sam_aln(const SamIn &in, uint64_t a, int field) { return sam_ld32(in.alns + (a * A_WORDS + (uint64_t)field)); }
__device__ __forceinline__ uint32_t sam_hit(const SamIn &in, uint64_t h, int field) { return sam_ld32(in.hits + (h * H_WORDS + (uint64_t)field)); }
__device__ __forceinline__ uint32_t sam_pair(const SamIn &in, uint64_t p, int field) { return sam_ld32(in.pairs + (p * P_WORDS + (uint64_t)field)); }

// a read_index that does not ascend (a zero-length read too), a hit_index or ref_name_index that decreases; H
__global__ __launch_bounds__(SAM_THREADS) void k_sam_head(const uint64_t *__restrict__ read_index, const uint64_t *__restrict__ hit_index, uint64_t Q,
                                                        const uint64_t *__restrict__ ref_name_index, uint64_t R,
                                                        unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x;
    if (g == 0) ctl[SAM_H] = sam_ld64(hit_index + Q);
    bool bad = false;
    if (g < Q) bad = sam_ld64(read_index + g + 1) <= sam_ld64(read_index + g) || sam_ld64(hit_index + g + 1) < sam_ld64(hit_index + g);
    if (g < R && sam_ld64(ref_name_index + g + 1) < sam_ld64(ref_name_index + g)) bad = true;
    if (__ballot(bad) && lane_id() == 0) ctl[SAM_BADIN] = 1;
}
// a cigar_index or md_index (null: none) that decreases
__global__ __launch_bounds__(SAM_THREADS) void k_sam_check(const uint64_t *__restrict__ cigar_index, uint64_t C, const uint64_t *__restrict__ md_index,
                                                         uint64_t H, unsigned long long *__restrict__ ctl)
{
    const uint64_t g = (uint64_t)blockIdx.x * SAM_THREADS + threadIdx.x;
    bool bad = g < C && sam_ld64(cigar_index + g + 1) < sam_ld64(cigar_index + g);
    if (md_index && g < H && sam_ld64(md_index + g + 1) < sam_ld64(md_index + g)) bad = true;
    if (__ballot(bad) && lane_id() == 0) ctl[SAM_BADIN] = 1;
}

// One lane, read q < Q: BAD or not, its lines, and whether its one line is an unmapped one (SAM_READ_BAD | SAM_READ_UNMAPPED).
// Only the read's own hits, the alignments and records they name once those exist, and its pair are read.
enum : uint32_t { SAM_READ_BAD = 1, SAM_READ_UNMAPPED = 2 };
__device__ __forceinline__ uint32_t sam_read_check(const SamIn &in, uint64_t q, uint64_t &lines)
{
    bool bad = false, unmapped = false;
    const uint64_t L = sam_ld64(in.read_index + q + 1) - sam_ld64(in.read_index + q);
    const uint64_t hb = sam_ld64(in.hit_index + q), he = sam_ld64(in.hit_index + q + 1);
    for (uint64_t h = hb; h < he; h++) {
        const uint64_t a = sam_hit(in, h, H_ALN), ref = sam_hit(in, h, H_REF);
        if (a >= in.C || (in.R && ref >= in.R)) {
            bad = true;
            continue;
        }
        const uint64_t rbeg = sam_aln(in, a, A_RBEG), rend = sam_aln(in, a, A_REND);
        if (rbeg > rend || rend > L) bad = true;
        if (in.R && (uint64_t)sam_aln(in, a, A_TBEG) < sam_ld64(in.bounds + ref)) bad = true;
    }
    lines = he > hb ? he - hb : 1;
    unmapped = he == hb;
    if (in.pairs) {
        const uint32_t mine = sam_pair(in, q >> 1, (q & 1) ? P_HIT2 : P_HIT1);
        if (sam_pair(in, q >> 1, P_FLAGS) & KISS_HIP_PAIR_BAD_INPUT) bad = true;
        if (mine != SAM_NONE && !(hb <= (uint64_t)mine && (uint64_t)mine < he)) bad = true;
        if (mine == SAM_NONE) {
            lines = 1;
            unmapped = true;
        }
    }
    return (bad ? SAM_READ_BAD : 0u) | (unmapped ? SAM_READ_UNMAPPED : 0u);
}

// ---- one line ------------------------------------------------------------------------------------------------------------
// what a wave knows of its line; every field is the same in all lanes
struct SamLine {
    uint64_t q, rb, L; // the read: its number, where it starts in reads, its length
    bool mapped;       // a hit line
    uint32_t flag, mapq;
    bool has_ref; // RNAME is the name of record ref ('*' otherwise)
    uint64_t ref, pos;
    uint64_t a, o0, nops; // a hit line: the alignment, its ops
    uint32_t rbeg, rend;
    int rnext; // 0 '*', 1 '=', 2 the name of record nref
    uint64_t nref, pnext, tlen; // (nref: the record of the place, whenever there is a place)
    bool tneg, rev;
    uint32_t nm, as, xs, ys;
    bool has_xs, has_ys, yt, yr, has_md;
    uint64_t md0, mdl;
};

// are the names of records r1 and r2 the same bytes?  (lanes over the bytes)
__device__ __forceinline__ bool sam_same_name(const SamIn &in, uint64_t r1, uint64_t r2)
{
    if (r1 == r2) return true;
    const uint64_t b1 = sam_ld64(in.ref_name_index + r1), e1 = sam_ld64(in.ref_name_index + r1 + 1);
    const uint64_t b2 = sam_ld64(in.ref_name_index + r2), e2 = sam_ld64(in.ref_name_index + r2 + 1);
    if (e1 - b1 != e2 - b2) return false;
    bool differ = false;
    for (uint64_t k = lane_id(); k < e1 - b1; k += 64) differ = differ || in.ref_names[b1 + k] != in.ref_names[b2 + k];
    return __ballot(differ) == 0ull;
}

// (record, POS, tbeg) of hit h
__device__ __forceinline__ void sam_place(const SamIn &in, uint64_t h, uint64_t &ref, uint64_t &pos, uint32_t &tbeg)
{
    tbeg = sam_aln(in, sam_hit(in, h, H_ALN), A_TBEG);
    ref = sam_hit(in, h, H_REF);
    pos = (uint64_t)tbeg - (in.R ? sam_ld64(in.bounds + ref) : 0ull) + 1ull;
}

// line `line` of a batch without BAD reads (the count pass has looked), read_line = the scanned lines of the reads
__device__ __forceinline__ void sam_describe(const SamIn &in, const uint64_t *__restrict__ read_line, uint64_t line, SamLine &d)
{
    // the largest q with read_line[q] <= line (every read has a line, read_line[Q] = lines > line)
    uint64_t lo = 0, hi = in.Q;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sam_ld64(read_line + mid) <= line) lo = mid;
        else hi = mid;
    }
    const uint64_t q = lo, k = line - sam_ld64(read_line + q);
    d = SamLine{};
    d.q = q;
    d.rb = sam_ld64(in.read_index + q);
    d.L = sam_ld64(in.read_index + q + 1) - d.rb;
    const uint64_t hb = sam_ld64(in.hit_index + q), he = sam_ld64(in.hit_index + q + 1);
    uint32_t bits = 0;
    uint64_t h = hb + k;
    bool place = false, chosen = false, paired = in.pairs != nullptr;
    uint64_t pref = 0, ppos = 0;
    uint32_t ptbeg = 0;
    d.mapped = he > hb;
    uint32_t mine = SAM_NONE, other = SAM_NONE;
    const uint32_t i = (uint32_t)(q & 1);
    if (paired) {
        const uint64_t p = q >> 1;
        mine = sam_pair(in, p, i ? P_HIT2 : P_HIT1);
        other = sam_pair(in, p, i ? P_HIT1 : P_HIT2);
        bits = 1u | (i ? 128u : 64u) | (other != SAM_NONE ? 0u : 8u);
        if (other != SAM_NONE && (sam_hit(in, other, H_FLAGS) & KISS_HIP_HIT_REVERSE)) bits |= 32u;
        if (other != SAM_NONE || mine != SAM_NONE) {
            place = true;
            sam_place(in, other != SAM_NONE ? other : mine, pref, ppos, ptbeg);
        }
        d.mapped = mine != SAM_NONE;
        if (d.mapped) {
            chosen = k == 0;
            if (chosen) h = mine;
            else {
                h = hb + (k - 1);
                if (h >= (uint64_t)mine) h++;
                if (h == hb) bits |= 256u; // the first hit of the read, displaced by the pair
            }
        }
    }
    d.pnext = place ? ppos : 0;
    d.nref = pref;
    d.has_md = false;
    if (!d.mapped) {
        d.flag = bits | 4u;
        d.has_ref = place && in.R;
        d.ref = pref;
        d.pos = place ? ppos : 0;
        d.rnext = place ? 1 : 0;
        return;
    }
    const uint32_t hflags = sam_hit(in, h, H_FLAGS);
    d.a = sam_hit(in, h, H_ALN);
    d.rev = hflags & KISS_HIP_HIT_REVERSE;
    d.flag = bits | (d.rev ? 16u : 0u);
    d.mapq = sam_hit(in, h, H_MAPQ);
    if (!chosen) d.flag |= ((hflags & KISS_HIP_HIT_SECONDARY) ? 256u : 0u) | ((hflags & KISS_HIP_HIT_SUPPLEMENTARY) ? 2048u : 0u);
    uint32_t tbeg;
    sam_place(in, h, d.ref, d.pos, tbeg);
    d.has_ref = in.R != 0;
    d.rbeg = sam_aln(in, d.a, A_RBEG);
    d.rend = sam_aln(in, d.a, A_REND);
    d.o0 = sam_ld64(in.cigar_index + d.a);
    const uint64_t o1 = sam_ld64(in.cigar_index + d.a + 1);
    d.nops = o1 > d.o0 ? o1 - d.o0 : 0;
    d.nm = sam_aln(in, d.a, A_MISM) + sam_aln(in, d.a, A_INS) + sam_aln(in, d.a, A_DEL);
    d.as = sam_hit(in, h, H_SCORE);
    d.has_xs = !(hflags & KISS_HIP_HIT_SECONDARY);
    d.xs = sam_hit(in, h, H_SUB);
    if (in.md) {
        d.has_md = true;
        d.md0 = sam_ld64(in.md_index + h);
        const uint64_t m1 = sam_ld64(in.md_index + h + 1);
        d.mdl = m1 > d.md0 ? m1 - d.md0 : 0;
    }
    if (place) {
        if (!in.R || sam_same_name(in, pref, d.ref)) d.rnext = 1;
        else d.rnext = 2;
    }
    if (paired) {
        const uint64_t p = q >> 1;
        if (chosen) {
            const uint32_t pflags = sam_pair(in, p, P_FLAGS), tl = sam_pair(in, p, P_TLEN);
            d.mapq = sam_pair(in, p, i ? P_MAPQ2 : P_MAPQ1);
            d.yt = pflags & KISS_HIP_PAIR_PROPER;
            if (d.yt) d.flag |= 2u;
            if (other != SAM_NONE) {
                d.has_ys = true;
                d.ys = sam_hit(in, other, H_SCORE);
                if (tl) { // (the place is the partner's)
                    d.tlen = tl;
                    d.tneg = !(tbeg < ptbeg || (tbeg == ptbeg && i == 0));
                }
            }
        } else if (h == hb) {
            d.mapq = 0;
        }
        d.yr = in.source && (uint64_t)sam_ld32(in.source + d.a) >= in.first_alns;
    }
}
