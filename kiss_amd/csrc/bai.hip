// bai.hip -- the BAI index of a coordinate-sorted BAM file, built on the GPU from the unframed records, their CSR and the offsets
// of the blocks they are framed in (kiss_hip_bai_*).  The definition is in include/kiss_hip_bai.h and restated in
// tests/bai_model.py; DESIGN.md 4.25.
//
//   blocks  : one lane per entry of block_index (k_bai_blocks): it never decreases, and the largest coff is below 2^48.
//   record  : ONE LANE PER RECORD (k_bai_record): its two index entries, the five words of its head read from naturally aligned
//             words, every check, the sort's key and the end of its interval.  A cigar of up to 8 ops is summed by the lane; a longer
//             one is handed to the WHOLE WAVE, record after record, 64 ops at a time (65535 ops: 1024 rounds of one load, not 65535).
//             The windows of a reference (n_intv) are an atomic maximum per reference: one per wave while the wave holds one reference.
//   runs    : one lane per record (k_bai_runs): key(r) < key(r - 1) is BAD; "starts a chunk" iff the reference or the bin differs
//             from the predecessor's.  kiss_scan_u64 numbers the chunks in file order, and makes the window CSR over the references.
//   windows : one lane per record (k_bai_windows): FILE ORDER IS beg ORDER, so the smallest voff over a window is that of the lowest
//             record index: a u32 atomicMin of the record index into the window array, preset to all ones.  A record of up to 4
//             windows is the lane's; a longer one (2^29 bases: 32768 windows) is handed to the whole wave.  Sorted records share
//             their windows with their neighbours, so a lane leaves a window that the lane in front covers as well to that lane:
//             a wave sends a handful of atomics, not 64 to one address (2 * 10^5 records: the kernel 75.6 -> 6.0 us).
//             The lane that starts a chunk writes its (key, number) into the ctx's radix arrays and its first record.
//   sort    : kiss_radix_sort, stable, over (ref << 16 | bin) moved to the top of the u64 (as bam_sort.hip): the bins of a reference
//             ascend, the chunks of a bin stay in file order.
//   sizes   : the file is a row of pieces -- per reference a head (n_bin), its chunks (16 bytes, 24 where one heads a bin), a tail
//             (the pseudo-bin, n_intv, the ioffsets) -- and piece 2 ref + (chunks in front) [+ 1 ..] is where each stands, so ONE
//             kiss_scan_u64 gives every byte offset.  The chunks and records in front of a reference are found by a search in the
//             sorted keys: no counter per reference.
//   emit    : one lane per reference, per chunk, per window.  A window that no record covers takes the next covered one to its
//             right: that is the first record of the reference that begins behind the window (a search in the keys), because a
//             record in front of it that reached past the window would cover it.
//
// ADDRESSING.  As bam_sort.hip: 64-bit offsets from kernel-argument base pointers, 64-bit values cross lanes as two halves, every
// load and store naturally aligned: the fields of bai are written as 4-byte words where its address allows and as bytes where not.
// The atomics are vector atomics at device scope in plain HIP.  No LDS, no scratch, no inline assembly.
#include "bam_record.hpp" // the word reads and the check of a record's head, shared with bam_sort.hip
#include "../../include/kiss_hip_bai.h"

namespace {

constexpr int BAI_THREADS = 256;
constexpr uint32_t BAI_LIGHT_OPS = 8;     // a cigar up to here is summed by the record's lane
constexpr uint32_t BAI_LIGHT_WINDOWS = 4; // a record up to here marks its windows itself
constexpr uint32_t BAI_BAD_END = 0xFFFFFFFFu;
constexpr uint64_t BAI_NO_KEY = ~0ull;
constexpr uint64_t BAI_COFF_END = 1ull << 48;
// control block of a call (u64 words); BAI_NFIRST holds the largest ~r of a bad record r
enum { BAI_BAD = 0, BAI_NFIRST, BAI_NO_COOR, BAI_UNMAPPED, BAI_BINS, BAI_BLOCKS_BAD, BAI_COFF_BIG, BAI_CTL_WORDS };

__device__ __forceinline__ uint32_t bai_reg2bin(uint32_t beg, uint32_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

// where the blocks stand in the file
struct BaiFrame {
    const uint64_t *rec_index;
    const uint64_t *block_index; // null: stored blocks
    uint64_t file_base;
    uint32_t bb;
};
__device__ __forceinline__ uint64_t bai_voff_at(const BaiFrame &f, uint64_t u)
{
    const uint64_t b = u / f.bb;
    const uint64_t coff = f.file_base + (f.block_index ? bs_ld64(f.block_index + b) : b * (uint64_t)(f.bb + 31u));
    return coff << 16 | (u - b * f.bb);
}
__device__ __forceinline__ uint64_t bai_voff(const BaiFrame &f, uint64_t r) { return bai_voff_at(f, bs_ld64(f.rec_index + r)); }

__device__ __forceinline__ void bai_put32(uint8_t *__restrict__ bai, uint64_t off, uint32_t v)
{
    uint8_t *p = bai + off;
    if (((uintptr_t)p & 3u) == 0) {
        *(uint32_t *)p = v;
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (8 * b));
    }
}
__device__ __forceinline__ void bai_put64(uint8_t *__restrict__ bai, uint64_t off, uint64_t v)
{
    bai_put32(bai, off, (uint32_t)v);
    bai_put32(bai, off + 4, (uint32_t)(v >> 32));
}
// the first i in [lo, hi) with a[i] >= v (hi: none); a ascends
__device__ __forceinline__ uint64_t bai_lower_bound(const uint64_t *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (bs_ld64(a + mid) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One lane per entry of block_index (blocks + 1 of them): no entry is below the one in front of it, and the coff of the block
// that holds the last byte's end, the largest one used, is below 2^48
__global__ __launch_bounds__(BAI_THREADS) void k_bai_blocks(const uint64_t *__restrict__ block_index, uint64_t blocks, uint64_t last, uint64_t file_base,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint64_t b = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (b > blocks) return;
    const uint64_t v = bs_ld64(block_index + b);
    if (b > 0 && v < bs_ld64(block_index + b - 1)) atomicAdd(&ctl[BAI_BLOCKS_BAD], 1ull);
    if (b == last && (v >= BAI_COFF_END || file_base + v >= BAI_COFF_END)) atomicAdd(&ctl[BAI_COFF_BIG], 1ull);
}

// One lane per record: the checks, the key, the end of the interval, the windows of its reference
__global__ __launch_bounds__(BAI_THREADS) void k_bai_record(const uint8_t *__restrict__ bam, uint64_t bam_bytes, const uint64_t *__restrict__ rec_index,
                                                          uint64_t records, uint32_t n_ref, uint64_t *__restrict__ key, uint32_t *__restrict__ end,
                                                          unsigned long long *__restrict__ ref_windows, uint32_t *__restrict__ ref_unmapped,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    const uint32_t lane = lane_id();
    const bool live = r < records;
    bool bad = false, fine = false; // fine: none of the sort's BAD kinds
    uint64_t a = 0, size = 0;
    int32_t ref = -1, pos = -1;
    uint32_t l_name = 0, n_ops = 0, flag = 4;
    if (live) {
        const BsHead h = bs_head(bam, bam_bytes, rec_index, records, n_ref, r);
        bad = h.bad;
        if (h.read) { // (only then are the twenty bytes there to be read)
            a = h.at, size = h.size, ref = h.ref, pos = h.pos;
            l_name = bs_word_at(bam, a + 12) & 0xFFu;
            const uint32_t w16 = bs_word_at(bam, a + 16);
            n_ops = w16 & 0xFFFFu;
            flag = w16 >> 16;
            fine = !bad;
        }
    }
    uint64_t k = BAI_NO_KEY;
    if (fine) k = (uint64_t)(ref == -1 ? n_ref : (uint32_t)ref) << 32 | (uint64_t)(uint32_t)(pos + 1);
    const bool placed = fine && ref >= 0;
    const bool unmapped = (flag & 4u) != 0;
    if (placed && pos == -1) bad = true;
    const bool walk = fine && !unmapped && 36ull + l_name + 4ull * n_ops <= size; // the cigar is read
    if (fine && !unmapped && !walk) bad = true;
    const uint64_t cigar_at = a + 36u + l_name;
    uint64_t reflen = 0;
    bool bad_op = false;
    if (walk && n_ops <= BAI_LIGHT_OPS) {
        for (uint32_t i = 0; i < n_ops; i++) {
            const uint32_t w = bs_word_at(bam, cigar_at + 4ull * i), op = w & 15u;
            bad_op |= op > 8u;
            if ((0x18Du >> op) & 1u) reflen += w >> 4; // M, D, N, =, X
        }
    }
    // the long cigars of the wave, one after the other, 64 ops at a time
    unsigned long long heavy = __ballot(walk && n_ops > BAI_LIGHT_OPS);
    while (heavy) {
        const int l = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const uint64_t at = bs_lane64(cigar_at, l);
        const uint32_t n = (uint32_t)__shfl((int)n_ops, l, 64);
        uint64_t s = 0;
        bool bo = false;
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t w = bs_word_at(bam, at + 4ull * i), op = w & 15u;
            bo |= op > 8u;
            if ((0x18Du >> op) & 1u) s += w >> 4;
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) s += bs_lane64(s, (int)(lane ^ (uint32_t)o));
        const bool any = __ballot(bo) != 0;
        if ((int)lane == l) reflen = s, bad_op = any;
    }
    if (bad_op) bad = true;
    uint64_t e = 0;
    if (placed && !bad) {
        e = (uint64_t)(uint32_t)pos + (unmapped ? 1ull : (reflen ? reflen : 1ull));
        if (e > KISS_HIP_BAI_MAX_END) bad = true;
    }
    if (live) {
        key[r] = k;
        end[r] = bad ? BAI_BAD_END : (uint32_t)e;
        if (bad) atomicMax(&ctl[BAI_NFIRST], (unsigned long long)~r);
    }
    const bool good = placed && !bad;
    // n_intv of the reference: one atomic per wave while the wave holds one reference
    const uint32_t windows = good ? 1u + (uint32_t)((e - 1) >> 14) : 0u;
    const unsigned long long G = __ballot(good);
    if (G) {
        const int lead = __ffsll((long long)G) - 1;
        const int32_t ref0 = __shfl(ref, lead, 64);
        if (__ballot(good && ref != ref0) == 0) {
            uint32_t m = windows;
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                const uint32_t t = (uint32_t)__shfl((int)m, (int)(lane ^ (uint32_t)o), 64);
                m = t > m ? t : m;
            }
            if ((int)lane == lead && m > bs_ld64((const uint64_t *)ref_windows + ref0)) atomicMax(&ref_windows[ref0], (unsigned long long)m);
        } else if (good && windows > bs_ld64((const uint64_t *)ref_windows + ref)) {
            atomicMax(&ref_windows[ref], (unsigned long long)windows);
        }
    }
    if (good && unmapped) atomicAdd(&ref_unmapped[ref], 1u);
    const unsigned long long B = __ballot(bad), N = __ballot(fine && !bad && ref == -1), U = __ballot(good && unmapped);
    if (lane == 0) {
        if (B) atomicAdd(&ctl[BAI_BAD], (unsigned long long)__popcll(B));
        if (N) atomicAdd(&ctl[BAI_NO_COOR], (unsigned long long)__popcll(N));
        if (U) atomicAdd(&ctl[BAI_UNMAPPED], (unsigned long long)__popcll(U));
    }
}

// One lane per record (and one behind the last, which closes the array for the scan): the order, and where a chunk starts
__global__ __launch_bounds__(BAI_THREADS) void k_bai_runs(const uint64_t *__restrict__ key, uint32_t *__restrict__ end, uint64_t records, uint32_t n_ref,
                                                        uint64_t *__restrict__ starts, unsigned long long *__restrict__ ctl)
{
    const uint64_t r = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    bool unsorted = false;
    if (r <= records) {
        uint64_t start = 0;
        if (r < records) {
            const uint64_t k = bs_ld64(key + r), kp = r ? bs_ld64(key + r - 1) : BAI_NO_KEY;
            const uint32_t e = bs_ld32(end + r), ep = r ? bs_ld32(end + r - 1) : BAI_BAD_END;
            unsorted = r > 0 && k != BAI_NO_KEY && kp != BAI_NO_KEY && k < kp && e != BAI_BAD_END; // (a BAD record counts once)
            if (e != BAI_BAD_END && (uint32_t)(k >> 32) < n_ref) { // placed
                start = 1;
                if (ep != BAI_BAD_END && kp != BAI_NO_KEY && (kp >> 32) == (k >> 32))
                    start = bai_reg2bin((uint32_t)kp - 1u, ep) != bai_reg2bin((uint32_t)k - 1u, e) ? 1 : 0;
            }
            if (unsorted) atomicMax(&ctl[BAI_NFIRST], (unsigned long long)~r);
        }
        starts[r] = start;
    }
    const unsigned long long B = __ballot(unsorted);
    if (lane_id() == 0 && B) atomicAdd(&ctl[BAI_BAD], (unsigned long long)__popcll(B));
}

// One lane per record: its windows; the chunk it starts.  cidx: the run flags scanned, records + 1 entries; win_base: the window
// CSR over the references
__global__ __launch_bounds__(BAI_THREADS) void k_bai_windows(const uint64_t *__restrict__ key, const uint32_t *__restrict__ end, uint64_t records,
                                                           uint32_t n_ref, uint64_t placed, const uint64_t *__restrict__ cidx, uint64_t chunks,
                                                           const uint64_t *__restrict__ win_base, uint32_t *__restrict__ win_min, int key_shift,
                                                           uint64_t *__restrict__ chunk_key, uint32_t *__restrict__ chunk_id,
                                                           uint32_t *__restrict__ chunk_first)
{
    const uint64_t r = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    const uint32_t lane = lane_id();
    if (r == 0) chunk_first[chunks] = (uint32_t)placed; // (the records behind the last chunk have no place)
    bool mine = false;
    uint64_t w0 = 0, count = 0; // the record's windows, as places in win_min
    if (r < records) {
        const uint64_t k = bs_ld64(key + r);
        const uint32_t ref = (uint32_t)(k >> 32);
        if (ref < n_ref) {
            mine = true;
            const uint32_t beg = (uint32_t)k - 1u, e = bs_ld32(end + r);
            w0 = bs_ld64(win_base + ref) + (beg >> 14);
            count = (uint64_t)((e - 1u) >> 14) - (beg >> 14) + 1;
            const uint64_t c = bs_ld64(cidx + r);
            if (bs_ld64(cidx + r + 1) != c) {
                chunk_key[c] = ((uint64_t)ref << 16 | bai_reg2bin(beg, e)) << key_shift;
                chunk_id[c] = (uint32_t)c;
                chunk_first[c] = (uint32_t)r;
            }
        }
    }
    // A window that the lane in front covers as well is left to that lane: its record is the lower one (and it leaves the window
    // to the lane in front of it by the same rule; lane 0 leaves none).  Sorted records share their windows with their neighbours,
    // so a wave sends a handful of atomics, not 64 to one address.
    const int before = lane ? (int)lane - 1 : 0;
    const uint64_t p0 = bs_lane64(w0, before), pc = bs_lane64(count, before); // (every lane takes part; count is 0 without a place)
    const uint64_t pn = lane ? pc : 0;
    if (mine && count <= BAI_LIGHT_WINDOWS)
        for (uint64_t i = 0; i < count; i++) {
            const uint64_t w = w0 + i;
            if (w >= p0 && w - p0 < pn) continue;
            if (bs_ld32(win_min + w) > (uint32_t)r) atomicMin(&win_min[w], (uint32_t)r);
        }
    unsigned long long heavy = __ballot(mine && count > BAI_LIGHT_WINDOWS);
    while (heavy) {
        const int l = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const uint64_t at = bs_lane64(w0, l), n = bs_lane64(count, l);
        const uint32_t rec = (uint32_t)(r - lane + (uint32_t)l);
        for (uint64_t i = lane; i < n; i += 64)
            if (bs_ld32(win_min + at + i) > rec) atomicMin(&win_min[at + i], rec);
    }
}

// One lane per chunk in sorted order: its bytes, as piece 2 ref + 1 + s
__global__ __launch_bounds__(BAI_THREADS) void k_bai_chunk_sizes(const uint64_t *__restrict__ skey, uint64_t chunks, int key_shift, uint64_t *__restrict__ items,
                                                               unsigned long long *__restrict__ ctl)
{
    const uint64_t s = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    bool head = false;
    if (s < chunks) {
        const uint64_t k = bs_ld64(skey + s);
        head = s == 0 || bs_ld64(skey + s - 1) != k;
        items[2 * ((k >> key_shift) >> 16) + 1 + s] = head ? 24 : 16;
    }
    const unsigned long long H = __ballot(head);
    if (lane_id() == 0 && H) atomicAdd(&ctl[BAI_BINS], (unsigned long long)__popcll(H));
}

// One lane per reference, and one behind the last: the records and the chunks in front of it, the bytes of its head and tail
__global__ __launch_bounds__(BAI_THREADS) void k_bai_ref_sizes(const uint64_t *__restrict__ key, uint64_t records, const uint64_t *__restrict__ skey,
                                                             uint64_t chunks, int key_shift, uint32_t n_ref, const uint64_t *__restrict__ win_base,
                                                             uint32_t *__restrict__ ref_first, uint32_t *__restrict__ ref_chunk, uint64_t *__restrict__ items)
{
    const uint64_t ref = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (ref > n_ref) return;
    const uint64_t f0 = bai_lower_bound(key, 0, records, ref << 32), c0 = bai_lower_bound(skey, 0, chunks, (ref << 16) << key_shift);
    ref_first[ref] = (uint32_t)f0;
    ref_chunk[ref] = (uint32_t)c0;
    if (ref == n_ref) {
        items[2 * ref + chunks] = 0; // (closes the array for the scan)
        return;
    }
    const uint64_t f1 = bai_lower_bound(key, f0, records, (ref + 1) << 32), c1 = bai_lower_bound(skey, c0, chunks, ((ref + 1) << 16) << key_shift);
    items[2 * ref + c0] = 4;
    items[2 * ref + 1 + c1] = (f1 > f0 ? 40u : 0u) + 4u + 8u * (bs_ld64(win_base + ref + 1) - bs_ld64(win_base + ref));
}

// One lane per reference, and one behind the last for the ends of the file.  ioff[ref]: where its ioffsets stand
__global__ __launch_bounds__(BAI_THREADS) void k_bai_emit_refs(BaiFrame f, uint32_t n_ref, uint64_t records, uint64_t chunks, const uint64_t *__restrict__ win_base,
                                                             const uint32_t *__restrict__ ref_first, const uint32_t *__restrict__ ref_chunk,
                                                             const uint32_t *__restrict__ ref_unmapped, const uint64_t *__restrict__ ioff_of_item,
                                                             uint64_t no_coor, uint64_t *__restrict__ ioff, uint8_t *__restrict__ bai)
{
    const uint64_t ref = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (ref > n_ref) return;
    if (ref == n_ref) {
        bai_put32(bai, 0, 0x01494142u); // "BAI\1"
        bai_put32(bai, 4, n_ref);
        bai_put64(bai, 8 + bs_ld64(ioff_of_item + 2 * ref + chunks), no_coor);
        return;
    }
    const uint64_t f0 = bs_ld32(ref_first + ref), f1 = bs_ld32(ref_first + ref + 1);
    const uint64_t c0 = bs_ld32(ref_chunk + ref), c1 = bs_ld32(ref_chunk + ref + 1);
    const uint64_t head = 8 + bs_ld64(ioff_of_item + 2 * ref + c0);
    uint64_t tail = 8 + bs_ld64(ioff_of_item + 2 * ref + 1 + c1);
    const uint64_t bins = (tail - head - 4 - 16 * (c1 - c0)) / 8; // a chunk takes 16 bytes and 8 more where it heads a bin
    bai_put32(bai, head, (uint32_t)bins + (f1 > f0 ? 1u : 0u));
    if (f1 > f0) {
        const uint64_t un = bs_ld32(ref_unmapped + ref);
        bai_put32(bai, tail, KISS_HIP_BAI_PSEUDO_BIN);
        bai_put32(bai, tail + 4, 2u);
        bai_put64(bai, tail + 8, bai_voff(f, f0));
        bai_put64(bai, tail + 16, bai_voff(f, f1)); // vend(f1 - 1)
        bai_put64(bai, tail + 24, f1 - f0 - un);
        bai_put64(bai, tail + 32, un);
        tail += 40;
    }
    bai_put32(bai, tail, (uint32_t)(bs_ld64(win_base + ref + 1) - bs_ld64(win_base + ref)));
    ioff[ref] = tail + 4;
}

// One lane per chunk in sorted order
__global__ __launch_bounds__(BAI_THREADS) void k_bai_emit_chunks(BaiFrame f, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sid, uint64_t chunks,
                                                               int key_shift, const uint32_t *__restrict__ chunk_first, const uint64_t *__restrict__ off_of_item,
                                                               uint8_t *__restrict__ bai)
{
    const uint64_t s = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (s >= chunks) return;
    const uint64_t k = bs_ld64(skey + s), rb = k >> key_shift;
    uint64_t off = 8 + bs_ld64(off_of_item + 2 * (rb >> 16) + 1 + s);
    if (s == 0 || bs_ld64(skey + s - 1) != k) { // heads its bin: the chunks of the bin are the ones up to the next key
        const uint64_t next = bai_lower_bound(skey, s + 1, chunks, k + (1ull << key_shift)); // (a bin is below 0xFFFF: no carry out of the key)
        bai_put32(bai, off, (uint32_t)(rb & 0xFFFFu));
        bai_put32(bai, off + 4, (uint32_t)(next - s));
        off += 8;
    }
    const uint64_t c = bs_ld32(sid + s);
    bai_put64(bai, off, bai_voff(f, bs_ld32(chunk_first + c)));
    bai_put64(bai, off + 8, bai_voff(f, bs_ld32(chunk_first + c + 1))); // vend of the record in front of the next chunk
}

// One lane per window
__global__ __launch_bounds__(BAI_THREADS) void k_bai_emit_windows(BaiFrame f, const uint64_t *__restrict__ key, uint32_t n_ref, uint64_t windows,
                                                                const uint64_t *__restrict__ win_base, const uint32_t *__restrict__ win_min,
                                                                const uint32_t *__restrict__ ref_first, const uint64_t *__restrict__ ioff,
                                                                uint8_t *__restrict__ bai)
{
    const uint64_t g = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (g >= windows) return;
    const uint64_t ref = bai_lower_bound(win_base, 0, (uint64_t)n_ref + 1, g + 1) - 1; // the last reference whose windows start at or before g
    const uint64_t w = g - bs_ld64(win_base + ref);
    uint64_t r = bs_ld32(win_min + g);
    if (r == 0xFFFFFFFFull) // nobody covers it: the first record that begins behind it (pos + 1 >= (w + 1) << 14 | 1)
        r = bai_lower_bound(key, bs_ld32(ref_first + ref), bs_ld32(ref_first + ref + 1), ref << 32 | (((w + 1) << 14) + 1));
    bai_put64(bai, bs_ld64(ioff + ref) + 8 * w, bai_voff(f, r));
}

// records == 0: one lane per reference and one for the ends
__global__ __launch_bounds__(BAI_THREADS) void k_bai_empty(uint32_t n_ref, uint8_t *__restrict__ bai)
{
    const uint64_t ref = (uint64_t)blockIdx.x * BAI_THREADS + threadIdx.x;
    if (ref > n_ref) return;
    if (ref == n_ref) {
        bai_put32(bai, 0, 0x01494142u);
        bai_put32(bai, 4, n_ref);
        bai_put64(bai, 8 + 8 * ref, 0);
        return;
    }
    bai_put64(bai, 8 + 8 * ref, 0); // n_bin = 0, n_intv = 0
}

struct BaiArgs {
    const uint8_t *bam;
    uint64_t bam_bytes;
    const uint64_t *rec_index;
    uint64_t records;
    uint32_t n_ref;
    uint32_t block_bytes; // (0 resolved)
    const uint64_t *block_index;
    uint64_t file_base;
    uint8_t *bai;
    uint64_t bai_capacity;
};

// what needs no device; the totals go into the report whatever follows
int bai_args_check(BaiArgs &a, kiss_hip_bai_report &rep)
{
    if (!a.rec_index || (a.bam_bytes && !a.bam) || (a.bai_capacity && !a.bai)) return KISS_HIP_E_INVALID;
    if (a.block_bytes > KISS_HIP_BGZF_BLOCK_MAX) return KISS_HIP_E_INVALID;
    if (a.block_bytes == 0) a.block_bytes = KISS_HIP_BGZF_BLOCK_DEFAULT;
    if (a.records == 0 && a.bam_bytes) return KISS_HIP_E_INVALID;
    rep.records = a.records;
    rep.bam_bytes = a.bam_bytes;
    if (a.records > 0xFFFFFFFFull || a.bam_bytes > (1ull << 62) || a.n_ref > 0x7FFFFFFFu) return KISS_HIP_E_UNSUPPORTED;
    if (a.records == 0) {
        rep.bai_bytes = 8 + 8 * (uint64_t)a.n_ref + 8;
        if (a.bai_capacity < rep.bai_bytes) return KISS_HIP_E_INVALID; // (the totals are in the report)
        return KISS_HIP_OK;
    }
    if (a.file_base >= BAI_COFF_END) return KISS_HIP_E_UNSUPPORTED;
    return KISS_HIP_OK;
}

int bai_steps(kiss_hip_ctx *ctx, const BaiArgs &a, kiss_hip_bai_report &rep, FmEvents &ev)
{
    kiss_opts_refresh(ctx);
    const uint64_t n = a.records, R = a.n_ref;
    const dim3 threads(BAI_THREADS);
    if (n == 0) {
        hipLaunchKernelGGL(k_bai_empty, dim3(fm_grid(R + 1, BAI_THREADS)), threads, 0, ctx->stream, a.n_ref, a.bai);
        KCHECK(hipGetLastError());
        KCHECK(hipStreamSynchronize(ctx->stream));
        return KISS_HIP_OK;
    }
    // the chunks (at most one per record) are sorted in the ctx's LMS key arrays; the pieces of the file are scanned in its scratch
    const uint64_t pieces = n + 2 * R + 2;
    if (n > ctx->m_cap || pieces / 4096 + 16 > ctx->scan_tmp_cap) return KISS_HIP_E_UNSUPPORTED;
    const uint64_t blocks = div_up(a.bam_bytes, a.block_bytes), last = a.bam_bytes / a.block_bytes;
    const int key_bits = fm_bits(R + 1, 32) + 16; // ref is 0 .. n_ref (the searches look for n_ref too), the bin is below 2^16
    const int key_shift = 64 - (key_bits + 7) / 8 * 8;
    FmCtl<BAI_CTL_WORDS> ctl;
    KTRY(ctl.take(ctx, FM_SLOT_BAI_CTL));
    FmSlab rs, fs;
    const uint64_t o_key = rs.carve(n * 8), o_starts = rs.carve((n + 1) * 8), o_end = rs.carve(n * 4), o_first = rs.carve((n + 1) * 4);
    const uint64_t o_win = fs.carve((R + 1) * 8), o_ioff = fs.carve((R + 1) * 8), o_unm = fs.carve((R + 1) * 4), o_rfirst = fs.carve((R + 1) * 4),
                   o_rchunk = fs.carve((R + 1) * 4);
    DevBuf rec, refs, items_buf;
    KTRY(rec.take(ctx, FM_SLOT_BAI_REC, rs.size));
    KTRY(refs.take(ctx, FM_SLOT_BAI_REF, fs.size));
    KTRY(items_buf.take(ctx, FM_SLOT_BAI_ITEMS, pieces * 8));
    uint8_t *const rp = (uint8_t *)rec.p, *const fp = (uint8_t *)refs.p;
    uint64_t *const key = (uint64_t *)(rp + o_key), *const starts = (uint64_t *)(rp + o_starts), *const items = (uint64_t *)items_buf.p;
    uint32_t *const end = (uint32_t *)(rp + o_end), *const chunk_first = (uint32_t *)(rp + o_first);
    uint64_t *const win_base = (uint64_t *)(fp + o_win), *const ioff = (uint64_t *)(fp + o_ioff);
    uint32_t *const ref_unm = (uint32_t *)(fp + o_unm), *const ref_first = (uint32_t *)(fp + o_rfirst), *const ref_chunk = (uint32_t *)(fp + o_rchunk);
    unsigned long long *const h = ctl.h;
    const BaiFrame frame{a.rec_index, a.block_index, a.file_base, a.block_bytes};
    uint64_t totals[2] = {0, 0}; // windows, chunks
    ev.mark(0);
    KTRY(ctl.zero());
    KTRY(kiss_zero_u32(ctx, win_base, (R + 1) * 2));
    KTRY(kiss_zero_u32(ctx, ref_unm, R + 1));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        if (a.block_index) {
            if (div_up(blocks + 1, BAI_THREADS) > 0x7FFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
            hipLaunchKernelGGL(k_bai_blocks, dim3(fm_grid(blocks + 1, BAI_THREADS)), threads, 0, ctx->stream, a.block_index, blocks, last, a.file_base, ctl.d);
        }
        hipLaunchKernelGGL(k_bai_record, dim3(fm_grid(n, BAI_THREADS)), threads, 0, ctx->stream, a.bam, a.bam_bytes, a.rec_index, n, a.n_ref, key, end,
                           (unsigned long long *)win_base, ref_unm, ctl.d);
        hipLaunchKernelGGL(k_bai_runs, dim3(fm_grid(n + 1, BAI_THREADS)), threads, 0, ctx->stream, (const uint64_t *)key, end, n, a.n_ref, starts, ctl.d);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, win_base, win_base, R + 1));
    KTRY(kiss_scan_u64(ctx, starts, starts, n + 1));
    ev.mark(1);
    KCHECK(hipMemcpyAsync(&totals[0], win_base + R, 8, hipMemcpyDeviceToHost, ctx->stream));
    KCHECK(hipMemcpyAsync(&totals[1], starts + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    KTRY(ctl.fetch_sync());
    rep.ms_record = ev.ms(0, 1);
    if (h[BAI_BLOCKS_BAD]) return KISS_HIP_E_INVALID;
    if (h[BAI_BAD]) {
        rep.bad = h[BAI_BAD];
        rep.first_bad = ~h[BAI_NFIRST];
        return KISS_HIP_E_INVALID;
    }
    // (behind the records: an input that is BAD and too far is BAD, with or without a block_index, as the model has it)
    if (h[BAI_COFF_BIG] || (!a.block_index && a.file_base + last * (uint64_t)(a.block_bytes + 31u) >= BAI_COFF_END)) return KISS_HIP_E_UNSUPPORTED;
    const uint64_t W = totals[0], chunks = totals[1], placed = n - h[BAI_NO_COOR];
    if (W > 0xFFFFFFFFull) return KISS_HIP_E_UNSUPPORTED;
    rep.no_coor = h[BAI_NO_COOR];
    rep.unmapped_placed = h[BAI_UNMAPPED];
    rep.mapped = placed - h[BAI_UNMAPPED];
    rep.windows = W;
    rep.chunks = chunks;
    DevBuf win;
    KTRY(win.take(ctx, FM_SLOT_BAI_WIN, (W + 1) * 4));
    uint32_t *const win_min = (uint32_t *)win.p;
    if (W) KTRY(kiss_fill_u32(ctx, win_min, 0xFFFFFFFFu, W));
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n);
        hipLaunchKernelGGL(k_bai_windows, dim3(fm_grid(n, BAI_THREADS)), threads, 0, ctx->stream, (const uint64_t *)key, (const uint32_t *)end, n, a.n_ref, placed,
                           (const uint64_t *)starts, chunks, (const uint64_t *)win_base, win_min, key_shift, ctx->keyA, ctx->posA, chunk_first);
        KCHECK(hipGetLastError());
    }
    ev.mark(2);
    RadixBufs rb = kiss_ctx_radix_bufs(ctx);
    int res = 0;
    if (chunks) KTRY(kiss_radix_sort(ctx, rb, chunks, key_shift, 0, &res));
    const uint64_t *const skey = rb.key[res];
    const uint32_t *const sid = rb.pos[res];
    ev.mark(3);
    const uint64_t n_items = chunks + 2 * R + 1; // (the last one closes the array)
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n_items);
        if (chunks) hipLaunchKernelGGL(k_bai_chunk_sizes, dim3(fm_grid(chunks, BAI_THREADS)), threads, 0, ctx->stream, skey, chunks, key_shift, items, ctl.d);
        hipLaunchKernelGGL(k_bai_ref_sizes, dim3(fm_grid(R + 1, BAI_THREADS)), threads, 0, ctx->stream, (const uint64_t *)key, n, skey, chunks, key_shift, a.n_ref,
                           (const uint64_t *)win_base, ref_first, ref_chunk, items);
        KCHECK(hipGetLastError());
    }
    KTRY(kiss_scan_u64(ctx, items, items, n_items));
    uint64_t body = 0;
    KCHECK(hipMemcpyAsync(&body, items + n_items - 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    KTRY(ctl.fetch_sync());
    rep.bins = h[BAI_BINS];
    rep.bai_bytes = 8 + body + 8;
    if (a.bai_capacity < rep.bai_bytes) return KISS_HIP_E_INVALID; // (the totals are in the report, nothing is written)
    {
        KTimer t(ctx, KISS_HIP_K_FM_QUERY, n_items + W);
        hipLaunchKernelGGL(k_bai_emit_refs, dim3(fm_grid(R + 1, BAI_THREADS)), threads, 0, ctx->stream, frame, a.n_ref, n, chunks, (const uint64_t *)win_base,
                           (const uint32_t *)ref_first, (const uint32_t *)ref_chunk, (const uint32_t *)ref_unm, (const uint64_t *)items, rep.no_coor, ioff, a.bai);
        if (chunks)
            hipLaunchKernelGGL(k_bai_emit_chunks, dim3(fm_grid(chunks, BAI_THREADS)), threads, 0, ctx->stream, frame, skey, sid, chunks, key_shift,
                               (const uint32_t *)chunk_first, (const uint64_t *)items, a.bai);
        if (W)
            hipLaunchKernelGGL(k_bai_emit_windows, dim3(fm_grid(W, BAI_THREADS)), threads, 0, ctx->stream, frame, (const uint64_t *)key, a.n_ref, W,
                               (const uint64_t *)win_base, (const uint32_t *)win_min, (const uint32_t *)ref_first, (const uint64_t *)ioff, a.bai);
        KCHECK(hipGetLastError());
    }
    ev.mark(4);
    KTRY(kiss_radix_check(ctx)); // (synchronises)
    rep.ms_window = ev.ms(1, 2);
    rep.ms_sort = ev.ms(2, 3);
    rep.ms_emit = ev.ms(3, 4);
    return KISS_HIP_OK;
}

} // namespace

extern "C" {

int kiss_hip_bai_dev(kiss_hip_ctx *ctx, const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records,
                     uint32_t n_ref, uint32_t block_bytes, const uint64_t *block_index, uint64_t file_base, uint8_t *bai,
                     uint64_t bai_capacity, kiss_hip_bai_report *report, void *stream)
{
    KissOwnStreamAtExit own_stream_at_exit(ctx); // a ctx keeps no caller's stream past the call (kiss_internal.hpp)
    kiss_hip_bai_report rep{};
    if (report) *report = rep;
    BaiArgs a{bam, bam_bytes, rec_index, records, n_ref, block_bytes, block_index, file_base, bai, bai_capacity};
    int rc = bai_args_check(a, rep);
    if (report) *report = rep;
    if (rc) return rc;
    if (!ctx) return KISS_HIP_E_INVALID;
    KTRY(fm_enter(ctx, stream));
    FmEvents ev(ctx, report != nullptr);
    rc = bai_steps(ctx, a, rep, ev);
    rc = fm_leave(ctx, ev, rc, &rep.ms_total);
    if (report) *report = rep;
    return rc;
}

int kiss_hip_bai_host(const uint8_t *bam, uint64_t bam_bytes, const uint64_t *rec_index, uint64_t records, uint32_t n_ref,
                      uint32_t block_bytes, const uint64_t *block_index, uint64_t file_base, uint8_t *bai, uint64_t bai_capacity,
                      kiss_hip_bai_report *report, int device)
{
    kiss_hip_bai_report rep{};
    BaiArgs a{bam, bam_bytes, rec_index, records, n_ref, block_bytes, block_index, file_base, bai, bai_capacity};
    const int rc0 = bai_args_check(a, rep);
    if (report) *report = rep;
    if (rc0) return rc0;
    if (records == 0) { // the empty index: no device
        for (uint64_t i = 0; i < rep.bai_bytes; i++) bai[i] = 0;
        for (int b = 0; b < 4; b++) bai[b] = (uint8_t)"BAI\1"[b], bai[4 + b] = (uint8_t)(n_ref >> (8 * b));
        return KISS_HIP_OK;
    }
    const uint64_t blocks = div_up(bam_bytes, a.block_bytes);
    return kiss_one_shot_cached(device, fm_host_max_n(0, records + 2 * (uint64_t)n_ref + 2), [&](kiss_hip_ctx *ctx) -> int {
        FmStage st(ctx);
        const uint8_t *dbam = st.up(bam, bam_bytes);
        const uint64_t *dri = st.up(rec_index, (records + 1) * 8);
        const uint64_t *dbi = st.up(block_index, (blocks + 1) * 8);
        uint8_t *dbai = st.room<uint8_t>(bai_capacity > 0, bai_capacity);
        if (st.rc) return st.rc;
        kiss_hip_bai_report got{};
        const int rc = kiss_hip_bai_dev(ctx, dbam, bam_bytes, dri, records, n_ref, a.block_bytes, dbi, file_base, dbai, bai_capacity, &got, nullptr);
        if (report) *report = got;
        if (rc) return rc;
        st.down(bai, dbai, got.bai_bytes);
        return st.rc;
    });
}

} // extern "C"
