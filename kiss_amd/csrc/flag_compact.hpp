// flag_compact.hpp -- the toolbox the LMS sort (lms_sort.hip) and the two rank-doubling forms (doubling.hip) share: flag the
// items of a sorted list that are still tied with a neighbour, compact them into the tied-segment arrays and retire the
// rest; totals of flag words; the members of big groups sorted apart.  Kernels and drivers are in flag_compact.hip.
#pragma once
#include "kiss_internal.hpp"

namespace kiss_fc {

constexpr int LS_THREADS = 256; // one item per thread: the kernels of the three units that are not tiled

// where a segment starts: FC_KEY = the key changes, FC_KEY_SEG = the key or the segment id changes,
// FC_HEADS = `key` points at one byte per item (1 = starts a segment)
constexpr int FC_KEY = 0, FC_KEY_SEG = 1, FC_HEADS = 2;

// One flag + compact pass over `count` sorted items.  What is null is not read or written.
struct FcJob {
    int src = FC_KEY;
    const uint64_t *key = nullptr;  // FC_HEADS: the head bytes
    const uint32_t *seg = nullptr;  // FC_KEY_SEG
    const uint32_t *pos = nullptr;
    const uint32_t *slot = nullptr; // null: an item's slot is its index in the list
    uint64_t count = 0;
    int cmp_shift = 0;              // keys are compared above this bit
    int last_round = 0;             // nothing survives: every item retires
    // ---- what a retiring item leaves behind
    uint32_t *out = nullptr;        // out[slot] = position (out == pos without slots: the list is in place already)
    uint32_t *isa = nullptr;        // isa[position >> isa_shift] = slot
    int isa_shift = 0;
    uint32_t *octx = nullptr;       // round 0: octx[slot] = the context word in the key's payload bits, 0 for slots still tied
    uint32_t *nctx = nullptr;       // round 0 (k_fc0_compact): the survivors' context words, parallel to the survivor arrays
    uint32_t *tmark = nullptr;      // the LMS sort's retirements: taint marks (and tie flags in ctx->hfar)
    const uint64_t *payload = nullptr; // with tmark: words whose low KISS_KEY_CTX bits are the items' context words
    uint32_t *cfix = nullptr;       // cfix[slot] = context word of the retiring item's own position, gathered from the text
};
// where the survivors go: positions, slots, dense segment ids, and the first survivor of every segment
struct FcOut {
    uint32_t *npos, *nslot, *nseg, *nsegstart;
};

// the two halves of a pass, so that a caller can size buffers in between.  fc_count leaves (survivors << 32 | surviving
// segments) in d_total[0] and the tile offsets where fc_compact finds them.
int fc_count(kiss_hip_ctx *ctx, const FcJob &job, uint64_t *d_total);
int fc_compact(kiss_hip_ctx *ctx, const FcJob &job, const FcOut &to, bool *nctx_written = nullptr);

// tile counts are in tcnt: exclusive scan over the tiles into tex, grand total into d_total[0]; host_total (optional): wait
// for it.  Without it the total stays on the device for a caller that launches more before it reads.
int tiles_total(kiss_hip_ctx *ctx, const uint64_t *tcnt, uint64_t *tex, uint64_t tiles, uint64_t *d_total,
                uint64_t *host_total = nullptr);
// the same for one flag word per item: ex = exclusive scan of flags, d_total[0] = the grand total
int flags_total(kiss_hip_ctx *ctx, const uint64_t *flags, uint64_t *ex, uint64_t count, uint64_t *d_total,
                uint64_t *host_total = nullptr);

// round 0 in one pass over the sorted keys (k_fc0_onepass): can it run for `count` items?
bool fc0_onepass_fits(const kiss_hip_ctx *ctx, uint64_t count);
// One attempt: survivors beyond ctx->t_cap are counted but not stored (the caller regrows and runs it again).  rec != null:
// tied pairs leave as records in three columns of rcol words.  *tot = survivors << 32 | segments.
struct Fc0Job {
    const uint64_t *key;
    const uint32_t *pos;
    uint64_t count;
    int cmp_shift;
    uint32_t *octx, *nctx;
    uint32_t *rec;
    uint32_t rcol;
};
int fc0_onepass(kiss_hip_ctx *ctx, const Fc0Job &job, const FcOut &to, uint64_t *d_total, uint64_t *tot, uint64_t *npairs);

// the items of big segments after a refinement round, from the byte flags `bb` (1: member of a big segment, 3: its first):
// count -> *tot = items << 32 | segments; compact into the compact arrays (key == null: no keys are carried along), whose
// segment starts get their end entry (bsegstart[nbigseg] = nbig)
struct BigbOut {
    uint64_t *bkey;
    uint32_t *bpos, *bseg, *bslot, *bsegstart;
};
int bigb_count(kiss_hip_ctx *ctx, const uint8_t *bb, uint64_t count, uint64_t *d_total, uint64_t *tot);
int bigb_compact(kiss_hip_ctx *ctx, const uint8_t *bb, const uint64_t *key, const uint32_t *pos, const uint32_t *slot,
                 uint64_t count, const BigbOut &to, uint64_t nbig, uint64_t nbigseg);

// Members of big groups of a list (flags[i] = (1 << 32) | starts-a-group, ex = its scan): pulled out, radix sorted on
// (group, key bits from key_lo_bit up), written to okey / opos where they came from.  The sort's buffers are the caller's
// scratch; bidx remembers where each member came from.
struct BigSort {
    const uint64_t *key;
    const uint32_t *pos;
    uint64_t count; // the list
    const uint64_t *flags, *ex;
    uint64_t nbig, ngroups;
    int key_lo_bit;
    uint64_t *kbuf[2];
    uint32_t *pbuf[2], *sbuf[2], *bidx;
    uint64_t *okey;
    uint32_t *opos;
    unsigned sync_points = 0; // hooks build (KISS_HIP_LX_SYNC_POINTS): bits 2 / 3 / 4 = wait after extract / sort / write back
};
int sort_big_members(kiss_hip_ctx *ctx, const BigSort &b);

// *p = v (and *zero_me = 0) on the ctx stream, after what is queued there
void set_u32(kiss_hip_ctx *ctx, uint32_t *p, uint32_t v, uint32_t *zero_me = nullptr);
int read_u64(kiss_hip_ctx *ctx, const void *dptr, uint64_t *out);
int bits_for(uint64_t count); // bits that tell `count` values apart

} // namespace kiss_fc
