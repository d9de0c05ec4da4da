// gsr_mailbox.h -- the words a frame's kernels write into mapped host memory, named once for both sides (no HIP: the kernels include it
// through gsr_device.h, the host's frame outcome through gsr_frame_plan.h).  DESIGN.md section 4 ("The mailbox") is the prose.
//
// FrameSlot::h_total[4], written by the publishing workgroup of k_bin_ranges / k_bin_place (k_binning.h: bn_ranges):
//   [0]  ticket << 32 | pair count                  (GSR_MB_TOO_MANY_PAIRS: the lists would exceed GSR_MAX_PAIRS)
//   [1]  kept << 32   | hint bits                   (kept = splats that reached the depth sort; hints: GSR_HINT_*)
//   [2]  surviving clusters (k_cluster_cull)
//   [3]  largest kept key << 32 | smallest kept key (relative to the frame's key_min; 0 when nothing was kept)
// FrameSlot::h_end, written first by a culled frame's frame-end kernel (k_blend.h: gsr_sum_work):
//        ticket << 32 | GSR_END_HORIZON_BROKE
// The host recognises a word of THIS frame by the ticket in the upper half of word 0 / of h_end (wait_mailbox).
#pragma once
#include <stdint.h>

// hint bits of word 1.  Bits 0..3 are k_sum_work's verdicts on the frame BEFORE (GsrSumArgs' lazy_hint word, forwarded);
// bits 5 and 6 are about this frame.
static constexpr uint32_t GSR_HINT_LAZY_PAYS = 1u;          // lazy colour would pay for a frame like the last one
static constexpr uint32_t GSR_HINT_ORDER_PAYS = 2u;         // a heaviest-first tile order would pay (k_tile_order)
static constexpr uint32_t GSR_HINT_CULL_PAYS = 4u;          // occlusion culling has something to work with
static constexpr uint32_t GSR_HINT_PREFIX_CHEAPER = 8u;     // the list-prefix colour pass evaluates fewer colours than one per kept splat
static constexpr uint32_t GSR_HINT_VERDICTS = 31u;          // (the bits k_sum_work's word may carry)
static constexpr uint32_t GSR_HINT_SORT_GAVE_UP = 32u;      // the small-frame sort gave a bucket up: the frame's lists mean nothing
static constexpr uint32_t GSR_HINT_DEPTH_COVERED = 64u;     // the frame's depth buffer holds something in front of the far plane
static constexpr uint32_t GSR_MB_TOO_MANY_PAIRS = 0xffffffffu;
static constexpr uint32_t GSR_END_HORIZON_BROKE = 1u;       // h_end: a tile of the culled frame looked past its horizon

// the host's reading of words 0..3 (once word 0 carries the frame's ticket)
struct GsrMailbox {
    uint32_t pairs = 0, hints = 0, kept = 0, clusters = 0, key_lo = 0, key_hi = 0;
    static GsrMailbox read(const volatile unsigned long long* box)
    {
        GsrMailbox m;
        const unsigned long long w1 = box[1], w3 = box[3];
        m.pairs = (uint32_t)box[0];
        m.hints = (uint32_t)w1; m.kept = (uint32_t)(w1 >> 32);
        m.clusters = (uint32_t)box[2];
        m.key_lo = (uint32_t)w3; m.key_hi = (uint32_t)(w3 >> 32);
        return m;
    }
    bool has(uint32_t hint) const { return (hints & hint) != 0u; }
};
