// gsr_frame_plan.h -- the frame driver's DECISIONS as two functions (host code only, no HIP), in the style of gsr_policy.h.
//
//   gsr_plan_frame     what frame_begin reads (options, the slot's hints, the context's flags, the policies, the phase it is given)
//                      -> which regime the frame takes: culled or not, front-slab phase, lazy colour, sort-cache hit, position-keyed
//                      order, small-frame sort, and the grids that follow from them.
//   gsr_frame_outcome  what the frame's mailbox said (gsr_mailbox.h) -> how frame_finish ends the attempt, and the slot's hints and the
//                      kernels' verdicts for the frames behind it.
//
// Neither can change a pixel (every regime renders the same frame); they decide how much work a frame does and when
// an attempt is rendered again.  gsr_api.hip keeps what they decide ON: the buffers, the launches, the waits.  gsr_debug_frame_plan is
// the test door (tests/test_frame_plan.py drives every rule on the CPU through the flat layouts at the end of this file).
#pragma once
#include <algorithm>
#include <cstdint>
#include "gsr_mailbox.h"
#include "gsr_policy.h"

// what the slot's last frame left for its next one (frame_finish writes them, frame_begin reads them)
struct GsrSlotHints {
    uint32_t surv_hint = 0;            // surviving clusters of this slot's last frame (sizes K1's grid; 0 = unknown)
    uint32_t kept_hint = 0;            // splats that reached the depth sort in this slot's last frame (picks the sort; 0 = unknown)
    uint32_t kept_lo = 0, kept_hi = 0; // ... and the smallest / largest of their keys, as float bits of the distance^2 (0, 0 = unknown)
    bool kept_culled = false;          // ... in a frame that was occlusion-culled (an unculled one keeps ten times as much: no prediction across)
    uint32_t slab_kept = 0;            // splats phase 1 sent to the depth sort
    uint32_t slab_kept1 = 0, slab_kept2 = 0;   // ... in this slot's LAST front-slab frame, per phase (0 = none yet): which sort a phase takes
};

// (the kernels' launch constants the grids are counted in; gsr_api.hip static_asserts them against k_preprocess.h / k_binning.h /
//  gsr_device.h / k_cluster.h)
enum : uint32_t { GSR_PLAN_K1_THREADS = 256, GSR_PLAN_BN_THREADS = 256, GSR_PLAN_BK_BUCKETS = 1024, GSR_PLAN_CLUSTER = 64 };

static inline uint32_t gsr_plan_div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---- frame_begin's inputs: X(type, name) lists, so that the struct and the test door's flat layout cannot disagree ----
#define GSR_PLAN_IN_FIELDS(X)                                                                                                      \
    X(int, phase_in)          /* 0 = a frame; 2 = the second phase of a front-slab frame */                                     \
    X(bool, allow_cull)       /* false: the re-render of a frame (frame_check / the slab re-entry) */                           \
    X(bool, out_is_device)                                                                                                      \
    X(bool, has_depth)        /* a depth-tested frame */                                                                        \
    X(uint32_t, n)            /* splats resident */                                                                             \
    X(uint32_t, nclus)        /* their clusters */                                                                              \
    X(int, sh_order)                                                                                                            \
    X(uint32_t, key_min) X(uint32_t, key_max)                                                                                   \
    X(int, opt_deferred) X(int, opt_lazy) X(int, opt_cull) X(int, opt_slab) X(int, opt_cluster) X(int, opt_sort_cache)          \
    X(int, opt_local_sort) X(int, opt_k1_scatter) X(int, opt_scatter_direct) X(int, opt_mid_sort) X(int, opt_bn_items)           \
    X(bool, full_keys)        /* GSR_FLAG_FULL_KEYS */                                                                          \
    X(int, shard_count)                                                                                                         \
    X(bool, timing) X(bool, timing_all) X(int, opt_timing)                                                                      \
    X(bool, lazy_pays) X(bool, prefix_cheaper) X(bool, prefix_valid) X(bool, bbox_ok)                                           \
    X(bool, horizon_match)    /* the slot's horizons exist and belong to this frame's tiles and geometry */                     \
    X(int, hpyr_re)           /* the dilation radius built into them */                                                         \
    X(bool, sort_match)       /* the slot's cached order exists and its SortKey is this frame's */                              \
    X(bool, sorted_culled) X(bool, sorted_dculled)                                                                              \
    X(bool, pos_match)        /* the position-keyed order exists for this geometry, camera position and key range */            \
    X(bool, same_pos)         /* the camera stands where the last frame's stood */                                              \
    X(bool, jumped)           /* (the test door's answer to "did the camera jump"; the driver asks camera_jumped) */

#define GSR_PLAN_OUT_FIELDS(X)                                                                                                     \
    X(bool, deferred)         /* handed over before its pair count is looked at */                                              \
    X(bool, lazy)             /* K1 leaves the SH colours pending */                                                            \
    X(bool, cull)             /* culled against the slot's depth horizons */                                                    \
    X(bool, jumped)           /* ... it would have been, but the camera jumped (policy mode only) */                            \
    X(int, cull_dilate)                                                                                                         \
    X(int, phase)             /* 0, or the front-slab phase 1 / 2 */                                                            \
    X(bool, timing) X(bool, timing_all)                                                                                         \
    X(bool, dcull)            /* depth-tested frame with depth culling */                                                       \
    X(bool, cache_hit)        /* a static redraw: the cached order is the frame's */                                            \
    X(bool, want_pos)         /* the position-keyed order is kept up to date for this frame ... */                              \
    X(bool, ordered)          /* ... and K1 walks it */                                                                         \
    X(int, key_bits)                                                                                                            \
    X(uint32_t, n_slots)      /* slots K1 can fill at most */                                                                   \
    X(bool, held)             /* the small-frame sort's back-off holds this slot to the global passes */                        \
    X(bool, local)            /* small-frame sort over the key range the slot's last frame kept ... */                          \
    X(bool, local_phase)      /* ... or over a front-slab phase's range */                                                      \
    X(bool, k1_scatters)      /* its bucket pass runs inside K1 */                                                              \
    X(uint32_t, bk_lo) X(int, bk_shift)                                                                                         \
    X(bool, scatter_direct)   /* (small-frame sort outside K1: one atomic per key) */                                           \
    X(bool, mid_sort)         /* (global passes: the mid-size keys per thread) */                                               \
    X(uint32_t, k1_grid)                                                                                                        \
    X(int, bn_items) X(uint32_t, bn_blocks) X(uint32_t, bn_grid)

#define GSR_PLAN_DECLARE(t, name) t name{};
struct GsrPlanIn { GSR_PLAN_IN_FIELDS(GSR_PLAN_DECLARE) GsrSlotHints hints; };
struct GsrFramePlan { GSR_PLAN_OUT_FIELDS(GSR_PLAN_DECLARE) };
#undef GSR_PLAN_DECLARE

// The plan of one frame.  NOT pure: it is where the frame's policy events happen, in this order -- cull.tick() (a frame that could have
// been culled), slab.tick() (phase 0), local.begin_frame(), and classic_once is consumed -- so the caller passes the context's policies.
// camera_jumped() is asked only of a frame that would be culled in policy mode (it costs nine projections).
template <class JumpedFn>
GsrFramePlan gsr_plan_frame(const GsrPlanIn& in, GsrCullPolicy& cull_pol, GsrSlabPolicy& slab_pol, GsrLocalSortPolicy& local_pol,
                            bool& classic_once, JumpedFn&& camera_jumped)
{
    GsrFramePlan p;
    const GsrSlotHints& h = in.hints;
    const uint32_t n = in.n;
    p.timing = in.timing; p.timing_all = in.timing_all;
    p.deferred = in.opt_deferred && in.out_is_device && in.phase_in == 0;
    // order 0: the colour is Cd itself, nothing to defer; mode 1 follows the kernels' own verdict on the previous frames
    p.lazy = in.sh_order > 0 && (in.opt_lazy == 2 || (in.opt_lazy == 1 && in.lazy_pays));
    p.cull = in.allow_cull && in.phase_in == 0 && in.opt_cull && !p.deferred && n > 0 && in.horizon_match && !in.full_keys && in.opt_cull != 3 &&
             cull_pol.allows(in.opt_cull);
    if (p.cull && in.opt_cull == 1 && camera_jumped()) { p.cull = false; p.jumped = true; }
    if (in.allow_cull && in.phase_in == 0) cull_pol.tick();
    p.cull_dilate = std::max(cull_pol.dilate - in.hpyr_re, 0);   // (the rest of the radius is built into the slot's pyramid)
    // What K1 keeps is about what a culled frame composites: it evaluates the colours itself -- unless the frame keeps far more than its
    // tiles look at (oblique ground, silhouettes: then list prefixes + fallback), or lazy colour is forced
    if (p.cull && in.sh_order > 0 && in.opt_lazy) p.lazy = in.opt_lazy >= 2 || (in.prefix_cheaper && in.prefix_valid);

    // Front-slab frame?  A frame that cannot be culled against a previous frame's horizons is rendered in two phases where occlusion
    // culling is known to pay: the nearest splats first, then -- behind the tiles that are still open only -- the rest.  (The sort-cache
    // hit is asked BEFORE the phase is known: a static redraw is never a slab.)
    const bool hit = in.opt_sort_cache && in.sort_match && !p.cull && !in.sorted_culled && !in.sorted_dculled;
    const bool slab = in.phase_in == 0 && !p.cull && !p.deferred && n > 0 && in.opt_slab && in.opt_cull && in.opt_cluster && in.bbox_ok &&
                      !in.full_keys && in.opt_sort_cache < 2 && !hit &&
                      // (where a frame is heavy enough for two phases' worth of launches to be repaid; a slab that is weak holds ITSELF off)
                      slab_pol.allows(in.opt_slab >= 2 || in.opt_cull == 3, cull_pol);
    if (in.phase_in == 0) slab_pol.tick();
    p.phase = in.phase_in == 2 ? 2 : (slab ? 1 : 0);
    if (p.phase) {   // (a phase keeps about what it composites: K1 shades on the spot; events only around phase 1's blend kernel)
        p.lazy = false;
        p.timing = p.phase == 1 && p.timing && in.opt_timing == 1;
        p.timing_all = false;
    }
    if (p.phase == 2) p.cull_dilate = 0;   // (this frame's own tiles: nothing moves)
    p.dcull = in.has_depth && in.opt_cull != 0 && n > 0;

    // The sorted list holds just the splats visible to the frame that sorted: reused as is only for an identical frame description (a
    // static redraw) -- never by a culled frame, nor over a culled frame's order or one culled against its depth buffer, nor by a phase.
    p.cache_hit = hit && p.phase == 0;
    // Position-keyed order (GSR_OPT_SORT_CACHE = 2): while the camera POSITION stands still K1 walks the splats in the order sorted when it
    // last moved; built the second time a position is seen.  Not for sharded, deferred or full-key frames.
    p.want_pos = in.opt_sort_cache >= 2 && !p.cache_hit && n > 0 && in.shard_count == 1 && !p.deferred && !in.full_keys && p.phase == 0;
    p.ordered = p.want_pos && (in.pos_match || in.same_pos);

    // Which depth sort: a frame that keeps few splats is sorted by ONE bucket scatter + one local kernel instead of three global passes,
    // chosen from what the slot's previous frame kept (correct whatever it chooses).  Not for deferred frames (nobody could render them
    // again), and no prediction from a culled frame for an unculled one.
    p.key_bits = 1;
    while (p.key_bits < 32 && ((in.key_max - in.key_min) >> p.key_bits) != 0u) ++p.key_bits;
    p.n_slots = n ? gsr_plan_div_up(in.nclus, 4u) * (uint32_t)GSR_PLAN_K1_THREADS : 0u;
    p.held = local_pol.begin_frame(in.opt_local_sort, p.cache_hit);
    p.local = !p.cache_hit && !p.ordered && p.n_slots > 0 && p.key_bits > 9 && !in.full_keys && h.kept_hi > h.kept_lo && !p.deferred &&
              !classic_once && !p.held && h.kept_culled == p.cull && p.phase == 0 &&
              (in.opt_local_sort >= 2 || (in.opt_local_sort == 1 && h.kept_hint > 0 && h.kept_hint <= 500000u));
    // (classic_once is consumed AFTER the phase-0 choice above; phase 1 leaves it for the re-render's phase 2)
    const bool classic_now = classic_once;
    if (!p.cache_hit && p.phase != 1) classic_once = false;
    const uint32_t kept_prev = p.phase == 1 ? h.slab_kept1 : h.slab_kept2;
    p.local_phase = p.phase != 0 && p.n_slots > 0 && p.key_bits > 9 && in.opt_local_sort && !classic_now && !p.held && kept_prev > 0 &&
                    kept_prev <= 900000u;
    if (p.local) {
        // BK_BUCKETS buckets of equal width over the key range the previous frame kept, widened by a sixteenth on either side (the view
        // moves), in this frame's key domain (keys are stored relative to key_min)
        const uint64_t span = (uint64_t)h.kept_hi - h.kept_lo, margin = span / 16 + 64;
        const uint64_t lo_abs = h.kept_lo > margin ? h.kept_lo - margin : 0, hi_abs = (uint64_t)h.kept_hi + margin;
        p.bk_lo = lo_abs > in.key_min ? (uint32_t)(lo_abs - in.key_min) : 0u;
        const uint64_t width = (hi_abs > in.key_min ? hi_abs - in.key_min : 0) - p.bk_lo + 1;
        while (p.bk_shift < 31 && (width >> p.bk_shift) > (uint64_t)GSR_PLAN_BK_BUCKETS) ++p.bk_shift;
    }
    p.k1_scatters = n > 0 && in.opt_k1_scatter != 0 && (p.local || p.local_phase) && in.opt_scatter_direct >= 0;
    // one global atomic per key pays up to ~150 k keys (fps direct / aggregated: C1 16 700 / 14 400, C2 8830 / 8560, C3 4650 / 4920, C4 3800 / 3950)
    p.scatter_direct = in.opt_scatter_direct == 2 || (in.opt_scatter_direct == 1 && h.kept_hint <= 150000u);
    // (keys per thread of the global passes: by what the slot's previous frame kept, from a frame of the same kind)
    p.mid_sort = in.opt_mid_sort && h.kept_hint > 0 && h.kept_hint <= 1500000u && p.n_slots <= 4000000u && h.kept_culled == p.cull;

    if (n > 0) {
        // K1 over the survivors, four clusters per workgroup-iteration; the grid follows the slot's previous frame (+25 %), and a frame
        // that keeps more simply loops; what a phase keeps is not known beforehand: a bounded grid that loops
        const uint32_t all_iter = gsr_plan_div_up(in.nclus, 4u);
        p.k1_grid = all_iter;
        if (h.surv_hint > 0 && !p.ordered) p.k1_grid = std::min<uint32_t>(all_iter, gsr_plan_div_up(h.surv_hint, 4u) * 5u / 4u + 64u);
        if (p.phase) p.k1_grid = std::min<uint32_t>(all_iter, 8192u);
        // splats per binning thread: 4 for frames that keep millions, fewer for the small ones
        // (measured, fps with 4 / 2 / 1: C1 12 770 / 13 540 / 14 190, C2 7880 / 8270 / 8510, C3 4770 / 4900 / 4830, C4 3930 / 3950 / 3760)
        p.bn_items = in.opt_bn_items > 0 ? in.opt_bn_items : (p.phase ? 2 : (!p.local ? 4 : (h.kept_hint <= 150000u ? 1 : 2)));
        const uint32_t bn_tile = (uint32_t)GSR_PLAN_BN_THREADS * (uint32_t)p.bn_items;
        p.bn_blocks = gsr_plan_div_up(n, bn_tile);
        // the binning grids: what the slot's previous frame kept, + 25 % (they loop if the frame keeps more)
        p.bn_grid = (h.kept_hint > 0 && p.phase == 0) ? std::min<uint32_t>(p.bn_blocks, gsr_plan_div_up(h.kept_hint + h.kept_hint / 4u, bn_tile) + 64u)
                                                      : (p.phase ? std::min<uint32_t>(p.bn_blocks, 4096u) : p.bn_blocks);
    } else {
        p.bn_items = 4;
    }
    return p;
}

// ---- frame_finish: how an attempt ends, once its mailbox words carry its ticket ----
enum GsrFrameEnd : int {
    GSR_FE_DONE = 0,            // composited (or handed over, deferred): the frame end follows
    GSR_FE_PHASE_2 = 1,         // a front slab is composited: the rest of the frame follows in the same slot
    GSR_FE_SORT_GAVE_UP = 2,    // the small-frame sort gave a bucket up: nothing of the attempt is kept; frame_check re-sorts it
    GSR_FE_DEPTH_APPEARED = 3,  // a culled frame met opaque geometry its cluster pass was blind to: rendered again, pyramids in front
    GSR_FE_SLAB_OVERRUN = 4,    // phase 2 ran off a list buffer too short (it continues phase 1's target): the whole frame again
    GSR_FE_TOO_MANY_PAIRS = 5,  // an error
};
enum GsrBackEndStep : int {
    GSR_BE_KEPT = 0,             // the speculative back end fitted (or the frame has no splats)
    GSR_BE_QUEUED = 1,           // no list buffer at frame_begin: the back end is queued now
    GSR_BE_REQUEUED = 2,         // the speculative back end ran clamped: its work sums are cleared and it runs again
    GSR_BE_TRUNCATED = 3,        // ... of a deferred frame, already handed over: its lists missed their tails
};

#define GSR_OUTCOME_IN_FIELDS(X)                                                                                                   \
    X(bool, has_splats)       /* j.n > 0: the mailbox was read */                                                               \
    X(int, phase) X(bool, cull) X(bool, local_sort) X(bool, dcull) X(bool, dblind) X(bool, speculative) X(bool, deferred)       \
    X(bool, blend_guess_plain)                                                                                                  \
    X(uint32_t, key_min)                                                                                                        \
    X(uint64_t, pair_cap) X(bool, has_list_buffer)                                                                              \
    X(uint64_t, max_pairs)                                                                                                      \
    X(uint32_t, mb_pairs) X(uint32_t, mb_hints) X(uint32_t, mb_kept) X(uint32_t, mb_clusters) X(uint32_t, mb_key_lo) X(uint32_t, mb_key_hi)

#define GSR_OUTCOME_OUT_FIELDS(X)                                                                                                  \
    X(int, end)               /* GsrFrameEnd */                                                                                 \
    X(int, back_end)          /* GsrBackEndStep */                                                                              \
    X(bool, grow)             /* the list buffer is grown   (before anything is queued again) */                                \
    X(bool, guard_miss)       /* the guarded plain blend kernel found covered pixels: the depth-tested one draws the frame */   \
    X(int, local_result)      /* GsrLocalSortPolicy::on_sort_result: -1 none, 0 held, 1 gave a bucket up */                     \
    X(int, depth_active)      /* the context's depth_active: -1 unchanged, else the new value */                                \
    X(bool, verdicts)         /* the kernels' verdicts on the frame before apply (mb_hints: lazy / order / cull pay, prefix) */  \
    X(bool, kept_counts)      /* an ordinary frame: GsrCullPolicy::on_kept(cull, mb_kept) */                                    \
    X(bool, slab_done)        /* phase 2: GsrSlabPolicy::on_frame_done(hints.kept_hint) */

#define GSR_PLAN_DECLARE(t, name) t name{};
struct GsrOutcomeIn { GSR_OUTCOME_IN_FIELDS(GSR_PLAN_DECLARE) };
struct GsrFrameOutcome { GSR_OUTCOME_OUT_FIELDS(GSR_PLAN_DECLARE) };
#undef GSR_PLAN_DECLARE

// Pure but for the slot's hints, which it rewrites for the slot's next frame.  The caller applies the rest in the order of the fields.
inline GsrFrameOutcome gsr_frame_outcome(const GsrOutcomeIn& in, GsrSlotHints& h)
{
    GsrFrameOutcome o;
    o.local_result = -1;
    o.depth_active = -1;
    if (!in.has_splats) return o;
    const bool covered = (in.mb_hints & GSR_HINT_DEPTH_COVERED) != 0u;
    if (in.local_sort && (in.mb_hints & GSR_HINT_SORT_GAVE_UP)) {
        // this attempt's order, lists and pair count mean nothing: nothing of it is kept -- not its say in the policies, not the hints
        o.end = GSR_FE_SORT_GAVE_UP;
        o.local_result = 1;
        h.kept_hint = 0; h.kept_lo = h.kept_hi = 0;
        return o;
    }
    if (in.local_sort) o.local_result = 0;
    if (in.dcull && in.dblind && in.cull && covered) {
        // Horizons speak for uncovered pixels only; the covered ones are served by the depth clause, which k_cluster_cull could not apply
        // (the pyramids were built beside it: the previous depth buffer was clear): clusters they need may be gone.  Once, when opaque
        // geometry first appears.
        o.end = GSR_FE_DEPTH_APPEARED;
        o.depth_active = 1;
        return o;
    }
    if (in.dcull) o.depth_active = covered ? 1 : 0;   // (the kernels' word on THIS frame's depth buffer)
    o.verdicts = in.phase != 2;                       // (on the frame BEFORE: a phase 1 carries them, a phase 2 has none of its own)
    if (in.phase == 0) {
        o.kept_counts = true;
        h.surv_hint = in.mb_clusters;                 // clusters that survived k_cluster_cull: sizes the next frame's K1 grid
        h.kept_hint = in.mb_kept;                     // ... and how many splats reached the depth sort: picks the next frame's sort
        h.kept_culled = in.cull;
    } else if (in.phase == 1) {
        // a front-slab frame: its two phases say nothing about what an ordinary frame keeps (no say in the policies); the next frame --
        // usually one culled against this frame's horizons -- keeps about what both phases kept, from about as many clusters
        h.slab_kept = in.mb_kept; h.slab_kept1 = std::max(in.mb_kept, 1u);
    } else {
        h.slab_kept2 = std::max(in.mb_kept, 1u);
        h.kept_hint = h.slab_kept + in.mb_kept;
        o.slab_done = true;
        h.surv_hint = std::min<uint32_t>(in.mb_clusters, std::max<uint32_t>(16384u, 2u * gsr_plan_div_up(h.kept_hint, GSR_PLAN_CLUSTER)));
        h.kept_culled = true;
    }
    if (h.kept_hint > 0 && in.phase == 0) {           // ... between which keys (stored relative to THIS frame's key_min)
        h.kept_lo = in.mb_key_lo + in.key_min;
        h.kept_hi = in.mb_key_hi + in.key_min;
    } else {
        h.kept_lo = h.kept_hi = 0;
    }
    if (in.mb_pairs == GSR_MB_TOO_MANY_PAIRS || in.mb_pairs > in.max_pairs) { o.end = GSR_FE_TOO_MANY_PAIRS; return o; }
    o.grow = in.mb_pairs > in.pair_cap || !in.has_list_buffer;
    if (o.grow && in.speculative && in.phase == 2) { o.end = GSR_FE_SLAB_OVERRUN; return o; }
    if (in.deferred) o.back_end = o.grow ? GSR_BE_TRUNCATED : GSR_BE_KEPT;
    else if (!in.speculative) o.back_end = GSR_BE_QUEUED;
    else o.back_end = o.grow ? GSR_BE_REQUEUED : GSR_BE_KEPT;
    // (a back end queued here guesses again with the context's new depth_active: it never guards a covered frame)
    o.guard_miss = o.back_end == GSR_BE_KEPT && in.blend_guess_plain && covered;
    o.end = in.phase == 1 ? GSR_FE_PHASE_2 : GSR_FE_DONE;
    return o;
}

// ---- the test door (gsr_debug_frame_plan): flat int32 layouts, one entry per field of the lists above, in their order ----
//   which = 0: in  = GSR_PLAN_IN_FIELDS, then GsrSlotHints (surv_hint, kept_hint, kept_lo, kept_hi, kept_culled, slab_kept, slab_kept1,
//              slab_kept2), then classic_once; policy = gsr_debug_policy's 16-int state (in / out);
//              out = GSR_PLAN_OUT_FIELDS, then classic_once after the frame
//   which = 1: in  = GSR_OUTCOME_IN_FIELDS, then GsrSlotHints; policy unused;
//              out = GSR_OUTCOME_OUT_FIELDS, then GsrSlotHints after the frame
#define GSR_PLAN_HINT_FIELDS(X) X(uint32_t, surv_hint) X(uint32_t, kept_hint) X(uint32_t, kept_lo) X(uint32_t, kept_hi) X(bool, kept_culled) \
    X(uint32_t, slab_kept) X(uint32_t, slab_kept1) X(uint32_t, slab_kept2)
inline int gsr_frame_plan_apply(int which, const int32_t* in, int32_t* policy, int32_t* out)
{
    int k = 0, o = 0;
#define GSR_GET(t, name) v.name = (t)(uint32_t)in[k++];
#define GSR_GET_HINT(t, name) h.name = (t)(uint32_t)in[k++];
#define GSR_PUT(t, name) out[o++] = (int32_t)r.name;
#define GSR_PUT_HINT(t, name) out[o++] = (int32_t)h.name;
    if (which == 0) {
        GsrPlanIn v;
        GSR_PLAN_IN_FIELDS(GSR_GET)
        GsrSlotHints& h = v.hints;
        GSR_PLAN_HINT_FIELDS(GSR_GET_HINT)
        bool classic_once = in[k++] != 0;
        GsrCullPolicy c; GsrSlabPolicy s; GsrLocalSortPolicy l;
        c.pays = policy[0] != 0; c.weak = policy[1] != 0; c.vis_unculled = (uint32_t)policy[2]; c.holdoff = policy[3]; c.backoff = policy[4];
        c.streak = policy[5]; c.dilate = policy[6]; c.opt_dilate = policy[7]; s.holdoff = policy[8]; l.fails = policy[9]; l.holdoff = policy[10];
        const GsrFramePlan r = gsr_plan_frame(v, c, s, l, classic_once, [&] { return v.jumped; });
        GSR_PLAN_OUT_FIELDS(GSR_PUT)
        out[o++] = classic_once;
        policy[3] = c.holdoff; policy[8] = s.holdoff; policy[9] = l.fails; policy[10] = l.holdoff;   // (what the plan's events change)
        return 0;
    }
    if (which == 1) {
        GsrOutcomeIn v;
        GSR_OUTCOME_IN_FIELDS(GSR_GET)
        GsrSlotHints h;
        GSR_PLAN_HINT_FIELDS(GSR_GET_HINT)
        const GsrFrameOutcome r = gsr_frame_outcome(v, h);
        GSR_OUTCOME_OUT_FIELDS(GSR_PUT)
        GSR_PLAN_HINT_FIELDS(GSR_PUT_HINT)
        return 0;
    }
#undef GSR_GET
#undef GSR_GET_HINT
#undef GSR_PUT
#undef GSR_PUT_HINT
    return -1;
}
