// gsr_api.hip -- host side of libgsplat_hip.so: context, HBM buffers, the
// per-frame kernel pipeline and the C ABI declared in include/gsplat_hip.h.
// (The verbs that edit the resident cloud without a re-upload are in gsr_resident_edit.h, included at the end; the kernels that
// write, edit and read the resident layout -- once per geometry change, not per frame -- in k_resident.h, k_visibility.h, k_remove.h,
// k_add.h, k_read.h and k_copy.h.  The debug read-backs and sort doors are in gsr_debug_read.h, included in front of the edits.)
// What the context, its frame slots and an edit in progress allocate is held by the handles of gsr_host_buffers.h: a member that owns
// is a handle, a raw pointer never owns, and a buffer that grows carries its capacity (DevVec; TileSet, WirePair and MortonScratch
// where several share one).  There is no free list: gsr_destroy deletes the context, and a call that fails returns.
//
// Pipeline per gsr_render (all on one HIP stream):
//   k_cluster_cull         clusters of 64 Morton-ordered splats vs clip planes / screen / band / depth horizons (k_cluster.h)
//   K1 k_preprocess        the splats of the surviving clusters -> record, key, (idx, rect)            (HBM)
//   depth sort             3 x {hist, row scan, scatter}; the FIRST pass drops culled splats,
//                          so everything downstream runs on the visible ones (count in HBM)
//   binning (k_binning.h)  counting sort of the (splat, super-tile) pairs into per-super-tile, depth-ordered lists:
//      k_bin_count         pairs per (block of depth-consecutive splats, super-tile)
//      k_scan_rows         per super-tile: exclusive scan over the blocks
//      k_bin_ranges        list ranges; pair count D -> mapped host memory
//      [stream sync: the host sizes the list buffer from D]
//      k_bin_place         every pair's (idx, rect) entry straight to its list position
//   K6 k_blend             per-tile list filtering + front-to-back compositing (VALU/LDS)
//   k_sum_work             per-tile bookkeeping -> counters -> mapped host memory
// Reference counterpart: GSplatRenderer::render + the GLSL program it drives
// (/root/reference/gsplat_plugin/src/GSplatRenderer.C:534-658).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/gsplat_hip.h"
#include "gsr_device.h"
#include "k_binning.h"
#include "k_blend.h"
#include "k_cluster.h"
#include "k_colour.h"
#include "k_preprocess.h"   // (and, through it, k_resident.h)
#ifdef GSR_HOST_TIMING
static double g_t_verdict = 0, g_acc_py = 0, g_acc_pre = 0, g_acc_launch = 0; static long g_acc_n = 0;
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#endif
#include "k_sort.h"
#include "k_wire.h"
#include "gsr_frame_plan.h"
#include "gsr_host_buffers.h"
#include "k_visibility.h"   // (last: the kernels of the frame keep their places in the code object)
#include "k_remove.h"
#include "k_add.h"
#include "k_read.h"
#include "k_copy.h"
#include "k_select.h"
#include "k_transform.h"
#include "k_grade.h"
#include "k_select_attrs.h"
#include "k_marks.h"
#include "k_measure.h"
#include "k_density.h"
#include "k_connect.h"
static_assert(RS_SRC_BLOCK == GSR_K1_THREADS, "the gathering sort pass reads K1's per-workgroup compaction: 256 slots each");
static_assert(GSR_PLAN_K1_THREADS == GSR_K1_THREADS && GSR_PLAN_BN_THREADS == BN_THREADS && GSR_PLAN_BK_BUCKETS == BK_BUCKETS &&
              GSR_PLAN_CLUSTER == GSR_CLUSTER, "gsr_frame_plan.h counts its grids in the kernels' constants");

#define GSR_VERSION_STR "gsplat_hip 0.1.0 (gfx950)"
#define GSR_MAX_SLOTS 2
#define GSR_STAGE_EVENTS 7
#define GSR_HOST_BANDS_MAX 8
#ifndef GSR_SPIN_US
#define GSR_SPIN_US 2000         // how long a host wait for a mailbox word spins before it blocks in the runtime
#endif

// what identifies a depth order: the geometry generation, the shard (a rank sorts only the splats it owns) and the camera
struct SortKey {
    uint64_t gen = 0;
    int shard_index = 0, shard_count = 1, shard_layout = 0, flags = 0;
    int band_first = 0, band_tile_rows = -1;   // an explicit band (gsr_set_row_band), -1 rows: none
    gsr_camera cam{};
    bool same(const SortKey& o) const
    {
        return gen == o.gen && shard_index == o.shard_index && shard_count == o.shard_count && shard_layout == o.shard_layout && flags == o.flags &&
               band_first == o.band_first && band_tile_rows == o.band_tile_rows &&
               std::memcmp(&cam, &o.cam, sizeof(gsr_camera)) == 0;
    }
};

// a render call's arguments: what a frame that is rendered again (frame_check, a front slab's phase 2) is rendered from
struct FrameArgs {
    gsr_camera cam{};
    const float* depth = nullptr;      // the caller's depth buffer (host or device), or NULL
    bool depth_is_device = false;
    float* out = nullptr;              // the caller's image (host or device)
    bool out_is_device = false;
    int aov = 0;                       // GSR_AOV_*: the plane rendered beside the image (0: none) ...
    float* aov_out = nullptr;          // ... into the caller's buffer, where the image lives (host or device)
    gsr_background bg{};               // gsr_render_over: what the frame is composited over (kind 0: nothing); the image is the caller's
};

// what a queued frame needs again when it is finished (or its back end re-queued)
struct FrameJob {
    FrameArgs args;
    bool open = false;
    GsrFrame f{};
    uint32_t n = 0;
    int local_tiles = 0, band_rows = 0, n_super = 0;
    size_t out_px = 0;
    float* target = nullptr;       // device buffer the blend kernel writes (pixels of `format`)
    int format = 0;                // the context's target format when the frame was begun (GSR_TARGET_*)
    const float* d_depth = nullptr;   // the depth buffer on the device (args.depth, or the slot's copy of a host buffer)
    bool timing = false, timing_all = false, use_map = false;
    bool speculative = false;      // the back end was queued before the pair count was known
    int bn_items = 4;              // splats per thread of the binning kernels (k_binning.h): 4, or fewer for a small frame
    uint32_t bn_grid = 0;          // ... and their grid (workgroups that stride over the blocks)
    uint32_t k1_grid = 0;          // K1's grid: the estimate of its workgroup-iterations (sizes the bucket scatter's grid too)
    bool local_sort = false;       // the depth sort took the small-frame form (k_sort.h) ...
    bool sort_failed = false;      // ... and gave a bucket up: the frame is rendered again with the three global passes
    bool redo = false;             // phase 2 of a front-slab frame met a list buffer that was too short: the frame is rendered again (frame_check)
    bool ranges_folded = false;    // ... and k_bin_place forms the list ranges and posts the pair count itself (no k_bin_ranges launch)
    bool deferred = false;         // ... and the frame handed over without waiting for it (GSR_OPT_DEFERRED_CHECK)
    bool lazy = false;             // K1 left the SH colours pending (k_colour.h)
    bool cull = false;             // occlusion culling: k_cluster_cull and K1 drop what lies behind the slot's depth horizons
    bool direct = false;           // the frame runs on the public stream itself
    uint32_t ticket = 0;           // stamps the frame's pair count in the host mailbox
    // front-slab frames: 0 = an ordinary frame; 1 = the front slab (splats up to the slab key), followed at frame_finish by
    // 2 = the rest, culled against the tiles phase 1 left opaque
    int phase = 0;
    // depth-tested frames: K1 (and k_cluster_cull) drop what lies behind everything the opaque pass left under the tiles it reaches
    bool dcull = false;            // ... against the slot's tile-max depth pyramid, parity dpar
    int dpar = 0;
    bool sort_fresh = false;       // this frame sorted (it did not reuse a cached order)
    bool dblind = false;           // ... and k_cluster_cull ran without the depth pyramids (they were built beside it, for K1)
    bool dstat = false;            // ... and the depth pyramid pass masked the covered depths with the tiles' status (a culled frame with a valid status)
    bool blend_guess_plain = false;   // the plain blend kernel was launched, guarded by "no pixel is covered" (queue_back_end)
    float2* aov_target = nullptr;  // depth AOV: the device plane the blend kernel writes ({zsum, cov} per band pixel); NULL = a frame without it
    GsrBgArgs bg{};                // a background (k_blend.h: k_blend_over): kind 0 = a frame without one; the image on the device
};

// A frame slot's arrays that are sized by the capacity, as a set of their own: gsr_upload_begin allocates them for a new capacity, and
// gsr_add allocates the larger set before its first write and hands it over once nothing can fail for lack of memory any more.
struct SlotSplatArrays {
    DevMem<GsrRecord> rec;
    DevMem<uint32_t> keyA, keyB;
    DevMem<uint32_t> blk_cnt;          // splats each K1 workgroup kept (their keys/payloads head the workgroup's 256 slots)
    DevMem<uint2> valA, valB;          // depth-sort payload: (splat index, packed tile rect)
    DevMem<float> zwin;                // per-splat window depth (depth-tested frames)
    DevMem<uint32_t> cseg;             // cluster culling (k_cluster.h): the ordered list of surviving clusters, as per-workgroup segments [ngroups * per]
};

// Everything one frame in flight owns: its HIP stream, the per-frame HBM arrays (the per-splat ones: SlotSplatArrays), the small
// mailboxes and the stage events.  Two slots alternate, so that frame f+1's memory-bound front end
// (k_preprocess, depth sort, binning) overlaps frame f's VALU-bound k_blend on the GPU.
struct FrameSlot : SlotSplatArrays {
    Stream own;                        // the slot's private stream
    hipStream_t stream = nullptr;      // (not owned) the stream its frame runs on: `own` with two frames in flight; with strictly
                                       // serial frames the context's PUBLIC stream itself (no hand-over events at all)
    Event ev_done;                     // end of the frame on `stream`
    Event ev_user;                     // caller's stream position at gsr_render entry
    // host-target frames: the blend launch in bands of tile rows, each band's rows copied back while the next ones composite
    Event ev_band[GSR_HOST_BANDS_MAX];
    int bands = 0;                     // bands of the frame's last blend launch (0 / 1: one launch, one copy)
    int band_row[GSR_HOST_BANDS_MAX + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Event ev_pairs;                    // the frame's pair count has reached host memory
    DevMem<uint32_t> d_n;              // splats that survived culling = items after the first sort pass
    StageBuf depth_stage;              // device copy of a host depth buffer
    DevVec<float> dpyr;                // depth-tested frames: the two tile-max pyramids of the opaque pass's depth (k_cluster.h), by frame parity:
                                       // [par][which], cap() floats each; behind them the per-tile "covered" array k_blend reads (5 planes of cap())
    DevMem<uint32_t> dactive;          // [2] by parity: "some tile's largest depth is below 1" (something can be culled)
    int dpar = 0;                      // parity of the slot's last depth-tested frame
    bool dpyr_built = false;           // the pyramids of parity `dpar` hold this frame's depth buffer (a frame that only LOOKED for covered pixels has none)
    bool sorted_dculled = false;       // the cached depth order holds a frame that was culled against its depth buffer
    // scan / sort scratch
    DevVec<uint32_t> hist;             // (ensure_counts)
    DevMem<uint32_t> totals;           // [512] per-digit totals of the current radix pass
    // pairs
    DevVec<uint2> pvA;                 // super-tile lists: (splat index, tile column/row mask) per entry; cap() + 4 (the blend kernel scans in 4-entry steps)
    TileSet tiles;                     // the super-tile ranges, the per-tile bookkeeping, the tiles lazy colour gave up: one capacity
    // front-slab frames
    DevVec<float> tbuf;                // per pixel of the band: the transmittance phase 1 left
    DevMem<float> hpyr2;               // the pyramid of "this tile is finished" phase 2 culls against (GSR_PYR_FLOATS)
    DevMem<uint32_t> slab;             // [GSR_SLAB_BINS + 8] histogram of the surviving clusters' nearest keys; then [0] the slab key, [1] clusters,
                                       // [2..5] the bucket ranges of the two phases' small-frame sorts (k_slab_pick)
    bool slab_dirty = false;           // a phase 1 filled the histogram and no phase 2 followed (its cull pass is what clears it): the
                                       // next front-slab frame clears it itself before it counts
    DevVec<int32_t> order;             // blockIdx -> tile, heaviest tiles first: written by k_tile_order at the end of a frame
                                       //   for this slot's next frame (valid while the tile geometry stays what it was)
    bool order_valid = false;
    int order_age = 0;                 // frames the table has stood (tiles alike: it is rebuilt every opt_order_keep frames only)
    int order_sig[6] = {0, 0, 0, 0, 0, 0}, order_per_xcd = 0;
    DevMem<uint32_t> st_scan;          // [512] per super-tile: deepest scan of its opaque tiles / "a tile stayed open" (k_tile_pass -> k_sum_work)
    DevMem<GsrTilePartial> partial;    // [4096] per 8x8-tile block: partial sums of the frame's counters (k_tile_pass -> k_sum_work)
    DevMem<uint32_t> sup_work;         // [2][256] per-super-tile work sums of the blend kernel, by frame parity
    int sup_par = 0;
    // Depth horizons (occlusion culling): per TILE, the distance^2 beyond which this slot's NEXT frame needs nothing -- a max
    // pyramid written by k_sum_work at the end of every frame from how deep the frame's tiles had to look.  A culled frame is
    // checked there too (did a tile look past the horizon its splats were culled against?); the verdict goes to the mapped word
    // h_end, and the host renders a frame that failed again, without culling, before it hands it over.
    DevMem<float> hpyr;                // pyramid levels 0..3 (k_cluster.h), GSR_PYR_FLOATS floats: what the slot's next frame culls against
    DevMem<float> hpyr_next;           // ... double-buffered: a frame's last kernels read the one it was culled against while they fill the other
    DevMem<float> hraw;                // per-tile horizons before dilation (k_tile_pass -> k_horizon_dilate)
    DevMem<float> hstat;               // per tile: every tile of its neighbourhood was "classic" in the frame that left the horizons (k_blend.h: GsrHorizonArgs.stat)
    bool hstat_valid = false;          // ... written by a depth-tested frame's end (as old as the horizons)
    DevMem<uint32_t> dbg_viol;         // GSR_DEBUG_VIOL in the environment: which tiles broke their promise (k_tile_pass)
    int hpyr_re = 0;                   // the dilation radius built into hpyr
    DevMem<uint32_t> ccnt;             // cluster culling: [CC_MAX_GROUPS] the segments' counts
    DevMem<uint32_t> d_counts;         // [0] slots K1 filled, [1] surviving clusters, [2] the small-frame sort gave a bucket up
    DevMem<uint32_t> bkt_key;          // small-frame sort (k_sort.h): the bucket regions, BK_BUCKETS x BK_CAP keys ...
    DevMem<uint2> bkt_val;             // ... and payloads
    DevMem<uint32_t> bkt_cnt;          // ... and the bucket counters, BK_STRIDE apart
    GsrSlotHints hints;                // what the slot's last frame kept, from how many clusters, between which keys (gsr_frame_plan.h)
    GsrLocalSortPolicy local_pol;      // back-off of the small-frame sort (gsr_policy.h): a run of > 64 equal keys defeats it EVERY frame
    PinnedMem<unsigned long long> h_end;      // pinned + mapped: ticket << 32 | violation
    // GSR_OPT_ROW_WORK: per global tile row, ticket << 32 | blend work of the row (k_blend.h: k_row_work), pinned + mapped + coherent,
    // GSR_MAX_TILES_SIDE words; allocated when the option is switched on
    PinnedMem<unsigned long long> h_rows;
    uint32_t rows_ticket = 0;          // ticket of the attempt whose frame end queued the slot's last k_row_work (0: none yet)
    int rows_tiles_y = 0;              // ... and the tile rows of its image
    bool horizon_valid = false;
    int horizon_sig[7] = {0, 0, 0, 0, 0, 0, 0};   // tile geometry + geometry generation the horizons belong to
    gsr_camera horizon_cam{};                     // ... and the camera of the frame that left them (camera_jumped)
    bool sorted_culled = false;        // the cached depth order holds a culled frame's splats only
    DevMem<unsigned long long> lazy_ctr;      // [0] low word: redo count of the frame, [1]: colours evaluated (running)
    DevMem<uint32_t> colour_evals;            // [256] colours evaluated per super-tile list (this frame; folded into lazy_ctr[1])
    bool last_lazy = false;            // the last frame of this slot left colours pending
    StageBuf fb;                       // staging for host-pointer output: pixels of the context's target format; cleared per band shape and format
    StageBuf aovb;                     // staging for a host-pointer AOV plane: two floats per band pixel; cleared per band shape
    DevVec<float> fb32;                // packed target formats and over-frames, front-slab frames: the f32 pixels phase 1 leaves for phase 2 (k_blend.h: out_format)
    StageBuf bgb;                      // device copy of a host background image: per slot, staged anew by every attempt of a frame
    // small device/host mailboxes
    DevMem<unsigned long long> counters;     // k_sum_work's layout: [1]/[2] records gathered (frame/running), [3]/[4] list entries
                                             // scanned, [5] wave-record evaluations (running)
    PinnedMem<unsigned long long> h_total;      // pinned + mapped + coherent [4]: k_bin_ranges writes (frame ticket << 32 | pair count), hints, survivors
    uint32_t ticket = 0;                        // ticket of the frame queued last in this slot
    PinnedMem<unsigned long long> h_counters;  // host copy of the frame's bookkeeping (fetched from d_frame when stats are asked for)
    DevMem<unsigned long long> d_frame;        // device: k_sum_work's per-frame summary [8]
    // depth-sort cache: the frame description whose order is in (keyA, valA)
    bool sort_valid = false;
    SortKey sort_key{};
    uint32_t key_min = 0;              // of the frame whose order is cached
    FrameJob job;                      // the frame queued in this slot (open until frame_finish)
    // last frame rendered in this slot
    int last_tiles_x = 0, last_local_ty = 0, last_supers = 0;
    uint32_t last_cc_groups = 0, last_cc_per = 0;   // the grid of the slot's last k_cluster_cull (0: none, or slots in cached order instead of clusters)
    uint32_t last_pairs = 0;
    GsrFramePlan last_plan;            // the plan of the attempt queued last in this slot (gsr_debug_last_plan)
    int super_tile = 0, stiles_x = 0, stiles_y = 0;
    uint64_t frame_id = 0;             // 1-based id of that frame, 0 = never used
    Event ev[GSR_STAGE_EVENTS];
    bool ev_pending = false;
    bool ev_all = false;             // all seven stage events were recorded (timing level 2), not just the blend kernel's
};

// What a gsr_get_* of the resident-edit family reports of its verb: the calls, the count of the last one, and its clock (each verb's
// header names the four entries).  report(): into the caller's pointers, any of them NULL.
struct EditTally {
    int64_t calls = 0, last = 0;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    int report(int64_t* calls_out, int64_t* last_out, double* ms_out) const
    {
        if (calls_out) *calls_out = calls;
        if (last_out) *last_out = last;
        if (ms_out) for (int k = 0; k < 4; ++k) ms_out[k] = ms[k];
        return GSR_OK;
    }
};

struct gsr_context {
    int device = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;      // (not owned) the PUBLIC stream: results are ordered on it

    // geometry (SoA of 16-byte vectors), shared read-only by the frame slots
    uint32_t n = 0, cap = 0;
    bool has_sh = false;
    float origin[3] = {0, 0, 0};
    uint64_t geo_gen = 0;              // generation of the resident geometry: only ever counts up (cached orders, horizons, the wire overlay's
                                       // inverse permutation are stamped with it), so a stamp of an older cloud can never match a newer one
    bool has_geometry = false;         // a complete upload is resident (gsr_render: GSR_E_NO_GEOMETRY otherwise)
    DevMem<float4> geoA;
    DevMem<uint4> geoB;
    DevMem<uint4> col;                 // colour halves as SoA chunks (eager colour in K1)
    DevMem<uint4> colrow;              // ... and as one contiguous row per splat (lazy colour gathers by index)
    int col_chunks = 0;
    // gsr_move: the SPARE copy of the planes (at the capacity c->cap) that k_repack writes the new storage order into; the two sets are
    // then swapped by pointer.  Allocated at the first move that re-orders, kept until the geometry is freed or an add grows the
    // capacity (gsr_add: the set it leaves as the spare one is at the old capacity and is freed); the spare cluster bounds (nclus
    // entries) go whenever an upload gives the live ones up, and after every add (they are the smaller cloud's).
    DevMem<float4> geoA2;
    DevMem<uint4> geoB2, col2, colrow2;
    DevMem<float4> clusA2, clusB2;
    // spatially ordered storage (k_cluster.h): storage slot j holds the perm[j]-th splat of the upload; clusters of 64 slots
    DevMem<uint32_t> perm;             // NULL = upload order
    std::vector<int32_t> h_perm;       // host copy (debug read-backs un-permute through it), fetched on demand
    DevMem<float4> clusA, clusB;
    uint32_t nclus = 0;
    DevMem<uint32_t> prefix;           // lazy colour: per super-tile, list entries to colour next frame (k_sum_work writes it)
    DevMem<uint32_t> prefix_all;       // 256 x 0xffffffff: colour every list completely (first frame, debug read-back)
    DevMem<uint32_t> prefix_none;      // 256 x 0: colour nothing ahead of time (GSR_FLAG_LAZY_NO_PREFIX: every tile takes the fallback)
    bool prefix_valid = false;
    bool uploading = false;
    uint32_t up_total = 0, up_filled = 0;
    // bounding box of the uploaded positions (bounds the sort keys of a frame)
    bool bbox_ok = false;
    double bb_lo[3] = {0, 0, 0}, bb_hi[3] = {0, 0, 0};

    FrameSlot slot[GSR_MAX_SLOTS];
    // position-keyed order (GSR_OPT_SORT_CACHE = 2): all splats in depth order for one camera position
    DevMem<uint32_t> pos_order;
    bool pos_valid = false;
    uint64_t pos_gen = 0;
    float pos_cam[3] = {0, 0, 0}, last_cam[3] = {0, 0, 0};
    uint32_t pos_kmin = 0, pos_kmax = 0;
    bool last_cam_set = false;
    DevVec<uint32_t> blk_pre;          // exclusive prefix of K1's per-iteration counts (k_scan_counts; ensure_counts)
    int opt_order_keep = 32;           // (A/B hook, GSR_ORDER_KEEP in the environment: 0 = no tile order where the tiles are alike)
    int opt_fuse_order = 1;            // (A/B hook, GSR_FUSE_ORDER) the tile order is built in the frame-end launch instead of behind it
    int opt_mid_sort = 1;              // (A/B hook, GSR_MID_SORT) RS_ITEMS_MID keys per thread in the global sort passes of mid-size frames
    int opt_host_bands = 4;            // (A/B hook, GSR_HOST_BANDS) host-target frames: bands of tile rows whose copy-back overlaps the compositing of the next (1: off)
    Stream copy_stream;                // ... and the stream the copies run on
    int opt_k1_scatter = 1;            // (A/B hook, GSR_K1_SCATTER) the small-frame sort's bucket pass inside K1 (0: a kernel of its own behind it)
    int opt_scatter_direct = 1;        // (A/B hook, GSR_SCATTER_DIRECT in the environment) the small-frame sort's scatter: one workgroup per K1 block
    int opt_bn_items = 0;              // (A/B hook, GSR_BN_ITEMS in the environment: 1, 2 or 4 splats per binning thread; 0 = by frame size)
    int nslots = 1;                    // frames in flight (GSR_OPT_FRAMES_IN_FLIGHT): serial by default -- occlusion culling wants the
                                       // horizons of the frame just before, and two slots hand it those of the frame before that

    DevVec<int32_t> tile_map;          // blockIdx -> tile (XCD-aware order), -1 = idle block
    int map_w = 0, map_h = 0, map_si = -1, map_sc = 0, map_rpb = -1, map_first = -1, map_shift = -1, map_grid = 0;

    int shard_index = 0, shard_count = 1, shard_layout = 0;   // layout: 0 = interleaved rows, 1 = contiguous bands
    int band_first = 0, band_tile_rows = -1;   // gsr_set_row_band: the explicit band [band_first, band_first + band_tile_rows) of tile rows; -1 rows: none
    int opt_row_work = 0;              // GSR_OPT_ROW_WORK: every frame ends with k_row_work
    int target_format = GSR_TARGET_RGBA32F;   // what a pixel of every target is (gsr_set_target_format)
    int opt_swizzle = 2, opt_timing = 1, opt_sort_cache = 1, opt_super = 0, opt_flags = 0, opt_deferred = 0, opt_lazy = 1, opt_cull = 1, opt_timing_every = 1;
    int opt_cluster = 1, opt_morton = 1, opt_local_sort = 1;
    int opt_slab = 1;                  // front-slab frames (GSR_OPT_FRONT_SLAB): 0 off, 1 where occlusion culling pays but has no horizons, 2 always
    int slab_frac = 40, slab_min = 4096, slab_max = 8192;   // the slab: this many 256ths of the surviving clusters, at least / at most so many
                                       // clusters (A/B hooks: GSR_SLAB_FRAC, GSR_SLAB_MIN, GSR_SLAB_MAX)
    bool classic_once = false;         // the next frame sorts with the three global passes whatever the prediction says

    gsr_stats st{};
    uint64_t frame_no = 0;
    size_t pair_want = 0;              // largest list buffer any frame slot needed so far
    int64_t lazy_base = 0;             // lazy_colours_total at the last gsr_stats_reset
    DevMem<uint32_t> lazy_hint;        // device: would lazy colour pay? (k_sum_work -> k_bin_ranges -> mailbox -> lazy_pays)
    bool lazy_pays = false;
    GsrCullPolicy cull_pol;            // occlusion culling: pays / weak / hold-off / back-off / dilation radius (gsr_policy.h; DESIGN.md section 4's state table)
    GsrSlabPolicy slab_pol;            // front-slab frames: held off for 256 frames after one that kept more than a third of an unculled frame (B1 at 0.46 loses 9 %)
    bool prefix_cheaper = false;       // the list-prefix colour pass would evaluate fewer colours than one per kept splat
    bool depth_active = false;         // the last depth-tested frame's depth buffer held opaque geometry in front of the far plane: the next one
                                       // builds its depth pyramid in a launch of its own, IN FRONT of k_cluster_cull (which then culls against it
                                       // too); otherwise the pyramid is built beside the cluster tests, for K1 alone (no extra launch)
    bool order_pays = false;           // k_sum_work's other verdict: the tiles differ enough in work for k_tile_order to pay
    WirePair wire;                             // wireframe overlay: the z-buffer and the image staged for a host target, kept between calls
    DevMem<uint32_t> wire_inv;                 // ... and, with spatially ordered storage, upload index -> storage slot (built on first use per geometry; gsr_update scatters through it too)
    uint64_t wire_inv_gen = 0;
    // An upload in progress.  The registerUpdate()-layout arrays of ALL its entries sit in one device arena (sized at gsr_upload_begin,
    // kept between uploads: an animated sequence re-stages every cook), in upload order; gsr_upload_end orders and packs them (k_pack).
    DevVec<char> stage;                        // (ensure_stage)
    DevVec<char> stage_raw;                    // ... and the raw float arrays of ONE gsr_upload_append_raw call (quantised into the arena); exact
    MortonScratch up_sort;                     // Morton codes / upload indices, ping-pong (kept between uploads)
    DevMem<float> up_part;                     // bounding-box partials
    Event up_ev[4];
    double up_t_begin = 0.0, up_h2d_ms = 0.0, up_quant_ms = 0.0;
    // gsr_set_visibility (k_visibility.h): the rule in force, the TRUE alphas in upload order (one float per splat of capacity, valid
    // while vis_on: geoA holds +0.0f for the hidden splats), the mask of the resident cloud, and the counter slots of k_visibility.
    // (Behind everything a frame reads: the fields above lie where they lay before there was a visibility.)
    bool vis_on = false;               // volumes or a mask are in force: the hooks of upload / update / move run
    GsrVisRule vis{};
    DevMem<float> alpha0;
    DevMem<uint32_t> vis_mask;         // ceil(n / 32) words, NULL: no mask
    DevMem<unsigned long long> vis_counters;      // k_visibility's counter slots ...
    PinnedMem<unsigned long long> vis_h_counters; // ... and where they are read back: pinned host memory, like the slots' read-backs
    int64_t vis_hidden = 0;            // what the last application hid
    // gsr_remove (k_remove.h): the SECOND array of true alphas the compaction writes (swapped with alpha0 like the planes; only with a
    // visibility in force)
    DevMem<float> alpha0_2;
    // gsr_select (k_select.h) and gsr_select_attrs (k_select_attrs.h): the counter slots of either kernel, and where they are read back
    DevMem<unsigned long long> sel_counters;
    PinnedMem<unsigned long long> sel_h_counters;
    // the mask verbs (gsr_remove, gsr_read_masked, gsr_duplicate, gsr_transform, gsr_grade): the pinned words a count arrives in
    // (ensure_h_word; two words, read behind a wait of the verb's own)
    PinnedMem<uint32_t> h_word;
    // what gsr_get_removal, _add, _read, _select, _transform, _grade, _duplicate and _select_attrs report (gsr_get_add: also the
    // capacity in force, c->cap, and the adds that grew it)
    EditTally rm, add, rd, sel, xf, gr, dup, sela;
    int64_t add_grows = 0;
    EditTally marks;                   // gsr_get_marks (k_marks.h): the calls that drew, the pixels the last one wrote
    EditTally meas;                    // gsr_get_measure (k_measure.h): the calls that measured, the splats the last one measured
    PinnedMem<uint32_t> meas_h;        // ... and the pinned words its result block arrives in (allocated by the first measure)
    EditTally seld;                    // gsr_get_select_density (k_density.h): the calls that selected, the splats the last one hit
    DevVec<uint32_t> den_cnt;          // ... its count word per upload index (kept between calls; allocated by the first one)
    PinnedMem<uint32_t> den_h;         // ... and the pinned words its result block arrives in
    EditTally selc;                    // gsr_get_select_connected (k_connect.h): the calls that selected, the splats the last one hit
    DevVec<uint32_t> con_tab;          // ... its cell table and union-find: GSR_CON_TAB_ARRAYS arrays of n + 1 words (kept between calls;
                                       // allocated by the first one; the per-splat size words are den_cnt's)
    PinnedMem<uint32_t> con_h;         // ... the pinned words its result block arrives in
    Event con_ev[8];                   // ... and the events around its stages (gsr_debug_select_connected_stages)
    double con_stage_ms[6] = {0, 0, 0, 0, 0, 0};
};

static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// for the other translation units of the library (gsr_multi.cpp)
#ifdef GSR_KPROF
extern "C" int gsr_debug_kprof_blocks(unsigned int* out8192) {
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(out8192, HIP_SYMBOL(g_kprof_blk), sizeof(g_kprof_blk)) == hipSuccess ? 0 : -1;
}
extern "C" int gsr_debug_kprof(unsigned long long* out128) {
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(out128, HIP_SYMBOL(g_kprof), sizeof(g_kprof)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef SW_PROFILE
extern "C" int gsr_debug_sw_profile(unsigned long long* out8) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_sw_prof), 64);
    return 0;
}
#endif
#ifdef GSR_DEBUG_XCC
extern "C" int gsr_debug_xcc(unsigned* out4, int reset) {
    hipDeviceSynchronize();
    if (out4) hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_dbg_xcc), 16);
    if (reset) { void* p = nullptr; hipGetSymbolAddress(&p, HIP_SYMBOL(g_dbg_xcc)); hipMemset(p, 0, 16); }
    return 0;
}
#endif
#ifdef BL_PROFILE
extern "C" int gsr_debug_blend_profile(unsigned long long* out, int reset) {   // out: [BLP_MAX_WG][4][16]
    hipDeviceSynchronize();
    if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blend_prof), sizeof(unsigned long long) * BLP_MAX_WG * 4 * 16);
    if (reset) { void* p = nullptr; hipGetSymbolAddress(&p, HIP_SYMBOL(g_blend_prof)); hipMemset(p, 0, sizeof(unsigned long long) * BLP_MAX_WG * 4 * 16); }
    return 0;
}
#endif
__attribute__((visibility("hidden"))) int gsr_internal_set_error(int code, const char* text) { return set_err(code, "%s", text); }
void gsr_internal_comm_release(gsr_context* c);
bool gsr_internal_comm_set_user_stream(gsr_context* c, void* stream, void* own);
int gsr_internal_comm_sync(gsr_context* c);

extern "C" int gsr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int gsr_debug_live_handles(int64_t out4[4])
{
    if (!out4) return set_err(GSR_E_INVALID, "gsr_debug_live_handles: out4 is NULL");
    for (int k = 0; k < 4; ++k) out4[k] = g_live[k].load(std::memory_order_relaxed);
    return GSR_OK;
}

extern "C" const char* gsr_last_error(void) { return g_err; }
extern "C" const char* gsr_version(void) { return GSR_VERSION_STR; }

static int finish_open_frames(gsr_context* c);

static int sync_all(gsr_context* c)
{
    int frc = finish_open_frames(c);   // deferred frames: look at their pair counts now
    if (frc) return frc;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k)
        if (c->slot[k].own) HIP_TRY(hipStreamSynchronize(c->slot[k].own));
    if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
    return GSR_OK;
}

static bool slot_init(FrameSlot& sl)
{
    const unsigned mailbox = hipHostMallocMapped | hipHostMallocCoherent;
    const size_t tiles = (size_t)GSR_MAX_TILES_SIDE * GSR_MAX_TILES_SIDE;
    bool ok = sl.own.create(hipStreamNonBlocking) == hipSuccess;
    sl.stream = sl.own;
    ok = ok && sl.ev_done.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && sl.ev_user.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && sl.ev_pairs.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && !sl.counters.alloc_zeroed(8);
    ok = ok && !sl.d_n.alloc_zeroed(1);
    ok = ok && !sl.totals.alloc(512);
    ok = ok && !sl.lazy_ctr.alloc_zeroed(2);
    ok = ok && !sl.colour_evals.alloc_zeroed(256);
    ok = ok && !sl.hpyr.alloc(GSR_PYR_FLOATS);
    ok = ok && !sl.hpyr_next.alloc(GSR_PYR_FLOATS);
    ok = ok && !sl.hraw.alloc(tiles);
    ok = ok && !sl.hstat.alloc(tiles);
    ok = ok && !sl.hpyr2.alloc(GSR_PYR_FLOATS);
    ok = ok && !sl.slab.alloc_zeroed(GSR_SLAB_BINS + 8);
    ok = ok && !sl.ccnt.alloc(CC_MAX_GROUPS);
    ok = ok && !sl.bkt_key.alloc((size_t)BK_BUCKETS * BK_CAP);
    ok = ok && !sl.bkt_val.alloc((size_t)BK_BUCKETS * BK_CAP);
    ok = ok && !sl.bkt_cnt.alloc_zeroed((size_t)BK_BUCKETS * BK_STRIDE);
    ok = ok && !sl.d_counts.alloc_zeroed(4);
    ok = ok && !sl.h_end.alloc(1, mailbox);
    ok = ok && !sl.st_scan.alloc_zeroed(512);
    ok = ok && !sl.partial.alloc((size_t)(GSR_MAX_TILES_SIDE / 8) * (GSR_MAX_TILES_SIDE / 8));
    ok = ok && !sl.sup_work.alloc_zeroed(512);
    ok = ok && !sl.h_total.alloc(4, mailbox);
    ok = ok && !sl.h_counters.alloc(8, 0);
    ok = ok && !sl.d_frame.alloc_zeroed(8);
    for (int k = 0; k < GSR_STAGE_EVENTS && ok; ++k) ok = sl.ev[k].create(hipEventDefault) == hipSuccess;
    return ok;
}

static int alloc_splat_arrays(SlotSplatArrays& a, size_t cap)
{
    int rc = GSR_OK;
    // (+256: K1 writes what it keeps at the head of its workgroup's 256 slots)
    if ((rc = a.rec.alloc(cap)) || (rc = a.keyA.alloc(cap + 256)) || (rc = a.keyB.alloc(cap + 256)) ||
        (rc = a.valA.alloc(cap + 256)) || (rc = a.valB.alloc(cap + 256)) ||
        (rc = a.zwin.alloc(cap)) || (rc = a.blk_cnt.alloc(cap / 256 + 16)) ||
        (rc = a.cseg.alloc(cap / GSR_CLUSTER + (size_t)CC_THREADS * 64 + 16)))
        a = SlotSplatArrays{};
    return rc;
}
// (nothing of the slot is in flight; an empty set takes the slot's arrays away)
static void slot_take_splat_arrays(FrameSlot& sl, SlotSplatArrays&& a)
{
    static_cast<SlotSplatArrays&>(sl) = std::move(a);
    sl.sort_valid = false;
}

extern "C" int gsr_create(int device, gsr_context** out)
{
    if (!out) return set_err(GSR_E_INVALID, "gsr_create: out is NULL");
    *out = nullptr;
    int ndev = gsr_device_count();
    if (ndev <= 0) return set_err(GSR_E_NO_DEVICE, "gsr_create: no HIP device visible");
    if (device < 0 || device >= ndev) return set_err(GSR_E_NO_DEVICE, "gsr_create: device %d out of range (0..%d)", device, ndev - 1);
    HIP_TRY(hipSetDevice(device));
    gsr_context* c = new (std::nothrow) gsr_context();
    if (!c) return set_err(GSR_E_OOM, "gsr_create: host allocation failed");
    c->device = device;
    if (const char* e = std::getenv("GSR_ORDER_KEEP")) c->opt_order_keep = std::atoi(e);   // (A/B hook)
    if (const char* e = std::getenv("GSR_SCATTER_DIRECT")) c->opt_scatter_direct = std::atoi(e);   // (A/B hook: -1 the general scatter, 0 never direct, 1 direct by frame size, 2 always direct)
    if (const char* e = std::getenv("GSR_K1_SCATTER")) c->opt_k1_scatter = std::atoi(e);   // (A/B hook)
    if (const char* e = std::getenv("GSR_HOST_BANDS")) c->opt_host_bands = std::min(std::max(std::atoi(e), 1), GSR_HOST_BANDS_MAX);   // (A/B hook)
    if (const char* e = std::getenv("GSR_MID_SORT")) c->opt_mid_sort = std::atoi(e);       // (A/B hook)
    if (const char* e = std::getenv("GSR_FUSE_ORDER")) c->opt_fuse_order = std::atoi(e);   // (A/B hook)
    if (const char* e = std::getenv("GSR_SLAB_FRAC")) { const int v = std::atoi(e); if (v >= 1 && v <= 255) c->slab_frac = v; }   // (A/B hook)
    if (const char* e = std::getenv("GSR_SLAB_MIN")) { const int v = std::atoi(e); if (v >= 1) c->slab_min = v; }                 // (A/B hook)
    if (const char* e = std::getenv("GSR_SLAB_MAX")) { const int v = std::atoi(e); if (v >= 1) c->slab_max = v; }                 // (A/B hook)
    if (const char* e = std::getenv("GSR_BN_ITEMS")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4) c->opt_bn_items = v; }   // (A/B hook)
    hipError_t e = c->own_stream.create(hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return set_err(GSR_E_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    c->stream = c->own_stream;
    bool ok = true;
    for (int k = 0; k < GSR_MAX_SLOTS && ok; ++k) ok = slot_init(c->slot[k]);
    if (!ok) {
        gsr_destroy(c);
        return set_err(GSR_E_HIP, "gsr_create: allocating frame slots (streams/events/mailboxes) failed");
    }
    if (c->prefix.alloc(256) || c->prefix_all.alloc(256) || c->prefix_none.alloc(256) ||
        hipMemset(c->prefix, 0xff, 256 * 4) != hipSuccess || hipMemset(c->prefix_all, 0xff, 256 * 4) != hipSuccess ||
        hipMemset(c->prefix_none, 0, 256 * 4) != hipSuccess || c->lazy_hint.alloc_zeroed(1)) {
        gsr_destroy(c);
        return set_err(GSR_E_HIP, "gsr_create: allocating the colour-prefix tables failed");
    }
    c->st.record_bytes = (int32_t)sizeof(GsrRecord);
    c->st.pair_bytes = 8;
    *out = c;
    return GSR_OK;
}

// the mask belongs to a cloud: gone with it (a visibility that was a mask alone is then no visibility)
static void vis_drop_mask(gsr_context* c)
{
    c->vis_mask.reset();
    if (c->vis.n_volumes == 0) { c->vis_on = false; c->vis_hidden = 0; }
}

// the storage order and the cluster bounds, live and spare: gone whenever the arrays are filled in upload order again
static void drop_order(gsr_context* c)
{
    c->perm.reset(); c->clusA.reset(); c->clusB.reset(); c->clusA2.reset(); c->clusB2.reset();
    c->nclus = 0; c->h_perm.clear();
}
// the spare planes of the edits (gsr_resident_edit.h: ensure_spare_planes)
static void free_spare_planes(gsr_context* c) { c->geoA2.reset(); c->geoB2.reset(); c->col2.reset(); c->colrow2.reset(); }

static void free_geometry(gsr_context* c)
{
    c->geoA.reset(); c->geoB.reset(); c->col.reset(); c->colrow.reset();
    drop_order(c);
    free_spare_planes(c);
    c->alpha0.reset();                 // (sized by the capacity; the volumes stay in force, the next complete upload captures again)
    c->alpha0_2.reset();
    vis_drop_mask(c);
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) slot_take_splat_arrays(c->slot[k], SlotSplatArrays{});
    c->cap = 0; c->n = 0;
}

// (the handles of the context and its slots release on the device that is current)
extern "C" void gsr_destroy(gsr_context* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    gsr_internal_comm_release(c);
    delete c;
}

extern "C" int gsr_set_stream(gsr_context* c, void* s)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_stream: ctx is NULL");
    // a context with a communicator (gsr_comm_init, world > 1) keeps its kernels on a stream of its own; results are ordered on `s`
    if (gsr_internal_comm_set_user_stream(c, s, c->own_stream)) return GSR_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) c->slot[k].stream = c->slot[k].own;   // (re-bound by the next frame)
    return GSR_OK;
}

extern "C" int gsr_set_option(gsr_context* c, int option, int value)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_option: ctx is NULL");
    switch (option) {
    case GSR_OPT_XCD_SWIZZLE: c->opt_swizzle = value < 0 ? 0 : (value > 3 ? 3 : value); break;
    case GSR_OPT_STAGE_TIMING: c->opt_timing = value < 0 ? 0 : (value > 2 ? 2 : value); break;
    case GSR_OPT_SORT_CACHE:
        if (value < 0 || value > 2) return set_err(GSR_E_INVALID, "gsr_set_option: sort cache is 0, 1 or 2");
        c->opt_sort_cache = value;
        c->pos_valid = false;
        for (int k = 0; k < GSR_MAX_SLOTS; ++k) c->slot[k].sort_valid = false;
        break;
    case GSR_OPT_DEBUG_FLAGS: c->opt_flags = value; break;
    case GSR_OPT_DEFERRED_CHECK: c->opt_deferred = value ? 1 : 0; break;
    case GSR_OPT_TIMING_EVERY: c->opt_timing_every = value < 1 ? 1 : (value > 1024 ? 1024 : value); break;
    case GSR_OPT_OCCLUSION_CULL: c->opt_cull = value < 0 ? 0 : (value > 3 ? 3 : value); break;
    case GSR_OPT_LAZY_COLOUR: c->opt_lazy = value < 0 ? 0 : (value > 2 ? 2 : value); break;
    case GSR_OPT_SHARD_LAYOUT: c->shard_layout = value ? 1 : 0; break;   // (2, gsr_multi's balanced bands: bands, to a context)
    case GSR_OPT_ROW_WORK: {
        if (value) {   // the rows' mailboxes, once
            HIP_TRY(hipSetDevice(c->device));
            for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
                FrameSlot& sl = c->slot[k];
                int rc = GSR_OK;
                if (!sl.h_rows && (rc = sl.h_rows.alloc(GSR_MAX_TILES_SIDE, hipHostMallocMapped | hipHostMallocCoherent))) return rc;
            }
        }
        c->opt_row_work = value ? 1 : 0;
        break;
    }
    case GSR_OPT_CLUSTER_CULL: c->opt_cluster = value ? 1 : 0; break;
    case GSR_OPT_LOCAL_SORT: c->opt_local_sort = value < 0 ? 0 : (value > 2 ? 2 : value); break;
    case GSR_OPT_FRONT_SLAB: c->opt_slab = value < 0 ? 0 : (value > 2 ? 2 : value); break;
    case GSR_OPT_CULL_DILATE: c->cull_pol.set_dilate_option(value); break;
    case GSR_OPT_STORAGE_ORDER: c->opt_morton = value ? 1 : 0; break;   // (takes effect at the next upload)
    case GSR_OPT_SUPER_TILE:
        if (value != 0 && (value < 1 || value > 16 || (value & (value - 1))))
            return set_err(GSR_E_INVALID, "gsr_set_option: super-tile edge must be 0 (auto) or 1,2,4,8,16");
        c->opt_super = value;
        break;
    case GSR_OPT_FRAMES_IN_FLIGHT: {
        if (value < 1 || value > GSR_MAX_SLOTS)
            return set_err(GSR_E_INVALID, "gsr_set_option: frames in flight must be 1..%d", GSR_MAX_SLOTS);
        HIP_TRY(hipSetDevice(c->device));
        int rc = sync_all(c);
        if (rc) return rc;
        c->nslots = value;
        break;
    }
    default: return set_err(GSR_E_INVALID, "gsr_set_option: unknown option %d", option);
    }
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// target format: what a pixel of every target (frames, band images, the wire overlay) is.  Not an option: it changes pixels.
extern "C" int gsr_target_pixel_bytes(int format)
{
    const int b = gsr_format_pixel_bytes(format);
    return b ? b : set_err(GSR_E_INVALID, "gsr_target_pixel_bytes: unknown target format %d", format);
}

extern "C" int gsr_set_target_format(gsr_context* c, int format)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_target_format: ctx is NULL");
    if (!gsr_format_pixel_bytes(format)) return set_err(GSR_E_INVALID, "gsr_set_target_format: unknown target format %d", format);
    if (format == c->target_format) return GSR_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);    // (finishes what is in flight -- a front-slab frame included -- in the format it was begun in)
    if (rc) return rc;
    rc = gsr_internal_comm_sync(c);
    if (rc) return rc;
    for (FrameSlot& sl : c->slot) { sl.fb.release(); sl.fb32.reset(); }   // the staging images are laid out for the old pixel size
    c->target_format = format;
    return GSR_OK;
}

extern "C" int gsr_get_target_format(gsr_context* c)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_target_format: ctx is NULL");
    return c->target_format;
}

// the same conversion on the host, through the same functions as the kernels' stores (gsr_device.h): for callers who keep f32 frames,
// and the yardstick the GPU path is held to.  No context, no GPU.
extern "C" int gsr_convert_pixels(const float* rgba32f, int64_t n_pixels, int format, void* out)
{
    if (!gsr_format_pixel_bytes(format)) return set_err(GSR_E_INVALID, "gsr_convert_pixels: unknown target format %d", format);
    if (n_pixels < 0 || (n_pixels > 0 && (!rgba32f || !out))) return set_err(GSR_E_INVALID, "gsr_convert_pixels: bad argument");
    if (format == GSR_TARGET_RGBA32F) { std::memcpy(out, rgba32f, (size_t)n_pixels * 16); return GSR_OK; }
    for (int64_t i = 0; i < n_pixels; ++i) {
        const float* p = rgba32f + 4 * i;
        if (format == GSR_TARGET_RGBA16F) {
            const uint2 v = gsr_pack_rgba16f(p[0], p[1], p[2], p[3]);
            std::memcpy(static_cast<char*>(out) + 8 * i, &v, 8);
        } else {
            const uint32_t v = gsr_pack_rgba8(p[0], p[1], p[2], p[3]);
            std::memcpy(static_cast<char*>(out) + 4 * i, &v, 4);
        }
    }
    return GSR_OK;
}

static inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }
// the arena's arrays for `total` splats (256-byte aligned sections)
struct UpArena {
    float *P, *alpha;
    uint16_t *Cd, *scale, *orient, *shx, *shy, *shz;
    size_t bytes;
};
static UpArena up_arena(char* base, size_t total, bool has_sh)
{
    UpArena a{};
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += pad256(bytes); return p; };
    a.P = reinterpret_cast<float*>(take(total * 12)); a.alpha = reinterpret_cast<float*>(take(total * 4));
    a.Cd = reinterpret_cast<uint16_t*>(take(total * 6)); a.scale = reinterpret_cast<uint16_t*>(take(total * 6));
    a.orient = reinterpret_cast<uint16_t*>(take(total * 8));
    if (has_sh) {
        a.shx = reinterpret_cast<uint16_t*>(take(total * 32)); a.shy = reinterpret_cast<uint16_t*>(take(total * 32));
        a.shz = reinterpret_cast<uint16_t*>(take(total * 32));
    }
    a.bytes = off;
    return a;
}
static double up_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The arena holds `bytes` (kept between uploads and edits; only ever grown, to 256 bytes beyond the need; what it held does not survive it).
static int ensure_stage(gsr_context* c, size_t bytes) { return bytes <= c->stage.cap() ? GSR_OK : c->stage.ensure(bytes + 256); }
// The first `count` events of the upload / edit clock.  oom_code: hipErrorOutOfMemory comes back as GSR_E_OOM (upload, update, remove)
// or, like every other failure, as GSR_E_HIP (move, add): the verbs differ there, and each keeps its code.
static int ensure_up_events(gsr_context* c, int count, const char* who, bool oom_code)
{
    for (int k = 0; k < count; ++k) {
        if (c->up_ev[k]) continue;
        const hipError_t e = c->up_ev[k].create(hipEventDefault);
        if (e != hipSuccess) return set_err(oom_code && e == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "%s: no event: %s", who, hipGetErrorString(e));
    }
    return GSR_OK;
}
// n rows of host arrays (rows: HOST pointers here) into the arena behind its first `at` rows, on `us`; complete on return, so the caller's
// arrays may be freed.  Host -> device, nothing else.  (Pageable memory: the runtime stages it through its own pinned buffers at the
// link's rate -- 56 GB/s measured on this box, the same as from pinned memory: tools/ubench_h2d.hip.)
static hipError_t stage_host_rows(const UpArena& A, size_t at, uint32_t n, const GsrPackSrc& rows, bool has_sh, hipStream_t us)
{
    hipError_t e = hipSuccess;
    auto h2d = [&](void* d, const void* h, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, us); };
    h2d(A.P + 3 * at, rows.P, (size_t)n * 12); h2d(A.alpha + at, rows.alpha, (size_t)n * 4); h2d(A.Cd + 3 * at, rows.Cd, (size_t)n * 6);
    h2d(A.scale + 3 * at, rows.scale, (size_t)n * 6); h2d(A.orient + 4 * at, rows.orient, (size_t)n * 8);
    if (has_sh) { h2d(A.shx + 16 * at, rows.shx, (size_t)n * 32); h2d(A.shy + 16 * at, rows.shy, (size_t)n * 32); h2d(A.shz + 16 * at, rows.shz, (size_t)n * 32); }
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    return e;
}
// One launch for a kernel template's two <SH> forms: launch(std::true_type / std::false_type).  (A kernel template takes its place in
// the code object where it is first used: the launches of k_pack, k_update, k_repack and k_update_f32 stay in this file, in that order.)
template <class Launch>
static void launch_sh(bool has_sh, Launch&& launch)
{
    if (has_sh) launch(std::true_type{});
    else launch(std::false_type{});
}

// ---------------------------------------------------------------------------
// geometry staging
extern "C" int gsr_upload_begin(gsr_context* c, int64_t total, int has_sh, const float origin[3])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_upload_begin: ctx is NULL");
    if (total < 0 || total > 0x7fffffffll) return set_err(GSR_E_INVALID, "gsr_upload_begin: bad splat count %lld", (long long)total);
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    const uint32_t n = (uint32_t)total;
    const int chunks = has_sh ? 6 : 1;
    if (n > c->cap || chunks != c->col_chunks) {
        free_geometry(c);
        const size_t cap = n ? n : 1;
        if ((rc = c->geoA.alloc(cap)) || (rc = c->geoB.alloc(cap)) || (rc = c->col.alloc(cap * chunks)) ||
            (has_sh && (rc = c->colrow.alloc(cap * 8)))) {
            free_geometry(c);
            return rc;
        }
        for (int k = 0; k < GSR_MAX_SLOTS; ++k)
            if ((rc = alloc_splat_arrays(c->slot[k], cap))) {      // (free_geometry left the slot's set empty, and no order cached)
                free_geometry(c);
                return rc;
            }
        c->cap = (uint32_t)cap;
        c->col_chunks = chunks;
    }
    // the staging arena of the whole upload (kept between uploads; only ever grown)
    if ((rc = ensure_stage(c, up_arena(nullptr, n, has_sh != 0).bytes))) return rc;
    c->up_t_begin = up_now_ms(); c->up_h2d_ms = 0.0; c->up_quant_ms = 0.0;
    c->n = 0;
    c->has_sh = has_sh != 0;
    c->up_total = n;
    c->up_filled = 0;
    c->uploading = true;
    for (int k = 0; k < 3; ++k) c->origin[k] = origin ? origin[k] : 0.0f;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) c->slot[k].sort_valid = false;
    drop_order(c);                     // (the arrays are filled in upload order again)
    return GSR_OK;
}

extern "C" int gsr_upload_append(gsr_context* c, int64_t n64, const float* P, const uint16_t* Cd, const float* alpha,
                                 const uint16_t* scale, const uint16_t* orient, const uint16_t* shx,
                                 const uint16_t* shy, const uint16_t* shz)
{
    if (!c || !c->uploading) return set_err(GSR_E_INVALID, "gsr_upload_append: no upload in progress");
    if (n64 < 0 || (uint64_t)n64 + c->up_filled > c->up_total)
        return set_err(GSR_E_INVALID, "gsr_upload_append: %lld splats exceed the %u announced", (long long)n64, c->up_total);
    if (n64 == 0) return GSR_OK;
    if (!P || !Cd || !alpha || !scale || !orient) return set_err(GSR_E_INVALID, "gsr_upload_append: NULL attribute array");
    if (c->has_sh && (!shx || !shy || !shz)) return set_err(GSR_E_INVALID, "gsr_upload_append: SH announced but arrays are NULL");
    HIP_TRY(hipSetDevice(c->device));
    const double t0 = up_now_ms();
    const uint32_t n = (uint32_t)n64;
    const size_t at = c->up_filled;
    hipStream_t us = c->slot[0].own;
    const UpArena A = up_arena(c->stage, c->up_total, c->has_sh);
    // The entry lands behind the ones before it, in upload order.  (Ordering, packing and the cluster bounds happen once, over the whole
    // upload, in gsr_upload_end.)
    const hipError_t e = stage_host_rows(A, at, n, GsrPackSrc{P, alpha, Cd, scale, orient, shx, shy, shz}, c->has_sh, us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_upload_append: %s", hipGetErrorString(e));
    c->up_filled += n;
    c->up_h2d_ms += up_now_ms() - t0;
    return GSR_OK;
}

static int order_and_pack(gsr_context* c);
// visibility (the verb and its hooks are at the end of the file)
static int vis_after_upload(gsr_context* c);
static hipError_t vis_apply(gsr_context* c, hipStream_t us, uint32_t cap_first, uint32_t cap_cnt, bool apply, const GsrVisRule& rule,
                            const uint32_t* mask, bool* changed);

// an upload that failed after the arrays were filled: the context goes back to "nothing uploaded"
static void drop_geometry(gsr_context* c)
{
    c->n = 0; c->up_total = c->up_filled = 0; c->st.n_splats = 0;
    drop_order(c);
    vis_drop_mask(c);
    c->has_geometry = false;           // gsr_render: GSR_E_NO_GEOMETRY (the generation is NOT rewound: stamps of the lost cloud stay stale)
    c->geo_gen++;
    c->wire_inv.reset(); c->wire_inv_gen = 0;
    c->pos_valid = false; c->prefix_valid = false;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
        FrameSlot& sl = c->slot[k];
        sl.sort_valid = false; sl.horizon_valid = false; sl.order_valid = false;
        sl.hints.surv_hint = 0; sl.hints.kept_hint = 0; sl.hints.kept_lo = sl.hints.kept_hi = 0;
    }
}
// gsr_multi_remove: ranks that disagree keep nothing
__attribute__((visibility("hidden"))) void gsr_internal_drop_geometry(gsr_context* c) { if (c) drop_geometry(c); }

extern "C" int gsr_upload_append_raw(gsr_context* c, int64_t n64, const gsr_raw_attrs* a)
{
    if (!c || !c->uploading) return set_err(GSR_E_INVALID, "gsr_upload_append_raw: no upload in progress");
    if (!a) return set_err(GSR_E_INVALID, "gsr_upload_append_raw: attrs is NULL");
    if (n64 < 0 || (uint64_t)n64 + c->up_filled > c->up_total)
        return set_err(GSR_E_INVALID, "gsr_upload_append_raw: %lld splats exceed the %u announced", (long long)n64, c->up_total);
    if (n64 == 0) return GSR_OK;
    if (!a->P) return set_err(GSR_E_INVALID, "gsr_upload_append_raw: P is NULL");
    if (a->sh_scheme < 0 || a->sh_scheme > 3 || (a->sh_scheme == 1 && (!a->sh_array || a->sh_vec3_per_point < 1)) || (a->sh_scheme >= 2 && !a->sh_ptr))
        return set_err(GSR_E_INVALID, "gsr_upload_append_raw: bad spherical-harmonics description");
    if (c->has_sh != (a->sh_scheme != 0)) return set_err(GSR_E_INVALID, "gsr_upload_append_raw: SH presence differs from gsr_upload_begin");
    HIP_TRY(hipSetDevice(c->device));
    const double t0 = up_now_ms();
    const uint32_t n = (uint32_t)n64;
    const size_t at = c->up_filled;
    hipStream_t us = c->slot[0].own;
    const UpArena A = up_arena(c->stage, c->up_total, c->has_sh);
    // the raw float arrays of THIS entry: their own scratch (kept between calls), quantised into the arena behind the entries before it
    const int nsh = a->sh_scheme == 2 ? 15 : (a->sh_scheme == 3 ? 45 : 0);
    int sh_live = 0;                 // schemes 2 / 3: the arrays before the first gap
    if (nsh) while (sh_live < nsh && a->sh_ptr[sh_live]) ++sh_live;
    const size_t rC = a->Cd ? pad256((size_t)n * 12) : 0, rS = a->scale ? pad256((size_t)n * 12) : 0, rO = a->orient ? pad256((size_t)n * 16) : 0;
    const size_t rArr = a->sh_scheme == 1 ? pad256((size_t)n * std::min(a->sh_vec3_per_point, 16) * 12) : 0;
    const size_t rEach = a->sh_scheme == 2 ? pad256((size_t)n * 12) : (a->sh_scheme == 3 ? pad256((size_t)n * 4) : 0);
    const size_t need = rC + rS + rO + rArr + rEach * sh_live + 256;
    int rc = GSR_OK;
    if ((rc = c->stage_raw.ensure_drained(us, need))) return rc;
    char* base = c->stage_raw;
    auto take = [&](size_t bytes) { char* p = base; base += bytes; return p; };
    hipError_t e = hipSuccess;
    auto h2d = [&](void* d, const void* h, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, us); };
    h2d(A.P + 3 * at, a->P, (size_t)n * 12);
    std::vector<float> ones;
    if (a->alpha) h2d(A.alpha + at, a->alpha, (size_t)n * 4);
    else { ones.assign(n, 1.0f); h2d(A.alpha + at, ones.data(), (size_t)n * 4); }     // missing opacity: opaque
    const float *rCd = nullptr, *rSc = nullptr, *rOr = nullptr;
    if (a->Cd) { float* p = reinterpret_cast<float*>(take(rC)); h2d(p, a->Cd, (size_t)n * 12); rCd = p; }
    if (a->scale) { float* p = reinterpret_cast<float*>(take(rS)); h2d(p, a->scale, (size_t)n * 12); rSc = p; }
    if (a->orient) { float* p = reinterpret_cast<float*>(take(rO)); h2d(p, a->orient, (size_t)n * 16); rOr = p; }
    GsrRawSh sh{};
    sh.scheme = a->sh_scheme;
    sh.vec3_per_point = a->sh_vec3_per_point > 16 ? 16 : a->sh_vec3_per_point;
    if (a->sh_scheme == 1) {
        // (only the first 16 vec3 of a longer array are used: copy them compactly)
        float* p = reinterpret_cast<float*>(take(rArr));
        if (a->sh_vec3_per_point <= 16) h2d(p, a->sh_array, (size_t)n * a->sh_vec3_per_point * 12);
        else if (e == hipSuccess)
            e = hipMemcpy2DAsync(p, (size_t)16 * 12, a->sh_array, (size_t)a->sh_vec3_per_point * 12, (size_t)16 * 12, n, hipMemcpyHostToDevice, us);
        sh.array = p;
    } else {
        for (int j = 0; j < sh_live; ++j) { float* p = reinterpret_cast<float*>(take(rEach)); h2d(p, a->sh_ptr[j], a->sh_scheme == 2 ? (size_t)n * 12 : (size_t)n * 4); sh.ptr[j] = p; }
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_quantize_raw, dim3(div_up(n, 256)), dim3(256), 0, us, n, rCd, rSc, rOr, sh, A.Cd + 3 * at, A.scale + 3 * at, A.orient + 4 * at,
                           c->has_sh ? A.shx + 16 * at : (uint16_t*)nullptr, c->has_sh ? A.shy + 16 * at : (uint16_t*)nullptr, c->has_sh ? A.shz + 16 * at : (uint16_t*)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(us);   // the caller's arrays may be freed on return
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_upload_append_raw: %s", hipGetErrorString(e));
    c->up_filled += n;
    c->up_h2d_ms += up_now_ms() - t0;
    return GSR_OK;
}

// What the frames of a cloud learned about it -- prefixes, the tile order's verdict, policies, hints, horizons -- goes: behind a new
// cloud, and behind an edit that changes the shape of the resident one (after_update).  e: the state of the call so far -- the device
// word is reset (on `us`, and waited for) only behind a success, and the first failure is what comes back.
static hipError_t forget_frame_learning(gsr_context* c, hipStream_t us, hipError_t e)
{
    c->prefix_valid = false;           // lazy colour: the first frame of a new cloud colours every list completely
    c->order_pays = false;
    c->cull_pol.on_upload(); c->slab_pol.on_upload();
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
        GsrSlotHints& h = c->slot[k].hints;
        h.surv_hint = 0; h.kept_hint = 0; h.kept_lo = h.kept_hi = 0; h.slab_kept1 = h.slab_kept2 = 0;
        c->slot[k].horizon_valid = false; c->slot[k].local_pol.on_upload();
    }
    c->lazy_pays = false;              // ... and in automatic mode the first frames are eager until the kernels say it pays
    // (the kernels' verdicts on the last frame of the PREVIOUS cloud must not reach the first frame of this one through the device word)
    if (e == hipSuccess && c->lazy_hint) e = hipMemsetAsync(c->lazy_hint, 0, 4, us);
    if (e == hipSuccess && c->lazy_hint) e = hipStreamSynchronize(us);
    return e;
}
// A new cloud is resident (the end of an upload, or of a move: the same splats at other positions are a new cloud to everything a
// frame keeps): a new generation, and nothing the frames of the cloud before learned survives.
static int new_cloud_state(gsr_context* c, const char* who)
{
    c->geo_gen++;
    c->has_geometry = true;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) c->slot[k].sort_valid = false;
    if (forget_frame_learning(c, c->slot[0].own, hipSuccess) != hipSuccess) return set_err(GSR_E_HIP, "%s: could not reset the policy word", who);
    return GSR_OK;
}

extern "C" int gsr_upload_end(gsr_context* c)
{
    if (!c || !c->uploading) return set_err(GSR_E_INVALID, "gsr_upload_end: no upload in progress");
    c->uploading = false;
    if (c->up_filled != c->up_total)
        return set_err(GSR_E_INVALID, "gsr_upload_end: %u of %u announced splats were appended", c->up_filled, c->up_total);
    c->n = c->up_total;
    c->bbox_ok = false;
    if (c->n > 0) {
        HIP_TRY(hipSetDevice(c->device));
        int rc = order_and_pack(c);
        if (rc) {
            // nothing half-made may stay renderable: no geometry, no cached order, no horizons, no hints (a later gsr_render says
            // GSR_E_NO_GEOMETRY until a complete upload has succeeded)
            drop_geometry(c);
            return rc;
        }
    }
    int rc = new_cloud_state(c, "upload");
    if (rc) return rc;
    if ((rc = vis_after_upload(c))) { drop_geometry(c); return rc; }   // (the volumes in force hide their share of the new cloud; its mask is gone)
    c->st.n_splats = c->n;
    c->st.uploads += 1;
    c->st.upload_ms[0] = c->up_h2d_ms;
    c->st.upload_ms[3] = up_now_ms() - c->up_t_begin;
    return GSR_OK;
}

extern "C" int gsr_upload_abort(gsr_context* c)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_upload_abort: ctx is NULL");
    // an upload that failed half-way leaves no geometry behind: rendering needs a complete new upload
    if (c->uploading) { c->uploading = false; c->n = 0; c->up_total = c->up_filled = 0; c->st.n_splats = 0; }
    return GSR_OK;
}

extern "C" int gsr_upload(gsr_context* c, int64_t n, const float* P, const uint16_t* Cd, const float* alpha,
                          const uint16_t* scale, const uint16_t* orient, const uint16_t* shx, const uint16_t* shy,
                          const uint16_t* shz, const float origin[3])
{
    const int has_sh = (shx && shy && shz) ? 1 : 0;
    int rc = gsr_upload_begin(c, n, has_sh, origin);
    if (rc) return rc;
    rc = gsr_upload_append(c, n, P, Cd, alpha, scale, orient, shx, shy, shz);
    if (!rc) rc = gsr_upload_end(c);
    if (rc) (void)gsr_upload_abort(c);
    return rc;
}

// ---------------------------------------------------------------------------
// multi-GPU shard helpers
extern "C" int gsr_set_row_shard(gsr_context* c, int index, int count)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_row_shard: ctx is NULL");
    if (count < 1 || index < 0 || index >= count) return set_err(GSR_E_INVALID, "gsr_set_row_shard: bad shard %d/%d", index, count);
    c->shard_index = index;
    c->shard_count = count;
    c->band_first = 0; c->band_tile_rows = -1;   // (cancels an explicit band)
    return GSR_OK;
}

bool gsr_internal_comm_has(gsr_context* c);
extern "C" int gsr_set_row_band(gsr_context* c, int first_tile_row, int tile_rows)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_row_band: ctx is NULL");
    if (first_tile_row < 0 || tile_rows < 0 || (int64_t)first_tile_row + tile_rows > GSR_MAX_DIM / GSR_TILE)
        return set_err(GSR_E_INVALID, "gsr_set_row_band: bad band [%d, %d + %d) (at most %d tile rows)", first_tile_row, first_tile_row, tile_rows, GSR_MAX_DIM / GSR_TILE);
    if (gsr_internal_comm_has(c)) return set_err(GSR_E_INVALID, "gsr_set_row_band: the context holds a communicator (gsr_comm_init sets its shard)");
    c->shard_index = 0; c->shard_count = 1;      // (cancels a row shard)
    c->band_first = first_tile_row; c->band_tile_rows = tile_rows;
    return GSR_OK;
}
// pixel rows of the context's band image of a frame `height` pixels high
static inline int ctx_band_rows(const gsr_context* c, int height)
{
    if (c->band_tile_rows >= 0) return c->band_tile_rows * GSR_TILE;
    return c->shard_count > 1 ? gsr_band_rows(height, c->shard_index, c->shard_count) : height;
}

extern "C" int gsr_band_rows(int height, int index, int count)
{
    (void)index;  // every shard uses the same (padded) band height so that gathers are uniform
    if (height <= 0 || count < 1) return 0;
    const int tiles_y = (height + GSR_TILE - 1) / GSR_TILE;
    return ((tiles_y + count - 1) / count) * GSR_TILE;
}

__attribute__((visibility("hidden"))) int gsr_internal_shard_layout(gsr_context* c) { return c ? c->shard_layout : 0; }
__attribute__((visibility("hidden"))) int gsr_internal_stitch(gsr_context* c, const float* gathered, int count, int width, int height, float* out, void* stream);
extern "C" int gsr_stitch_bands(gsr_context* c, const float* gathered, int count, int width, int height, float* out)
{
    return gsr_internal_stitch(c, gathered, count, width, height, out, c ? (void*)c->stream : nullptr);
}
// (the stream: the multi-GPU gather stitches on its transfer stream, gsr_multi.cpp)
__attribute__((visibility("hidden"))) int gsr_internal_stitch(gsr_context* c, const float* gathered, int count, int width, int height, float* out, void* stream)
{
    // (the bands were rendered with this context's shard layout: GSR_OPT_SHARD_LAYOUT)
    if (!c || !gathered || !out || count < 1 || width <= 0 || height <= 0)
        return set_err(GSR_E_INVALID, "gsr_stitch_bands: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)width * height;
    const int bpp = gsr_format_pixel_bytes(c->target_format);
    if (((uintptr_t)gathered | (uintptr_t)out) % (uintptr_t)bpp) return set_err(GSR_E_INVALID, "gsr_stitch_bands: a buffer is not aligned to the %d-byte pixel", bpp);
    const int rpb = (c->shard_layout == 1 && count > 1) ? ((height + GSR_TILE - 1) / GSR_TILE + count - 1) / count : 0;
    // (pixels of the target format move as they are: a row copy, no conversion)
#define GSR_STITCH(PIX) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stitch_bands<PIX>), dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), \
                                           reinterpret_cast<const PIX*>(gathered), count, rpb, gsr_band_rows(height, 0, count), width, height, reinterpret_cast<PIX*>(out))
    if (bpp == 16) GSR_STITCH(float4); else if (bpp == 8) GSR_STITCH(uint2); else GSR_STITCH(uint32_t);
#undef GSR_STITCH
    HIP_TRY(hipGetLastError());
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// scan + sort drivers (all on the slot's stream)
// the sort histogram and K1's prefix follow a frame's (or a cloud's) size: a quarter and 1024 words beyond the need
static int ensure_counts(DevVec<uint32_t>& v, size_t need) { return need <= v.cap() ? GSR_OK : v.ensure(need + need / 4 + 1024); }

template <typename V, int DBITS, bool GATHER, int ITEMS>
static int radix_pass(FrameSlot& sl, uint32_t* kA, V* vA, uint32_t* kB, V* vB, uint32_t n, const uint32_t* n_dev,
                      int shift, uint32_t nblk, bool contig, uint32_t* n_out = nullptr, const uint32_t* src_cnt = nullptr, uint32_t lo = 0u)
{
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radix_hist<DBITS, GATHER, false, ITEMS>), dim3(nblk), dim3(RS_THREADS), 0, sl.stream, kA, n,
                       n_dev, shift, sl.hist, nblk, contig, src_cnt, lo);
    hipLaunchKernelGGL(k_scan_rows, dim3(1u << DBITS), dim3(SC_THREADS), 0, sl.stream, sl.hist, nblk, sl.totals, n_dev, n,
                       (uint32_t)RS_THREADS * (uint32_t)ITEMS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radix_scatter<V, DBITS, GATHER, false, ITEMS>), dim3(nblk), dim3(RS_THREADS), 0, sl.stream, kA,
                       vA, kB, vB, n, n_dev, shift, sl.hist, sl.totals, nblk, contig, n_out, src_cnt, lo);
    HIP_TRY(hipGetLastError());
    return GSR_OK;
}

// stable LSD sort on key bits [0, bits); ping-pongs (kA,vA) <-> (kB,vB) and leaves the result
// in (kA,vA) by swapping the pointers.  9-bit digits are used when they save a pass.
// compact_to != NULL: the input is K1's block-compacted layout (src_cnt items at the head of every 256 slots, *src_n_dev <= n slots);
// the first pass gathers them and writes their number to *compact_to (device); the remaining passes and the caller's
// later kernels read it there.
template <typename V>
static int radix_sort(FrameSlot& sl, uint32_t*& kA, V*& vA, uint32_t*& kB, V*& vB, uint32_t n, int bits,
                      bool allow9 = true, uint32_t* compact_to = nullptr, bool contig = false, const uint32_t* src_cnt = nullptr,
                      const uint32_t* src_n_dev = nullptr /* compacting pass: the number of source SLOTS, on the device (<= n) */,
                      bool mid = false /* a frame expected to keep <= ~1.5 M keys: RS_ITEMS_MID keys per thread (shorter workgroups, more of them) */)
{
    if (n == 0) {
        if (compact_to) HIP_TRY(hipMemsetAsync(compact_to, 0, 4, sl.stream));
        return GSR_OK;
    }
    if (bits <= 0) bits = 1;
    const uint32_t nblk = div_up(n, (uint32_t)RS_THREADS * (uint32_t)(mid ? RS_ITEMS_MID : RS_ITEMS));
    int rc = ensure_counts(sl.hist, (size_t)512 * nblk + 8);
    if (rc) return rc;
    const int p8 = (bits + 7) / 8, p9 = (bits + 8) / 9;
    const bool use9 = allow9 && p9 < p8;
    const int passes = use9 ? p9 : p8, width = use9 ? 9 : 8;
    for (int p = 0; p < passes; ++p) {
        const bool skip = compact_to && p == 0;
        const uint32_t* n_dev = compact_to ? (p > 0 ? compact_to : src_n_dev) : nullptr;
#define GSR_PASS(W, I) (skip ? radix_pass<V, W, true, I>(sl, kA, vA, kB, vB, n, n_dev, p * width, nblk, contig, compact_to, src_cnt) \
                             : radix_pass<V, W, false, I>(sl, kA, vA, kB, vB, n, n_dev, p * width, nblk, contig))
        if (use9) rc = mid ? GSR_PASS(9, RS_ITEMS_MID) : GSR_PASS(9, RS_ITEMS);
        else rc = mid ? GSR_PASS(8, RS_ITEMS_MID) : GSR_PASS(8, RS_ITEMS);
#undef GSR_PASS
        if (rc) return rc;
        uint32_t* t = kA; kA = kB; kB = t;
        V* tv = vA; vA = vB; vB = tv;
    }
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// End of an upload: the splats go into MORTON ORDER of their positions (k_cluster.h) -- a stable sort of 30-bit codes, so
// equal codes keep their upload order and the storage order is a pure function of the positions -- and every 64 consecutive
// slots get their cluster bounds.  c->perm[j] = upload index of the splat in slot j (NULL: upload order kept).
static void cluster_grid(uint32_t nclus, int* rounds, uint32_t* ngroups)
{
    int r = 1;
    while ((uint64_t)CC_THREADS * (uint64_t)r * (uint64_t)CC_MAX_GROUPS < (uint64_t)nclus) ++r;
    *rounds = r;
    *ngroups = nclus ? div_up(nclus, (uint32_t)CC_THREADS * (uint32_t)r) : 0u;
}

// The ordering of a cloud, in the steps an upload and a move (gsr_move) share -- so both give the same storage order to the same
// positions.  P: every position, upload order, device memory.
// (1) the bounding box: bounds distance^2 to any camera, i.e. the sort-key range per frame -- and the Morton grid
static int position_box(gsr_context* c, const float* P, uint32_t n, hipStream_t us, const char* who)
{
    const int grid = 512;
    int rc = GSR_OK;
    if (!c->up_part && (rc = c->up_part.alloc((size_t)grid * 6))) return rc;
    hipLaunchKernelGGL(k_bbox_partials, dim3(grid), dim3(256), 0, us, P, n, c->up_part);
    std::vector<float> hp((size_t)grid * 6);
    hipError_t e = hipMemcpyAsync(hp.data(), c->up_part, hp.size() * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    bool ok = true;
    for (int k = 0; k < 3; ++k) { c->bb_lo[k] = 3.0e38; c->bb_hi[k] = -3.0e38; }
    for (int b = 0; b < grid; ++b)
        for (int k = 0; k < 3; ++k) {
            const float lo = hp[(size_t)b * 6 + k], hi = hp[(size_t)b * 6 + 3 + k];
            ok = ok && std::isfinite(lo) && std::isfinite(hi);
            c->bb_lo[k] = std::min(c->bb_lo[k], (double)lo);
            c->bb_hi[k] = std::max(c->bb_hi[k], (double)hi);
        }
    c->bbox_ok = ok;
    return GSR_OK;
}
// (2) the scratch of the sort, kept between uploads and moves: c->up_sort.hold(n) (MortonScratch, gsr_host_buffers.h)
// (3) 30-bit Morton codes in the box of (1), sorted stably with the upload index as the value: perm[j] = upload index of the splat
// in slot j (perm: n entries; the scratch of (2) is there)
static int morton_order(gsr_context* c, const float* P, uint32_t n, uint32_t* perm, const char* who)
{
    FrameSlot& sl = c->slot[0];
    float lo[3], sc[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = (float)c->bb_lo[k];
        const double ext = c->bb_hi[k] - c->bb_lo[k];
        sc[k] = ext > 0.0 ? (float)(1023.999 / ext) : 0.0f;
        if (!std::isfinite(sc[k])) sc[k] = 0.0f;
    }
    uint32_t *kA = c->up_sort.kA, *kB = c->up_sort.kB, *vA = c->up_sort.vA, *vB = c->up_sort.vB;
    hipLaunchKernelGGL(k_morton_codes, dim3(div_up(n, 256)), dim3(256), 0, sl.stream, P, n, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], kA, vA);
    int rc = radix_sort(sl, kA, vA, kB, vB, n, 30, true, (uint32_t*)nullptr, RS_XCD_DEPTH != 0);   // (leaves the result in what kA / vA name now)
    if (!rc && hipMemcpyAsync(perm, vA, (size_t)n * 4, hipMemcpyDeviceToDevice, sl.stream) != hipSuccess) rc = set_err(GSR_E_HIP, "%s: storage order", who);
    return rc;
}

static int order_and_pack(gsr_context* c)
{
    const uint32_t n = c->n;
    FrameSlot& sl = c->slot[0];
    hipStream_t us = sl.stream;
    int rc = GSR_OK;
    const UpArena A = up_arena(c->stage, c->up_total, c->has_sh);
    if ((rc = ensure_up_events(c, 4, "gsr_upload_end", true))) return rc;
    HIP_TRY(hipEventRecord(c->up_ev[0], us));
    if ((rc = position_box(c, A.P, n, us, "gsr_upload_end"))) return rc;
    // the storage order: perm[j] = upload index of the splat in slot j (NULL: upload order)
    c->perm.reset();
    if (c->opt_morton && c->bbox_ok && n > 1) {
        // without the scratch the splats simply stay in upload order (perm = NULL: ties then break by upload index, the
        // documented meaning of an unordered store) and get their clusters
        const bool have = c->up_sort.hold(n) == GSR_OK;
        if (have && !(rc = c->perm.alloc((size_t)n))) {
            rc = morton_order(c, A.P, n, c->perm, "gsr_upload_end");
            if (rc) { c->perm.reset(); return rc; }
        } else if (have) {
            (void)hipGetLastError();
            rc = GSR_OK;           // (no room for the permutation: upload order)
        }
    }
    HIP_TRY(hipEventRecord(c->up_ev[1], us));
    c->nclus = div_up(n, GSR_CLUSTER);
    c->clusA.reset(); c->clusB.reset();
    if ((rc = c->clusA.alloc(c->nclus)) || (rc = c->clusB.alloc(c->nclus))) return rc;
    const GsrPackSrc src{A.P, A.alpha, A.Cd, A.scale, A.orient, A.shx, A.shy, A.shz};
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack<decltype(sh)::value>), dim3(c->nclus), dim3(GSR_PACK_THREADS), 0, us, n, c->cap, src, c->perm, c->geoA, c->geoB, c->col, c->colrow, c->clusA, c->clusB);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_upload_end: packing the splats: %s", hipGetErrorString(e));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess) c->st.upload_ms[1] = ms;
    if (hipEventElapsedTime(&ms, c->up_ev[1], c->up_ev[2]) == hipSuccess) c->st.upload_ms[2] = ms;
    return GSR_OK;
}

// upload index -> storage slot: the inverse of the storage permutation, built once per geometry on slot 0's own stream and shared by
// the wire overlay (k_wire.h) and gsr_update.  Only an upload or a move (gsr_move) changes the permutation, and both count the generation the inverse is stamped with up.
static int ensure_inverse_perm(gsr_context* c)
{
    if (!c->perm || c->n == 0 || (c->wire_inv && c->wire_inv_gen == c->geo_gen)) return GSR_OK;
    int rc = c->wire_inv.alloc((size_t)c->n);
    if (rc) return rc;
    hipLaunchKernelGGL(k_invert_perm, dim3(div_up(c->n, 256)), dim3(256), 0, c->slot[0].own, c->perm, c->n, c->wire_inv);
    c->wire_inv_gen = c->geo_gen;
    return GSR_OK;
}

// The kernels that rewrite resident planes in place or into the spare set, behind the <SH> dispatch; the verbs that launch them are in
// gsr_resident_edit.h.  k_update / k_update_f32 on `us`: rows [first, first + n) from src, through the storage order's inverse (NULL:
// upload order)
static void launch_update(gsr_context* c, hipStream_t us, uint32_t first, uint32_t n, const GsrUpdateSrc& src, const uint32_t* inv)
{
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update<decltype(sh)::value>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, us, first, n, c->cap, src, inv, c->geoA, c->geoB, c->col, c->colrow);
    });
}
// k_repack on `us`: the n splats of the new order perm_new (NULL: upload order) from the slots old_slot names (upload index -> resident
// slot; NULL: upload order) into the spare planes, with the bounds of their clusters.  cap_dst: the capacity of the spare planes (0: the
// resident planes' own, c->cap -- everything but a gsr_duplicate that grows the context)
static hipError_t queue_repack(gsr_context* c, hipStream_t us, uint32_t n, const uint32_t* perm_new, const uint32_t* old_slot, uint32_t cap_dst = 0u)
{
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_repack<decltype(sh)::value>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, us, n, c->cap, cap_dst ? cap_dst : c->cap, perm_new, old_slot,
                           c->geoA, c->geoB, c->col, c->colrow, c->geoA2, c->geoB2, c->col2, c->colrow2, c->clusA2, c->clusB2);
    });
    return hipGetLastError();
}
static void launch_update(gsr_context* c, hipStream_t us, uint32_t first, uint32_t n, const GsrUpdateSrcF32& src, const uint32_t* inv)
{
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_f32<decltype(sh)::value>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, us, first, n, c->cap, src, inv, c->geoA, c->geoB, c->col, c->colrow);
    });
}

// the resident geometry as it is stored (tests hold gsr_update to a fresh upload with it)
extern "C" int gsr_debug_read_resident(gsr_context* c, int which, void* out, int64_t bytes)
{
    if (!c || which < 0 || which > 5) return set_err(GSR_E_INVALID, "gsr_debug_read_resident: bad argument");
    if (c->uploading || !c->has_geometry) return set_err(GSR_E_INVALID, "gsr_debug_read_resident: no geometry");
    if (which == 3 && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_debug_read_resident: a cloud without SH has no colour rows");
    const void* src = nullptr;
    size_t size = 0;
    switch (which) {
    case 0: src = c->geoA; size = (size_t)c->n * 16; break;
    case 1: src = c->geoB; size = (size_t)c->n * 16; break;
    case 2: src = c->col; size = (size_t)c->col_chunks * c->cap * 16; break;   // (chunk k starts k * cap splats in)
    case 3: src = c->colrow; size = (size_t)c->n * 128; break;
    case 4: src = c->clusA; size = (size_t)c->nclus * 16; break;
    default: src = c->clusB; size = (size_t)c->nclus * 16; break;
    }
    if (size > (size_t)0x7fffffff) return set_err(GSR_E_INVALID, "gsr_debug_read_resident: the plane is too large for this door");
    if (!out) return (int)size;
    if (bytes < (int64_t)size) return set_err(GSR_E_INVALID, "gsr_debug_read_resident: %lld bytes given, %zu needed", (long long)bytes, size);
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    if (size) HIP_TRY(hipMemcpy(out, src, size, hipMemcpyDeviceToHost));
    return (int)size;
}

// ---------------------------------------------------------------------------
static inline float M4h(const float* m, int r, int c) { return m[c * 4 + r]; }

// upper bound of the largest singular value (squared) of the 3x3 block of a GL column-major 4x4: power iteration on M^T M
// in double, padded; the Frobenius norm (always an upper bound) if the iteration misbehaves
static double sigma_max_sq(const float* m)
{
    double a[3][3], g[3][3];
    double fro = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) { a[r][k] = M4h(m, r, k); fro += a[r][k] * a[r][k]; }
    if (!(fro > 0.0) || !std::isfinite(fro)) return fro;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) g[i][k] = a[0][i] * a[0][k] + a[1][i] * a[1][k] + a[2][i] * a[2][k];
    double v[3] = {1.0, 0.7, 0.4}, lam = 0.0;
    for (int it = 0; it < 64; ++it) {
        double w[3];
        for (int i = 0; i < 3; ++i) w[i] = g[i][0] * v[0] + g[i][1] * v[1] + g[i][2] * v[2];
        const double nrm = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (!(nrm > 0.0)) return fro;
        lam = nrm / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int i = 0; i < 3; ++i) v[i] = w[i] / nrm;
    }
    // the iteration converges from below: pad generously (it only feeds a conservative cull), never above Frobenius
    const double padded = lam * 1.02 + 1e-12;
    return (std::isfinite(padded) && padded < fro) ? padded : fro;
}

// Depth-tested frames: the range of window depths the list entries' nine depth bits spread over (gsr_device.h: gsr_zq) -- that of the
// cloud's bounding box as this camera sees it.  Nothing depends on the range being right: the code clamps, and it is monotone whatever
// the constants are; a bad range only filters less.  Clouds of 2^23 splats or more have no spare index bits: no codes.
static void frame_depth_codes(const gsr_context* c, const gsr_camera* cam, GsrFrame* f)
{
    f->idx_mask = 0xffffffffu; f->zq0 = 0.0f; f->zqs = 0.0f;
    // (nor frames whose depth buffer is expected to be clear -- the plain kernel behind its guard -- where the codes would only cost)
    if (c->n >= (1u << GSR_ZQ_SHIFT) || !c->bbox_ok || !c->depth_active || (c->opt_flags & GSR_FLAG_NO_ZCODES)) return;
    double zlo = 1.0, zhi = 0.0;
    bool behind = false;
    for (int k = 0; k < 8; ++k) {
        double p[4], e[4], q[4];
        for (int a = 0; a < 3; ++a) p[a] = ((k >> a) & 1) ? c->bb_hi[a] : c->bb_lo[a];
        p[3] = 1.0;
        for (int r = 0; r < 4; ++r) e[r] = M4h(cam->obj_view, r, 0) * p[0] + M4h(cam->obj_view, r, 1) * p[1] + M4h(cam->obj_view, r, 2) * p[2] + M4h(cam->obj_view, r, 3);
        for (int r = 0; r < 4; ++r) q[r] = M4h(cam->proj, r, 0) * e[0] + M4h(cam->proj, r, 1) * e[1] + M4h(cam->proj, r, 2) * e[2] + M4h(cam->proj, r, 3) * e[3];
        if (!(q[3] > 1e-9)) { behind = true; continue; }
        const double zw = 0.5 * (q[2] / q[3]) + 0.5;
        if (std::isfinite(zw)) { zlo = std::min(zlo, zw); zhi = std::max(zhi, zw); }
    }
    if (behind) zlo = 0.0;
    zlo = std::min(std::max(zlo, 0.0), 1.0); zhi = std::min(std::max(zhi, 0.0), 1.0);
    if (!(zhi > zlo)) return;
    f->idx_mask = (1u << GSR_ZQ_SHIFT) - 1u;
    f->zq0 = (float)zlo;
    f->zqs = (float)(512.0 / (zhi - zlo));
    if (!std::isfinite(f->zqs)) { f->idx_mask = 0xffffffffu; f->zqs = 0.0f; }
}

static void build_frame(const gsr_context* c, const gsr_camera* cam, GsrFrame* f)
{
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) {
            f->ov[r * 4 + k] = M4h(cam->obj_view, r, k);
            f->vw[r * 4 + k] = M4h(cam->view, r, k);
        }
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) f->pr[r * 4 + k] = M4h(cam->proj, r, k);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            f->ob[r * 3 + k] = M4h(cam->object, r, k);
            f->io[r * 3 + k] = M4h(cam->inv_object, r, k);
        }
    for (int k = 0; k < 3; ++k) { f->cam[k] = cam->cam_pos[k]; f->origin[k] = c->origin[k]; }
    f->idx_mask = 0xffffffffu; f->zq0 = 0.0f; f->zqs = 0.0f;      // (depth-tested frames: frame_depth_codes)
    // CalcCovariance2D's per-frame constants, float32, in the contract's order
    // (/root/reference/gsplat_plugin/shaders/GSplatShaderCoreLib.h:44-53)
    volatile float p00 = M4h(cam->proj, 0, 0), p11 = M4h(cam->proj, 1, 1);
    volatile float aspect = p00 / p11;
    volatile float tanFovX = 1.0f / p00;
    volatile float p11a = p11 * aspect;
    volatile float tanFovY = 1.0f / p11a;
    f->limx = 1.3f * tanFovX;
    f->limy = 1.3f * tanFovY;
    f->sigma_vo2 = (float)(sigma_max_sq(cam->view) * sigma_max_sq(cam->object) * 1.0001);
    f->W = (float)cam->width;
    f->H = (float)cam->height;
    volatile float wp = f->W * p00;
    f->focal = wp * 0.5f;
    f->width = cam->width;
    f->height = cam->height;
    f->sh_order = (c->has_sh && cam->sh_order > 0) ? (cam->sh_order > 3 ? 3 : cam->sh_order) : 0;
    f->tiles_x = (cam->width + GSR_TILE - 1) / GSR_TILE;
    f->tiles_y = (cam->height + GSR_TILE - 1) / GSR_TILE;
    f->shard_index = c->shard_index;
    f->shard_count = c->shard_count;
    f->shard_rpb = (c->shard_layout == 1 && c->shard_count > 1) ? (f->tiles_y + c->shard_count - 1) / c->shard_count : 0;
    f->shard_first = c->shard_index * f->shard_rpb;
    if (c->band_tile_rows >= 0) {
        // an explicit band: a band layout of its own extent (an empty one owns one row beyond every image: rpb = 0 means interleaved rows)
        f->shard_rpb = c->band_tile_rows > 0 ? c->band_tile_rows : 1;
        f->shard_first = c->band_tile_rows > 0 ? c->band_first : GSR_MAX_DIM / GSR_TILE;
    }
    if (f->shard_rpb > 0) {
        const int lo = f->shard_first, hi = std::min(lo + f->shard_rpb, f->tiles_y);
        f->local_tiles_y = hi > lo ? hi - lo : 0;
    } else {
        f->local_tiles_y = (f->tiles_y > c->shard_index) ? (f->tiles_y - c->shard_index + c->shard_count - 1) / c->shard_count : 0;
    }
    // super-tile edge: smallest power of two that leaves <= 256 super-tiles (measured best at 1080p: S=8);
    // an explicit request is a lower bound -- the counting sort (k_binning.h) keeps one LDS bin per super-tile
    int shift = 0;
    if (c->opt_super > 0)
        while ((1 << shift) < c->opt_super) ++shift;
    while ((((f->tiles_x - 1) >> shift) + 1) * (((f->tiles_y - 1) >> shift) + 1) > 256) ++shift;
    // more than 256 tiles a side (> 4096 pixels): rects are packed in pairs of tiles (gsr_device.h), more than 512 (> 8192 pixels) in
    // blocks of four; a super-tile is then at least that wide (512 tiles a side cannot give <= 256 super-tiles otherwise), and its
    // edge in rect units stays <= 16: the list entries' column and row bits
    static_assert(GSR_MAX_DIM / GSR_TILE_PX == GSR_MAX_TILES_SIDE && GSR_MAX_TILES_SIDE <= 256 * 4, "tile coordinates are packed in 8 bits of rect units");
    f->rect_shift = (f->tiles_x > 512 || f->tiles_y > 512) ? 2 : ((f->tiles_x > 256 || f->tiles_y > 256) ? 1 : 0);
    if (shift < f->rect_shift) shift = f->rect_shift;
    f->super_shift = shift;
    f->flags = c->opt_flags;
    // sort-key range of this frame: distance^2 from cam_pos to the cloud's bounding box, as float bits
    f->key_min = 0u;
    f->key_max = 0xffffffffu;
    if (c->bbox_ok && !(c->opt_flags & GSR_FLAG_FULL_KEYS)) {
        double dmin2 = 0.0, dmax2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double p = cam->cam_pos[k];
            const double near_ = p < c->bb_lo[k] ? c->bb_lo[k] - p : (p > c->bb_hi[k] ? p - c->bb_hi[k] : 0.0);
            const double far_ = std::max(std::fabs(p - c->bb_lo[k]), std::fabs(p - c->bb_hi[k]));
            dmin2 += near_ * near_;
            dmax2 += far_ * far_;
        }
        const float lo = (float)(dmin2 * (1.0 - 1e-5)), hi = (float)(dmax2 * (1.0 + 1e-5));
        if (std::isfinite(lo) && std::isfinite(hi) && lo >= 0.0f && hi >= lo) {
            uint32_t blo, bhi;
            std::memcpy(&blo, &lo, 4);
            std::memcpy(&bhi, &hi, 4);
            f->key_min = blo > 2 ? blo - 2 : 0;
            f->key_max = bhi + 2;
        }
    }
    f->super = 1 << shift;
    f->stiles_x = ((f->tiles_x - 1) >> shift) + 1;
    f->stiles_y = ((f->tiles_y - 1) >> shift) + 1;
    int off = 0;
    for (int l = 0; l < GSR_PYR_LEVELS; ++l) {
        f->pyr_off[l] = off;
        off += gsr_pyr_dim(f->tiles_x, l) * gsr_pyr_dim(f->tiles_y, l);
    }
    f->cull_dilate = c->cull_pol.dilate;
    f->phase = 0;
}

// blockIdx -> tile table for the blend kernel.  Workgroup b lands on XCD b % 8; XCD x is
// handed the super-tiles x, x+8, x+16, ... (round robin for load balance), each with all of
// its owned tiles, so the 64 tiles that walk one list and gather the same records share an L2.
static int build_tile_map(gsr_context* c, const GsrFrame& f)
{
    if (c->map_w == f.width && c->map_h == f.height && c->map_si == c->shard_index && c->map_sc == c->shard_count &&
        c->map_rpb == f.shard_rpb && c->map_first == f.shard_first && c->map_shift == f.super_shift && c->tile_map)
        return GSR_OK;
    int rc = sync_all(c);   // a frame in flight may still be reading the old table
    if (rc) return rc;
    const int n_super = f.stiles_x * f.stiles_y;
    std::vector<std::vector<int32_t>> per_xcd(8);
    for (int st = 0; st < n_super; ++st) {
        std::vector<int32_t>& v = per_xcd[st & 7];
        const int sx = st % f.stiles_x, sy = st / f.stiles_x;
        for (int gty = sy << f.super_shift; gty < ((sy + 1) << f.super_shift) && gty < f.tiles_y; ++gty) {
            const GsrShard sh = gsr_frame_shard(f, 0);
            if (!gsr_shard_owns(sh, gty)) continue;
            const int lty = gsr_shard_local_row(sh, gty);
            for (int tx = sx << f.super_shift; tx < ((sx + 1) << f.super_shift) && tx < f.tiles_x; ++tx)
                v.push_back(lty * f.tiles_x + tx);
        }
    }
    size_t chunk = 0;
    for (auto& v : per_xcd) chunk = std::max(chunk, v.size());
    std::vector<int32_t> map(chunk * 8 + 8, -1);
    for (int x = 0; x < 8; ++x)
        for (size_t k = 0; k < per_xcd[x].size(); ++k) map[k * 8 + x] = per_xcd[x][k];
    if ((rc = c->tile_map.ensure(map.size()))) return rc;
    HIP_TRY(hipMemcpy(c->tile_map, map.data(), map.size() * 4, hipMemcpyHostToDevice));
    c->map_grid = (int)(chunk * 8);
    c->map_w = f.width; c->map_h = f.height; c->map_si = c->shard_index; c->map_sc = c->shard_count; c->map_rpb = f.shard_rpb; c->map_first = f.shard_first;
    c->map_shift = f.super_shift;
    return GSR_OK;
}

static void harvest_slot(gsr_context* c, FrameSlot& sl)
{
    if (!sl.ev_pending) return;
    sl.ev_pending = false;
    const Event* e = sl.ev;
    if (hipEventSynchronize(e[6]) != hipSuccess) return;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    if (!sl.ev_all) {   // only the blend kernel was bracketed
        if (hipEventElapsedTime(&ms[5], e[5], e[6]) != hipSuccess) ms[5] = 0.0f;
        c->st.ms_blend = ms[5];
        c->st.blend_ms_total += ms[5];
        c->st.blend_launches += 1;
        return;
    }
    for (int k = 0; k < 6; ++k)
        if (hipEventElapsedTime(&ms[k], e[k], e[k + 1]) != hipSuccess) ms[k] = 0.0f;
    c->st.ms_preprocess = ms[0];
    c->st.ms_depth_sort = ms[1];
    c->st.ms_emit = ms[2];
    c->st.ms_tile_sort = ms[3] + ms[4];
    c->st.ms_blend = ms[5];
    float tot = 0.0f;
    (void)hipEventElapsedTime(&tot, e[0], e[6]);
    c->st.ms_total = tot;
    c->st.blend_ms_total += ms[5];
    c->st.blend_launches += 1;
    c->st.frame_ms_total += tot;
    c->st.stage_ms_total[0] += ms[0];
    c->st.stage_ms_total[1] += ms[1];
    c->st.stage_ms_total[2] += ms[2];
    c->st.stage_ms_total[3] += ms[3] + ms[4];
    c->st.stage_ms_total[4] += ms[5];
    c->st.stage_frames += 1;
}

// ---------------------------------------------------------------------------
// A frame is QUEUED by frame_begin (everything, including a speculative back end) and COMPLETED by
// frame_finish (the one host-side wait of a frame: its pair count).  gsr_render = begin + finish; the
// multi-GPU driver begins on every GPU before it finishes on any, so the waits overlap; with
// GSR_OPT_DEFERRED_CHECK a device-target frame returns right after begin and its count is looked at later.
static inline int mark(FrameSlot& sl, int k)
{
    const FrameJob& j = sl.job;
    if (j.timing && (j.timing_all || k >= 5)) HIP_TRY(hipEventRecord(sl.ev[k], sl.stream));
    return GSR_OK;
}

// back end = placement + compositing.  The host needs the pair count D only to make sure the list buffer is
// large enough, so when a buffer exists the back end is queued SPECULATIVELY right behind the count (both
// kernels clamp to the buffer's capacity) and the host reads D while the GPU is already placing: the stream
// never drains mid-frame.  Only if D turns out to exceed the capacity (first frame, or the pair count grew by
// more than the 25 % headroom) is the buffer grown and the back end run again.
static GsrRangeArgs range_args(gsr_context* c, FrameSlot& sl)
{
    const FrameJob& j = sl.job;
    GsrRangeArgs a;
    a.totals = sl.totals; a.n_super = j.n_super; a.sstart = sl.tiles.sstart; a.send = sl.tiles.send; a.host_total = sl.h_total.dev();
    a.ticket = j.ticket; a.max_pairs = (unsigned long long)GSR_MAX_PAIRS; a.redo_count = reinterpret_cast<uint32_t*>(sl.lazy_ctr.get());
    a.lazy_hint = c->lazy_hint; a.n_sorted = sl.d_n; a.k1_counts = sl.d_counts; a.sorted_keys = sl.keyA;
    a.depth_active = j.dcull ? sl.dactive + j.dpar : (const uint32_t*)nullptr;
    return a;
}

// what the frame driver's caches are keyed by: the tile geometry of a frame (the horizons': this, and the geometry generation behind it)
static inline void tile_sig(const GsrFrame& f, int* sig /* [6] */)
{
    const int now[6] = {f.width, f.height, f.shard_rpb > 0 ? f.shard_first : f.shard_index, f.shard_count, f.shard_rpb, f.super_shift};   // (a band: where it begins, how many rows)
    std::memcpy(sig, now, sizeof now);
}

static inline int32_t list_cap(const FrameSlot& sl) { return (int32_t)std::min<size_t>(sl.pvA.cap(), (size_t)0x7fffffff); }

static GsrSumArgs sum_args(const FrameJob& j)
{
    GsrSumArgs g;
    g.n_tiles = j.local_tiles; g.tiles_x = j.f.tiles_x; g.tiles_y = j.f.tiles_y; g.shard = gsr_frame_shard(j.f, 0);
    g.super_shift = j.f.super_shift; g.stiles_x = j.f.stiles_x; g.n_super = j.n_super;
    return g;
}

// what every kernel that forms horizons needs of the frame (k_tile_pass, k_slab_mid): its lists, the positions, the camera, the pyramid's layout
static GsrHorizonArgs horizon_args(const gsr_context* c, const FrameSlot& sl)
{
    const GsrFrame& f = sl.job.f;
    GsrHorizonArgs hz{};
    hz.list_cap = list_cap(sl); hz.lists = sl.pvA; hz.geoA = c->geoA; hz.idx_mask = f.idx_mask;
    for (int l = 0; l < GSR_PYR_LEVELS; ++l) hz.pyr_off[l] = f.pyr_off[l];
    hz.cam[0] = f.cam[0]; hz.cam[1] = f.cam[1]; hz.cam[2] = f.cam[2];
    return hz;
}

// the compositing launch (+ the lazy-colour fallback behind it)
static int queue_blend(gsr_context* c, FrameSlot& sl, bool with_depth, bool guarded)
{
    const FrameJob& j = sl.job;
    const GsrFrame& f = j.f;
    hipStream_t s = sl.stream;
    if (j.local_tiles <= 0) return GSR_OK;
    if (!j.direct) HIP_TRY(hipStreamWaitEvent(s, sl.ev_user, 0));
    GsrBlendArgs a;
    a.guard = guarded ? sl.dactive + j.dpar : (const uint32_t*)nullptr; a.guard_want = 0u;
    {   // (a perspective projection -- clip w = -view z, clip z = a z + b: window depth = (1 - a) / 2 - beta / view depth)
        const bool persp = f.pr[8] == 0.0f && f.pr[9] == 0.0f && f.pr[12] == 0.0f && f.pr[13] == 0.0f && f.pr[14] == -1.0f && f.pr[15] == 0.0f;
        a.near_alpha = persp ? 0.5f * (1.0f - f.pr[10]) : 0.0f;
        a.near_scale = persp ? 1.12f : 0.0f;
    }
    a.tile_cov = (with_depth && j.dcull && !j.dblind) ? sl.dpyr + 4 * sl.dpyr.cap() : (const float*)nullptr;
    a.idx_mask = f.idx_mask; a.zq0 = f.zq0; a.zqs = f.zqs;
    a.tile_dmax = (with_depth && j.dcull && !j.dblind && f.idx_mask != 0xffffffffu) ? sl.dpyr + (size_t)(2 * j.dpar) * sl.dpyr.cap() + f.pyr_off[0] : (const float*)nullptr;
    a.width = f.width; a.height = f.height; a.tiles_x = f.tiles_x; a.local_tiles = j.local_tiles;
    a.shard = gsr_frame_shard(f, 0); a.band_rows = j.band_rows;
    a.super_shift = f.super_shift; a.rect_shift = f.rect_shift; a.stiles_x = f.stiles_x; a.use_map = j.use_map ? 1 : 0; a.flags = f.flags;
    a.list_cap = list_cap(sl);
    a.sup_work = (a.use_map && c->opt_swizzle >= 2 && sl.sup_work) ? sl.sup_work + 256 * sl.sup_par : nullptr;
    a.slab = j.phase; a.tbuf = sl.tbuf; a.tile_work_a = sl.tiles.tile_work_a;
    uint4* const tw = j.phase == 1 ? sl.tiles.tile_work_a : sl.tiles.tile_work;   // (phase 1's bookkeeping is kept for phase 2 and the frame end)
    // heaviest-first table of this slot's previous frame, if that frame had the same tiles
    int sig[6];
    tile_sig(f, sig);
    const bool ordered = a.use_map && c->opt_swizzle >= 2 && sl.order_valid && std::memcmp(sig, sl.order_sig, sizeof sig) == 0;
    const int32_t* tmap = ordered ? sl.order : c->tile_map;
    const unsigned grid = ordered ? (unsigned)(8 * sl.order_per_xcd) : a.use_map ? (unsigned)c->map_grid : (unsigned)j.local_tiles;
    GsrLazyArgs lz;
    lz.f = f; lz.colrow = c->colrow;
    lz.redo = j.lazy ? sl.tiles.redo : nullptr;
    lz.redo_count = reinterpret_cast<uint32_t*>(sl.lazy_ctr.get());
    // (a packed target: the kernel converts at its store; the f32 pointer is the slot's own buffer, which only front-slab frames use)
    // (a frame over a background is laid out like a packed one whatever its format: the composited pixel goes to the target, the raw one
    //  of a front slab's phase 1 to the slot's own buffer -- phase 2 must never continue from a composited pixel)
    const bool over = j.bg.kind != 0;
    a.out_format = j.format; a.out_packed = (j.format != GSR_TARGET_RGBA32F || over) ? (void*)j.target : nullptr;
    float4* tgt = reinterpret_cast<float4*>((j.format != GSR_TARGET_RGBA32F || over) ? sl.fb32 : j.target);
    // One launch of the blend family: every member takes the same arguments up to the lazy-colour block; the AOV kernels take the
    // plane behind them (k_blend.h: k_blend_aov), the background kernels what the frame is composited over (k_blend_over)
    auto launch = [&](auto kernel, unsigned g, const int32_t* map, uint4* work, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g), dim3(256), 0, s, a, map, sl.pvA, sl.tiles.sstart, sl.tiles.send, sl.rec, tgt, work, sl.zwin, j.d_depth, lz, tail...);
    };
    auto launch_verb = [&](auto plain, auto aov, auto bg, unsigned g, const int32_t* map, uint4* work) {
        if (j.aov_target) launch(aov, g, map, work, j.aov_target);
        else if (over) launch(bg, g, map, work, j.bg);
        else launch(plain, g, map, work);
    };
    // Host-target frames (a caller without GL interop): the frame's LAST blend launch is issued band by band of tile rows, an event
    // behind each, and queue_frame_end copies a band's rows back on a second stream as soon as its event fires: all but the first
    // band's compositing hides behind the link, which is what bounds such a frame (33 MB at ~55 GB/s = 0.6 ms per 1080p frame).
    // The launches walk the same tile table; a workgroup of another band's tile leaves at once (~3 us per extra launch).
    int nb = 1;
    if (!j.args.out_is_device && j.phase != 1 && c->opt_host_bands > 1 && c->shard_count == 1 && c->band_tile_rows < 0 && f.local_tiles_y >= 4 * c->opt_host_bands) nb = c->opt_host_bands;
    if (nb > 1 && !c->copy_stream && c->copy_stream.create(hipStreamNonBlocking) != hipSuccess) { nb = 1; (void)hipGetLastError(); }
    for (int b = 0; b < nb && nb > 1; ++b)
        if (!sl.ev_band[b] && sl.ev_band[b].create(hipEventDisableTiming) != hipSuccess) { nb = 1; (void)hipGetLastError(); }
    sl.bands = nb;
    for (int b = 0; b < nb; ++b) {
        a.row_lo = nb > 1 ? (int)((int64_t)f.local_tiles_y * b / nb) : 0;
        a.row_hi = nb > 1 ? (int)((int64_t)f.local_tiles_y * (b + 1) / nb) : 0x7fffffff;
        sl.band_row[b] = a.row_lo; sl.band_row[b + 1] = nb > 1 ? a.row_hi : f.local_tiles_y;
        if (with_depth) launch_verb(k_blend<true>, k_blend_aov<true>, k_blend_over<true>, grid, tmap, tw);
        else launch_verb(k_blend<false>, k_blend_aov<false>, k_blend_over<false>, grid, tmap, tw);
        // the tiles that met a pending colour, with on-demand evaluation (normally none: the blocks exit at once)
        if (j.lazy && with_depth) launch_verb(k_blend_lazy<true>, k_blend_aov_lazy<true>, k_blend_over_lazy<true>, (unsigned)j.local_tiles, c->tile_map, sl.tiles.tile_work);
        else if (j.lazy) launch_verb(k_blend_lazy<false>, k_blend_aov_lazy<false>, k_blend_over_lazy<false>, (unsigned)j.local_tiles, c->tile_map, sl.tiles.tile_work);
        if (nb > 1) HIP_TRY(hipEventRecord(sl.ev_band[b], s));
    }
    HIP_TRY(hipGetLastError());
    return GSR_OK;
}

static int queue_back_end(gsr_context* c, FrameSlot& sl)
{
    const FrameJob& j = sl.job;
    const GsrFrame& f = j.f;
    hipStream_t s = sl.stream;
    int rc;
    if ((rc = mark(sl, 3))) return rc;
    if (j.n > 0) {
        const uint32_t nblk = div_up(j.n, (uint32_t)BN_THREADS * (uint32_t)j.bn_items);
        const size_t lds = (size_t)4 * j.bn_items * j.n_super * (8 + 4);   // lane masks (u64) + first list position (u32) per (group of 64 splats, super-tile)
        const GsrShard shd = gsr_frame_shard(f, f.rect_shift);
        const GsrRangeArgs ra = j.ranges_folded ? range_args(c, sl) : GsrRangeArgs{};
        // (+ the extra work items of the blocks that are split by rows of super-tiles, k_binning.h; +1: the publishing workgroup)
        const uint32_t bn_extra = (uint32_t)BN_SPLIT_TILES * (uint32_t)std::max(f.stiles_y - 1, 0);
        const uint32_t grid = std::min(nblk, j.bn_grid) + bn_extra + (j.ranges_folded ? 1u : 0u);
#define GSR_PLACE(I) hipLaunchKernelGGL((f.idx_mask != 0xffffffffu ? k_bin_place<I, true> : k_bin_place<I, false>), dim3(grid), dim3(BN_THREADS), lds, s, sl.valA, sl.d_n,          \
                                        f.super_shift - f.rect_shift, shd, f.stiles_x, j.n_super, sl.hist, sl.tiles.sstart, nblk, (uint32_t)sl.pvA.cap(), sl.pvA, ra,   \
                                        f.idx_mask != 0xffffffffu ? sl.zwin : (const float*)nullptr, f.zq0, f.zqs)
        if (j.bn_items == 1) GSR_PLACE(1); else if (j.bn_items == 2) GSR_PLACE(2); else GSR_PLACE(4);
#undef GSR_PLACE
        HIP_TRY(hipGetLastError());
    }
    if ((rc = mark(sl, 4))) return rc;
    if (j.lazy && j.n > 0) {
        // colours for the front of every super-tile list: as deep as the previous frame's tiles scanned (+ headroom)
        const bool predict = c->prefix_valid && !(f.flags & GSR_FLAG_LAZY_NO_PREFIX);
        hipLaunchKernelGGL(k_colour_prefix, dim3((unsigned)(j.n_super * CL_BLOCKS_PER_LIST)), dim3(CL_THREADS), 0, s, f, sl.pvA,
                           sl.tiles.sstart, sl.tiles.send, (f.flags & GSR_FLAG_LAZY_NO_PREFIX) ? c->prefix_none : (predict ? c->prefix : c->prefix_all),
                           (int)list_cap(sl), c->colrow, sl.rec, sl.colour_evals);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = mark(sl, 5))) return rc;
    // Depth-tested frames: the plain kernel, guarded, while the slot's depth buffers have been clear (k_blend.h: GsrBlendArgs.guard);
    // not for a frame that is handed over before its mailbox is read (nobody could queue the other kernel in time)
    // (... nor over lists whose index words carry depth codes: only the depth-tested kernel masks them off)
    // (... nor for a frame with the depth AOV: a void launch would leave its plane unwritten, and the AOV kernels have no guarded form)
    // (... nor for a frame over a background: the over-kernels have no guarded form either)
    sl.job.blend_guess_plain = j.d_depth != nullptr && j.dcull && !c->depth_active && !j.deferred && j.f.idx_mask == 0xffffffffu && !j.aov_target && j.bg.kind == 0;
    if ((rc = queue_blend(c, sl, j.d_depth != nullptr && !sl.job.blend_guess_plain, sl.job.blend_guess_plain))) return rc;
    return mark(sl, 6);
}

// bookkeeping + hand-over: the frame's counters to the host mirror, host copy if asked, result ordered on the public stream
static int queue_frame_end(gsr_context* c, FrameSlot& sl)
{
    const FrameJob& j = sl.job;
    hipStream_t s = sl.stream;
    const GsrSumArgs g = sum_args(j);
    GsrHorizonArgs hz{};
    hz.list_cap = list_cap(sl);
    // (below a few hundred thousand splats in the sort the frame is bound by launch floors: nothing for culling to win)
    // ... and while culling is held off nobody needs horizons: they are prepared again two frames before it may resume.
    // A deferred frame (handed over before its pair count was known) never culls and may have clamped lists: no horizons from it.
    if (c->opt_cull && c->opt_cull != 3 && j.n > 0 && !j.deferred && (c->opt_cull >= 2 || j.cull || j.phase == 2 || (c->cull_pol.vis_unculled >= 300000u && c->cull_pol.holdoff <= 2))) {
        hz = horizon_args(c, sl);
        hz.raw = sl.hraw; hz.pyr_in = sl.hpyr; hz.pyr_out = sl.hpyr_next; hz.dilate = j.f.cull_dilate; hz.culled = j.cull ? 1 : 0;
        hz.host_end = j.cull ? sl.h_end.dev() : nullptr; hz.ticket = j.ticket;
        // (depth-tested frames leave, and culled ones check, the tiles' status: k_blend.h.  A frame without a depth buffer leaves every
        //  tile classic: the sign bits of its raw horizons are clear)
        hz.stat = sl.hstat;
        hz.stat_in_use = (j.cull && j.dcull && j.dstat) ? 1 : 0;
        hz.depth_culled = (j.dcull && !j.dblind) ? 1 : 0;
        static const bool dbgv = std::getenv("GSR_DEBUG_VIOL") != nullptr;
        if (dbgv) {
            if (!sl.dbg_viol) (void)sl.dbg_viol.alloc(80);
            if (sl.dbg_viol) (void)hipMemsetAsync(sl.dbg_viol, 0, 80 * 4, s);
            hz.dbg = sl.dbg_viol;
        }
    }
    if (j.phase == 2) { hz.slab = 2; hz.tile_work_a = sl.tiles.tile_work_a; }
    const int nblocks8 = ((j.f.tiles_x + 7) >> 3) * ((j.f.tiles_y + 7) >> 3);
    hipLaunchKernelGGL(k_tile_pass, dim3((unsigned)nblocks8), dim3(64), 0, s, sl.tiles.tile_work, g, sl.tiles.sstart, sl.tiles.send, hz, sl.partial, sl.st_scan);
    uint32_t* const prefix_arg = (j.f.sh_order > 0 && c->opt_lazy) ? c->prefix : (uint32_t*)nullptr;
    const uint32_t* const redo_arg = j.lazy ? reinterpret_cast<const uint32_t*>(sl.lazy_ctr.get()) : (const uint32_t*)nullptr;
    uint32_t* const work_next = sl.sup_work ? sl.sup_work + 256 * (sl.sup_par ^ 1) : (uint32_t*)nullptr;
    sl.horizon_valid = hz.raw != nullptr;
    sl.hstat_valid = hz.raw != nullptr;       // (the dilation writes it beside the pyramid)
    // The heaviest-first table is rebuilt every frame where the tiles differ a lot (k_sum_work's verdict); where they do not it is
    // still worth a few microseconds of k_blend's tail (C4: 0.142 -> 0.139 ms), but not the 10 us of k_tile_order every frame:
    // then a table stands for GSR_ORDER_KEEP frames of the same shape.
    int osig[6];
    tile_sig(j.f, osig);
    const bool order_due = c->opt_swizzle >= 3 || (c->opt_swizzle == 2 && c->order_pays);
    const bool order_kept = !order_due && c->opt_swizzle == 2 && c->opt_order_keep > 0 && sl.order_valid && sl.order_age < c->opt_order_keep &&
                            std::memcmp(osig, sl.order_sig, sizeof osig) == 0;
    const bool order_refresh = !order_due && !order_kept && c->opt_swizzle == 2 && c->opt_order_keep > 0 && c->n >= 1000000u;
    if (order_kept) sl.order_age += 1; else sl.order_valid = false;
    const bool order_now = j.use_map && (order_due || order_refresh) && j.local_tiles > 0 && j.n_super <= 256 && sl.sup_work;
    const int per_xcd = 2 * ((j.n_super + 15) / 16) << (2 * j.f.super_shift);
    if (order_now)
        if (const int rc = sl.order.ensure_drained(s, (size_t)8 * per_xcd)) return rc;
    // the next frame's tile order is built BESIDE the frame's sums (and the horizon dilation), in the same launch (k_blend.h: k_frame_end_order)
    const bool fused_order = order_now && c->opt_fuse_order != 0;
    if (sl.horizon_valid) sl.hpyr_re = std::min(c->cull_pol.dilate, GSR_DILATE_EXACT_MAX);
    if (fused_order) {
        const GsrOrderArgs oa{sl.tiles.tile_work, j.f.tiles_y, sl.sup_work + 256 * sl.sup_par, per_xcd, sl.order};
        const int ndil = sl.horizon_valid ? nblocks8 : 0;
        hipLaunchKernelGGL(k_frame_end_order, dim3(9u + (unsigned)((ndil + TO_THREADS / 64 - 1) / (TO_THREADS / 64))), dim3(TO_THREADS), 0, s, sl.partial, nblocks8, ndil, g, sl.counters, sl.d_n, sl.d_frame,
                           prefix_arg, redo_arg, sl.colour_evals, sl.lazy_ctr + 1, sl.tiles.sstart, sl.tiles.send, c->lazy_hint, work_next, hz, sl.st_scan, sl.hpyr_re, oa);
        HIP_TRY(hipGetLastError());
    } else if (sl.horizon_valid) {
        // the frame's sums and verdict, and BESIDE them (one launch) the next frame's pyramid: every tile's horizon widened to its
        // neighbourhood, into the slot's other pyramid buffer
        hipLaunchKernelGGL(k_frame_end, dim3((unsigned)nblocks8 + 1u), dim3(SW_THREADS), 0, s, sl.partial, nblocks8, g, sl.counters, sl.d_n, sl.d_frame,
                           prefix_arg, redo_arg, sl.colour_evals, sl.lazy_ctr + 1, sl.tiles.sstart, sl.tiles.send, c->lazy_hint, work_next, hz, sl.st_scan, sl.hpyr_re);
        HIP_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_sum_work, dim3(1), dim3(SW_THREADS), 0, s, sl.partial, nblocks8, g, sl.counters, sl.d_n, sl.d_frame,
                           prefix_arg, redo_arg, sl.colour_evals, sl.lazy_ctr + 1, sl.tiles.sstart, sl.tiles.send, c->lazy_hint, work_next, hz, sl.st_scan);
        HIP_TRY(hipGetLastError());
    }
    if (sl.horizon_valid) {
        std::swap(sl.hpyr, sl.hpyr_next);      // (what the slot's next frame culls against)
        tile_sig(j.f, sl.horizon_sig);
        sl.horizon_sig[6] = (int)c->geo_gen;
        sl.horizon_cam = j.args.cam;
    }
    if (order_now) {
        if (!fused_order) {
            hipLaunchKernelGGL(k_tile_order, dim3(8), dim3(TO_THREADS), 0, s, sl.tiles.tile_work, g, j.f.tiles_y, sl.sup_work + 256 * sl.sup_par,
                               per_xcd, sl.order);
            HIP_TRY(hipGetLastError());
        }
        std::memcpy(sl.order_sig, osig, sizeof osig);
        sl.order_per_xcd = per_xcd;
        sl.order_valid = true;
        sl.order_age = 0;
    }
    if (c->opt_row_work && sl.h_rows.dev()) {
        // the tile rows' work, into the slot's mapped words (one launch more; nothing waits for it)
        hipLaunchKernelGGL(k_row_work, dim3((unsigned)((j.f.tiles_y + RW_THREADS / 64 - 1) / (RW_THREADS / 64))), dim3(RW_THREADS), 0, s, sl.tiles.tile_work,
                           j.phase == 2 ? sl.tiles.tile_work_a : (const uint4*)nullptr, g, sl.h_rows.dev(), j.ticket);
        HIP_TRY(hipGetLastError());
        sl.rows_ticket = j.ticket; sl.rows_tiles_y = j.f.tiles_y;
    }
    sl.sup_par ^= 1;
    if (j.f.sh_order > 0 && c->opt_lazy) c->prefix_valid = j.phase == 0;   // (eager frames keep the scan depths too: the switch to lazy starts predicted;
                                                                           //  a front-slab frame's scan depths belong to two different lists)
    sl.last_lazy = j.lazy;
    if (j.timing) { sl.ev_pending = true; sl.ev_all = j.timing_all; }
    if (!j.args.out_is_device) {
        const size_t bpp = (size_t)gsr_format_pixel_bytes(j.format);
        if (sl.bands > 1 && c->copy_stream) {
            // (band by band behind the blend launches' events, on a stream of their own: k_tile_pass and the frame end run beside the copies)
            for (int b = 0; b < sl.bands; ++b) {
                const size_t r0 = std::min<size_t>((size_t)sl.band_row[b] * GSR_TILE, (size_t)j.band_rows), r1 = std::min<size_t>((size_t)sl.band_row[b + 1] * GSR_TILE, (size_t)j.band_rows);
                if (r1 <= r0) continue;
                const size_t off = r0 * (size_t)j.f.width * bpp;
                HIP_TRY(hipStreamWaitEvent(c->copy_stream, sl.ev_band[b], 0));
                HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(j.args.out) + off, sl.fb.p + off, (r1 - r0) * (size_t)j.f.width * bpp, hipMemcpyDeviceToHost, c->copy_stream));
            }
            HIP_TRY(hipStreamSynchronize(c->copy_stream));
        } else {
            HIP_TRY(hipMemcpyAsync(j.args.out, sl.fb.p, j.out_px * bpp, hipMemcpyDeviceToHost, s));
        }
        if (j.aov_target) HIP_TRY(hipMemcpyAsync(j.args.aov_out, sl.aovb.p, j.out_px * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    // results are ordered on the public stream: anything the caller queues there next sees this frame
    if (!j.direct) {
        HIP_TRY(hipEventRecord(sl.ev_done, s));
        HIP_TRY(hipStreamWaitEvent(c->stream, sl.ev_done, 0));
    }
    return GSR_OK;
}

// The middle of a front-slab frame: phase 1 is composited; which tiles are finished?  (k_blend.h: k_slab_mid, then the pyramid
// phase 2 culls against -- no dilation: same frame, same camera)
static int queue_slab_mid(gsr_context* c, FrameSlot& sl)
{
    const FrameJob& j = sl.job;
    hipStream_t s = sl.stream;
    const GsrSumArgs g = sum_args(j);
    GsrHorizonArgs hz = horizon_args(c, sl);
    hz.raw = (c->opt_cull && c->opt_cull != 3) ? sl.hraw : nullptr;          // the finished tiles' horizons for the slot's NEXT frame
    const int nblocks8 = ((j.f.tiles_x + 7) >> 3) * ((j.f.tiles_y + 7) >> 3);
    hipLaunchKernelGGL(k_slab_mid, dim3((unsigned)nblocks8), dim3(64), 0, s, sl.tiles.tile_work_a, g, sl.tiles.sstart, sl.tiles.send, hz, sl.hpyr2,
                       sl.slab + GSR_SLAB_BINS, j.f.key_min);
    HIP_TRY(hipGetLastError());
    return GSR_OK;
}

// a frame that failed half-way may have kernels queued that still write the caller's buffer: drain them first
static int frame_abort(FrameSlot& sl, int rc)
{
    sl.job.open = false;
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    return rc;
}

// A mailbox word in mapped host memory carries (frame ticket << 32 | value); the GPU writes it mid-stream while it carries on
// -- no event in the stream (an event costs the GPU ~6 us of idle queue), no API call.  The host watches the word: a bounded
// spin (the word normally arrives within tens of microseconds), then it stops burning the caller's core and blocks in
// hipStreamSynchronize -- by then the frame is a long one and the extra latency no longer matters.
static int wait_mailbox(FrameSlot& sl, volatile unsigned long long* box, uint32_t ticket, const char* what, unsigned long long* out)
{
    unsigned long long v = *box;
    if ((uint32_t)(v >> 32) != ticket) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned long spins = 1; (uint32_t)(v >> 32) != ticket; ++spins) {
            if ((spins & 0xffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(GSR_SPIN_US)) {
                const hipError_t q = hipStreamSynchronize(sl.stream);   // everything queued has run: the word must be there now
                if (q != hipSuccess) return set_err(GSR_E_HIP, "gsr_render: waiting for the %s: %s", what, hipGetErrorString(q));
                v = *box;
                if ((uint32_t)(v >> 32) != ticket) return set_err(GSR_E_HIP, "gsr_render: the frame finished without delivering its %s", what);
                break;
            }
            __builtin_ia32_pause();
            v = *box;
        }
    }
    *out = v;
    return GSR_OK;
}

// Did the camera JUMP since the frame that left the slot's depth horizons (a cut, a viewport switch, "home")?  Horizons tolerate a
// view that moves by a few tiles per frame (they are widened by the dilation radius, 16 tiles at most) and distances that change by
// a few per cent (a horizon sits a quarter of the tile's depth range behind what the tile needed).  Beyond that a culled attempt is
// wasted -- its check fails and the frame is rendered again -- so such a frame is rendered as if the slot had no horizons (a
// front-slab frame where that pays).  A heuristic on nine reference points (the corners and the centre of the cloud's bounding
// box: their direction as seen from the camera, and their distance); whatever it answers, the pixels are the same.
static bool camera_jumped(const gsr_context* c, const gsr_camera& was, const gsr_camera& now)
{
    if (!c->bbox_ok) return false;
    double diag2 = 0.0;
    for (int k = 0; k < 3; ++k) diag2 += ((double)c->bb_hi[k] - c->bb_lo[k]) * ((double)c->bb_hi[k] - c->bb_lo[k]);
    if (!(diag2 > 0.0) || !std::isfinite(diag2)) return false;
    const double near2 = diag2 / 16.0;                              // reference points closer than a quarter of the diagonal say nothing
    const double focal_px = 0.5 * std::fabs((double)now.proj[0]) * now.width;
    const double max_px = 24.0 * GSR_TILE_PX;
    for (int k = 0; k < 9; ++k) {
        double p[3], va[3], vb[3], da2 = 0.0, db2 = 0.0;
        for (int a = 0; a < 3; ++a) p[a] = k < 8 ? (((k >> a) & 1) ? c->bb_hi[a] : c->bb_lo[a]) : 0.5 * ((double)c->bb_lo[a] + c->bb_hi[a]);
        for (int r = 0; r < 3; ++r) {                               // view-space positions (GL column-major: m[c * 4 + r])
            va[r] = was.obj_view[r] * p[0] + was.obj_view[4 + r] * p[1] + was.obj_view[8 + r] * p[2] + was.obj_view[12 + r];
            vb[r] = now.obj_view[r] * p[0] + now.obj_view[4 + r] * p[1] + now.obj_view[8 + r] * p[2] + now.obj_view[12 + r];
            da2 += va[r] * va[r]; db2 += vb[r] * vb[r];
        }
        if (!(da2 > near2) || !(db2 > near2) || !std::isfinite(da2) || !std::isfinite(db2)) continue;
        const double ratio2 = db2 / da2;
        if (ratio2 > 1.25 * 1.25 || ratio2 < 0.8 * 0.8) return true;
        const double cosang = (va[0] * vb[0] + va[1] * vb[1] + va[2] * vb[2]) / std::sqrt(da2 * db2);
        const double ang = std::acos(std::min(1.0, std::max(-1.0, cosang)));
        if (ang * focal_px > max_px) return true;
    }
    return false;
}

static int frame_begin(gsr_context* c, const FrameArgs& a, FrameSlot** used, bool allow_cull, int phase_in = 0);
static int frame_finish(gsr_context* c, FrameSlot& sl);

// An attempt that is not handed over: its order is not cached, and the work sums its speculative back end added over its lists are
// cleared (k_tile_order reads them).  redo: frame_check renders the frame again, as it is.
static int abandon_attempt(FrameSlot& sl, bool redo)
{
    if (sl.sup_work) (void)hipMemsetAsync(sl.sup_work + 256 * sl.sup_par, 0, 256 * sizeof(uint32_t), sl.stream);
    sl.sort_valid = false;
    sl.job.redo = redo;
    sl.job.open = false;
    return GSR_OK;
}

// the same frame again, in the same slot: frame_begin counts it once more, so the frame counters step back first
static int render_again(gsr_context* c, const FrameArgs& a, int phase, FrameSlot** used)
{
    c->frame_no -= 1;
    c->st.frames -= 1;
    FrameSlot* sl = nullptr;
    int rc = frame_begin(c, a, &sl, false, phase);
    if (rc) return rc;
    if ((rc = frame_finish(c, *sl))) return rc;
    if (used) *used = sl;
    return GSR_OK;
}

static int frame_finish(gsr_context* c, FrameSlot& sl)
{
    if (!sl.job.open) return GSR_OK;
    FrameJob& j = sl.job;
    HIP_TRY(hipSetDevice(c->device));
    GsrMailbox mb;
    if (j.n > 0) {
        // The pair count arrives in mapped host memory, stamped with the frame's ticket, while the GPU carries on: the
        // host just watches the word -- no event in the stream (an event costs the GPU ~6 us of idle queue), no API call.
        unsigned long long v = 0;
        const int wrc = wait_mailbox(sl, sl.h_total, j.ticket, "pair count", &v);
        if (wrc) return frame_abort(sl, wrc);
        mb = GsrMailbox::read(sl.h_total);
    }
    GsrOutcomeIn in;
    in.has_splats = j.n > 0; in.phase = j.phase; in.cull = j.cull; in.local_sort = j.local_sort; in.dcull = j.dcull; in.dblind = j.dblind;
    in.speculative = j.speculative; in.deferred = j.deferred; in.blend_guess_plain = j.blend_guess_plain; in.key_min = j.f.key_min;
    in.pair_cap = sl.pvA.cap(); in.has_list_buffer = sl.pvA != nullptr; in.max_pairs = (uint64_t)GSR_MAX_PAIRS;
    in.mb_pairs = mb.pairs; in.mb_hints = mb.hints; in.mb_kept = mb.kept; in.mb_clusters = mb.clusters; in.mb_key_lo = mb.key_lo; in.mb_key_hi = mb.key_hi;
    const GsrFrameOutcome o = gsr_frame_outcome(in, sl.hints);
    const uint32_t D = mb.pairs;
    if (o.local_result >= 0) sl.local_pol.on_sort_result(o.local_result != 0);   // (back-off: GsrLocalSortPolicy::begin_frame)
    if (o.end == GSR_FE_SORT_GAVE_UP) {
        // frame_check renders it again with the three global passes; nothing of it is kept, not its bookkeeping (no frame end) either
        j.sort_failed = true;
        sl.last_pairs = 0;
        return abandon_attempt(sl, false);
    }
    if (o.end == GSR_FE_DEPTH_APPEARED) {   // (the frame again with the pyramids in front: frame_check)
        c->depth_active = true;
        c->st.frames_requeued += 1;
        return abandon_attempt(sl, true);
    }
    if (o.depth_active >= 0) {
        c->depth_active = o.depth_active != 0;
        if (j.sort_fresh) sl.sorted_dculled = c->depth_active;   // (conservatively "yes" until now)
    }
    if (o.verdicts) {   // (the kernels' verdicts on the frame BEFORE: lazy colour / occlusion culling / list prefixes / tile order pay)
        c->lazy_pays = mb.has(GSR_HINT_LAZY_PAYS);
        c->cull_pol.on_kernel_verdict(mb.has(GSR_HINT_CULL_PAYS));
        c->prefix_cheaper = mb.has(GSR_HINT_PREFIX_CHEAPER);
        c->order_pays = mb.has(GSR_HINT_ORDER_PAYS);
    }
    // occlusion culling earns its keep only if it drops a good part of what an unculled frame keeps; a slab behind which most of the frame
    // still has to be drawn (a ball seen from afar: its near cap finishes few tiles; oblique ground; a wall) costs more than it saves
    if (o.kept_counts) c->cull_pol.on_kept(j.cull, mb.kept, c->opt_cull);
    if (o.slab_done) c->slab_pol.on_frame_done(sl.hints.kept_hint, c->cull_pol.vis_unculled);
    if (j.n > 0 && j.phase != 0) {
        static const bool dbg = std::getenv("GSR_SLAB_DEBUG") != nullptr;
        if (dbg) fprintf(stderr, "[slab] phase %d: clusters through K1 %u, splats kept %u, pairs %u\n", j.phase, mb.clusters, mb.kept, D);
    }
    if (o.end == GSR_FE_TOO_MANY_PAIRS)
        return frame_abort(sl, set_err(GSR_E_TOO_MANY_PAIRS, "gsr_render: the frame's super-tile pairs exceed the limit of %lld", GSR_MAX_PAIRS));
    // (a slot that has never met a pair has no list buffer at all: the frame-end kernels read entry 0 of it unconditionally --
    //  a rank whose rows see nothing, under forced culling or forced front-slab frames, faulted on the null pointer)
    if (o.grow) {
        // (a slot's first buffer may be sized by a frame -- or a front slab -- that shows next to nothing: at least two entries per splat
        //  then, up to 32 MB, so that the frames behind it need not each grow it again.  The sync: a clamped back end may still read the old one)
        const size_t floor_ = sl.pvA ? 0 : std::min<size_t>((size_t)2 * j.n + 4096, (size_t)1 << 22);
        const size_t want = std::max<size_t>((size_t)D + D / 4 + 4096, std::max(floor_, c->pair_want));
        if (const int rc = sl.pvA.ensure_drained(sl.stream, want, want + 4)) return frame_abort(sl, rc);
        c->pair_want = std::max(c->pair_want, want);   // the other frame slot grows before its next frame
    }
    if (o.end == GSR_FE_SLAB_OVERRUN) {
        // Phase 2 of a front-slab frame CONTINUES from what phase 1 left in the target: the clamped back end that has run has composited on
        // top of it, and a second run would composite the same splats again.  The whole frame again, with the buffer that now fits.
        c->st.frames_requeued += 1;
        return abandon_attempt(sl, true);
    }
    if (o.back_end == GSR_BE_TRUNCATED) c->st.frames_truncated += 1;   // (handed over before its count was known: the lists missed their tails)
    if (o.back_end == GSR_BE_REQUEUED) {
        c->st.frames_requeued += 1;
        // the first, clamped back end has already added its tiles' work to the sums k_tile_order reads
        if (sl.sup_work) (void)hipMemsetAsync(sl.sup_work + 256 * sl.sup_par, 0, 256 * sizeof(uint32_t), sl.stream);
    }
    if (o.back_end == GSR_BE_QUEUED || o.back_end == GSR_BE_REQUEUED) {
        const int rc = queue_back_end(c, sl);
        if (rc) return frame_abort(sl, rc);
    }
    sl.last_pairs = D;
    if (o.guard_miss) {   // the guarded plain kernel found covered pixels and did nothing: the depth-tested one draws the frame
        j.blend_guess_plain = false;
        const int rc = queue_blend(c, sl, true, false);
        if (rc) return frame_abort(sl, rc);
    }
    if (o.end == GSR_FE_PHASE_2) {
        // front slab composited: find the finished tiles, then the rest of the frame (same slot, same call arguments)
        const int rc = queue_slab_mid(c, sl);
        if (rc) return frame_abort(sl, rc);
        if (j.timing) { sl.ev_pending = true; sl.ev_all = false; }
        j.open = false;
        const FrameArgs a = j.args;   // (frame_begin rewrites the job)
        return render_again(c, a, 2, nullptr);
    }
    if (!j.deferred) {
        const int rc = queue_frame_end(c, sl);
        if (rc) return frame_abort(sl, rc);
    }
    j.open = false;
    return GSR_OK;
}

// Occlusion culling: wait for k_sum_work's word on the frame just queued (it is the first thing that kernel writes, so the
// host is back in time to queue the next frame behind it): did a tile run off a list cut at its horizon?
static int frame_verdict(gsr_context* c, FrameSlot& sl, bool* broke)
{
    (void)c;
    const FrameJob& j = sl.job;
    volatile unsigned long long* box = sl.h_end;
    unsigned long long v = 0;
    const int wrc = wait_mailbox(sl, box, j.ticket, "culling verdict", &v);
    if (wrc) return wrc;
    *broke = (v & GSR_END_HORIZON_BROKE) != 0ull;
    return GSR_OK;
}

static int finish_open_frames(gsr_context* c)
{
    int rc = GSR_OK;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
        const int r = frame_finish(c, c->slot[k]);
        if (r && !rc) rc = r;
    }
    return rc;
}

// the depth order of ALL splats for the camera position of frame f (k_sort.h): keys -> LSD passes -> c->pos_order
static int build_pos_order(gsr_context* c, FrameSlot& sl, const GsrFrame& f, int key_bits)
{
    const uint32_t n = c->n;
    int rc;
    DevMem<uint32_t> scratch[4];           // the pairs (kA, vA) and (kB, vB) of the sort, gone with the call
    for (DevMem<uint32_t>& m : scratch)
        if ((rc = m.alloc((size_t)n + 256))) return rc;
    uint32_t *kA = scratch[0], *vA = scratch[1], *kB = scratch[2], *vB = scratch[3];
    hipStream_t s = sl.stream;
    hipLaunchKernelGGL(k_pos_keys, dim3(div_up(n, 256)), dim3(256), 0, s, c->geoA, n, f.cam[0], f.cam[1], f.cam[2], f.key_min, f.key_max, kA, vA);
    rc = radix_sort(sl, kA, vA, kB, vB, n, key_bits, true, (uint32_t*)nullptr, RS_XCD_DEPTH != 0);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = set_err(GSR_E_HIP, "position-keyed order: sort failed");
    if (rc) return rc;
    c->pos_order = std::move(scratch[vA == scratch[1] ? 1 : 3]);   // (radix_sort leaves the result in what vA names now)
    c->pos_valid = true;
    c->pos_gen = c->geo_gen;
    std::memcpy(c->pos_cam, f.cam, sizeof c->pos_cam);
    c->pos_kmin = f.key_min; c->pos_kmax = f.key_max;
    return GSR_OK;
}

// ---- frame_begin, stage by stage ----
// What crosses the stage boundaries: the frame's plan and the launch arguments more than one stage needs.  Lives on frame_begin's stack.
struct FrontEnd {
    GsrFramePlan p;
    bool pos_match = false;            // the position-keyed order is this frame's (plan_frame; queue_pos_order drops or builds it otherwise)
    SortKey key_now;                   // what this frame's depth order is cached under (queue_sort)
    int rounds = 0; uint32_t ngroups = 0;   // the cull grid: rounds per workgroup and workgroups of k_cluster_cull, whose segments K1 walks
    int hist_shift = 0;                // front-slab frames: key bits dropped by the slab histogram
    GsrDepthPyrArgs dp{};              // depth-tested frames: the pyramid pass ...
    uint32_t n_dp = 0;                 // ... its detection workgroups in front of k_cluster_cull's (0: none in this launch)
    GsrDepthCull dc_clus{nullptr, nullptr, nullptr}, dc_k1{nullptr, nullptr, nullptr};   // ... and what the cluster pass and K1 cull against
    GsrK1Scatter scat{};               // the small-frame sort's bucket pass inside K1
};

// argument checks, the slot and its stream, the slot's previous frame finished, the job and its derived sizes
static int frame_open(gsr_context* c, const FrameArgs& a, FrameSlot*& slot)
{
    const gsr_camera* cam = &a.cam;
    if (c->uploading) return set_err(GSR_E_INVALID, "gsr_render: upload in progress");
    if (cam->width <= 0 || cam->height <= 0 || cam->width > GSR_MAX_DIM || cam->height > GSR_MAX_DIM)
        return set_err(GSR_E_INVALID, "gsr_render: bad framebuffer size %dx%d (max %d)", cam->width, cam->height, GSR_MAX_DIM);
    if (!c->has_geometry) return set_err(GSR_E_NO_GEOMETRY, "gsr_render: nothing uploaded");
    HIP_TRY(hipSetDevice(c->device));

    // Frames alternate between the slots.  Everything up to the blend kernel touches only the slot's
    // private arrays (plus the read-only geometry), so it may run while the previous frame -- and
    // whatever the caller queued on the public stream -- is still executing.
    FrameSlot& sl = c->slot[c->frame_no % (uint64_t)c->nslots];
    slot = &sl;
    int rc = frame_finish(c, sl);   // a deferred frame of this slot: look at its pair count now
    if (rc) return rc;
    // strictly serial frames run on the public stream itself: nothing to hand over, no events; with two frames in flight a
    // slot runs on its own stream and the result is ordered onto the public stream by an event
    hipStream_t want = (c->nslots == 1) ? c->stream : sl.own;
    if (want != sl.stream) {
        HIP_TRY(hipStreamSynchronize(sl.stream));
        sl.stream = want;
    }
    // (the other slot met a frame that outgrew this slot's list buffer)
    if (sl.pvA.cap() > 0 && (rc = sl.pvA.ensure_drained(sl.stream, c->pair_want, c->pair_want + 4))) return rc;

    FrameJob& j = sl.job;
    j = FrameJob();
    j.args = a;
    build_frame(c, cam, &j.f);
    j.n = c->n;
    j.local_tiles = j.f.tiles_x * j.f.local_tiles_y;
    j.band_rows = ctx_band_rows(c, cam->height);
    j.out_px = (size_t)j.band_rows * cam->width;
    j.n_super = j.f.stiles_x * j.f.stiles_y;
    j.use_map = c->opt_swizzle != 0;
    return GSR_OK;
}

// the frame's regime (gsr_frame_plan.h: the policies' per-frame events happen in there), the frame counters, the ticket
static void plan_frame(gsr_context* c, FrameSlot& sl, FrontEnd& fe, bool allow_cull, int phase_in)
{
    FrameJob& j = sl.job;
    const FrameArgs& a = j.args;
    const gsr_camera* cam = &a.cam;
    const GsrFrame& f = j.f;
    fe.key_now = SortKey{c->geo_gen, c->shard_index, c->shard_count, c->shard_layout, c->opt_flags, c->band_first, c->band_tile_rows, *cam};
    int sig[7] = {0, 0, 0, 0, 0, 0, (int)c->geo_gen};
    tile_sig(f, sig);
    GsrPlanIn in;
    in.phase_in = phase_in; in.allow_cull = allow_cull; in.out_is_device = a.out_is_device; in.has_depth = a.depth != nullptr;
    in.n = j.n; in.nclus = c->nclus; in.sh_order = f.sh_order; in.key_min = f.key_min; in.key_max = f.key_max;
    in.opt_deferred = c->opt_deferred; in.opt_lazy = c->opt_lazy; in.opt_cull = c->opt_cull; in.opt_slab = c->opt_slab; in.opt_cluster = c->opt_cluster;
    in.opt_sort_cache = c->opt_sort_cache; in.opt_local_sort = c->opt_local_sort; in.opt_k1_scatter = c->opt_k1_scatter;
    in.opt_scatter_direct = c->opt_scatter_direct; in.opt_mid_sort = c->opt_mid_sort; in.opt_bn_items = c->opt_bn_items;
    in.full_keys = (c->opt_flags & GSR_FLAG_FULL_KEYS) != 0; in.shard_count = c->shard_count;
    in.timing = c->opt_timing != 0 && (c->opt_timing >= 2 || c->frame_no % (uint64_t)c->opt_timing_every == 0);
    in.timing_all = c->opt_timing >= 2;   // level 1 brackets only the blend kernel (events 5 and 6)
    in.opt_timing = c->opt_timing;
    in.lazy_pays = c->lazy_pays; in.prefix_cheaper = c->prefix_cheaper; in.prefix_valid = c->prefix_valid; in.bbox_ok = c->bbox_ok;
    in.horizon_match = sl.horizon_valid && std::memcmp(sig, sl.horizon_sig, sizeof sig) == 0;
    in.hpyr_re = sl.hpyr_re;
    in.sort_match = sl.sort_valid && sl.sort_key.same(fe.key_now);
    in.sorted_culled = sl.sorted_culled; in.sorted_dculled = sl.sorted_dculled;
    in.pos_match = c->pos_valid && c->pos_gen == c->geo_gen && std::memcmp(c->pos_cam, cam->cam_pos, sizeof c->pos_cam) == 0 &&
                   c->pos_kmin == f.key_min && c->pos_kmax == f.key_max;
    in.same_pos = c->last_cam_set && std::memcmp(c->last_cam, cam->cam_pos, sizeof c->last_cam) == 0;
    in.hints = sl.hints;
    fe.pos_match = in.pos_match;
    fe.p = gsr_plan_frame(in, c->cull_pol, c->slab_pol, sl.local_pol, c->classic_once, [&] { return camera_jumped(c, sl.horizon_cam, *cam); });
    const GsrFramePlan& p = fe.p;
    sl.last_plan = p;
    j.deferred = p.deferred; j.lazy = p.lazy; j.cull = p.cull; j.phase = p.phase; j.timing = p.timing; j.timing_all = p.timing_all;
    j.dcull = p.dcull; j.local_sort = p.local || p.local_phase; j.bn_items = p.bn_items; j.bn_grid = p.bn_grid; j.k1_grid = p.k1_grid;
    j.f.cull_dilate = p.cull_dilate;
    j.f.phase = p.phase;
    c->st.frames_jumped += p.jumped;
    c->st.frames_culled += p.cull;
    c->st.frames_slab += p.phase == 1;
    c->st.frames_lazy += p.lazy && j.n > 0 && phase_in == 0;
    j.ticket = ++sl.ticket ? sl.ticket : ++sl.ticket;   // (never 0: the mailbox starts at 0)
    if (j.timing) harvest_slot(c, sl);
}

// Everything the frame's kernels need in place before any of them is queued: the slot's arrays sized for the frame, the caller's
// host buffers staged (StageBuf), the targets chosen.  Errors return directly: nothing of the frame is in the stream yet.
static int stage_frame_buffers(gsr_context* c, FrameSlot& sl)
{
    FrameJob& j = sl.job;
    const FrameArgs& a = j.args;
    const gsr_camera* cam = &a.cam;
    const GsrFrame& f = j.f;
    hipStream_t s = sl.stream;
    int rc;
    // the caller's stream position now: the blend kernel (the only writer of caller-visible memory)
    // waits for it, so an output buffer that earlier work on the public stream still reads is safe
    j.direct = sl.stream == c->stream;
    if (!j.direct) HIP_TRY(hipEventRecord(sl.ev_user, c->stream));

    // per-tile bookkeeping + super-tile ranges
    if ((rc = sl.tiles.ensure_drained(s, (size_t)j.local_tiles + 1))) return rc;
    // (the transmittance a front slab leaves behind, per pixel of the band)
    if (j.phase == 1 && (rc = sl.tbuf.ensure_drained(s, j.out_px))) return rc;
    if (j.use_map && (rc = build_tile_map(c, f))) return rc;
    j.d_depth = a.depth;
    if (a.depth && !a.depth_is_device) {
        if ((rc = sl.depth_stage.upload(s, a.depth, (size_t)cam->width * cam->height * sizeof(float)))) return rc;
        j.d_depth = reinterpret_cast<const float*>(sl.depth_stage.p.get());
    }
    // A background: the colour as it is; a device image read in place; a host image staged in the slot's own buffer like a host depth
    // buffer -- by EVERY attempt of the frame (a repair, a re-queue, a front slab's phase 2 come through here again with the caller's
    // arguments), so whatever is composited last read the original background
    if (a.bg.kind != 0) {
        j.bg.kind = a.bg.kind; j.bg.format = a.bg.format;
        std::memcpy(j.bg.rgba, a.bg.rgba, sizeof j.bg.rgba);
        j.bg.image = a.bg.kind == GSR_BG_IMAGE ? a.bg.image : nullptr;
        if (a.bg.kind == GSR_BG_IMAGE && !a.bg.image_is_device) {
            if ((rc = sl.bgb.upload(s, a.bg.image, (size_t)cam->width * cam->height * (size_t)gsr_format_pixel_bytes(a.bg.format)))) return rc;
            j.bg.image = sl.bgb.p.get();
        }
    }
    // Depth-tested frames: the tile-max pyramid of the opaque pass's depth (k_cluster.h), rebuilt every frame (the buffer's content is
    // the caller's), one per slot; the second phase of a front-slab frame uses the first one's.  GSR_OPT_OCCLUSION_CULL = 0 switches
    // it off like every other occlusion test (what is left is k_blend's own per-quadrant classification and per-fragment compare).
    if (j.dcull) {
        frame_depth_codes(c, cam, &j.f);
        const size_t need = (size_t)f.pyr_off[GSR_PYR_LEVELS - 1] + (size_t)gsr_pyr_dim(f.tiles_x, GSR_PYR_LEVELS - 1) * gsr_pyr_dim(f.tiles_y, GSR_PYR_LEVELS - 1) + 16;
        if (!sl.dactive) sl.dpyr.reset();   // (a slot whose first depth-tested frame failed half-way starts over)
        if (need > sl.dpyr.cap()) {
            if ((rc = sl.dpyr.ensure_drained(s, need, 5 * need))) return rc;
            HIP_TRY(hipMemsetAsync(sl.dpyr, 0, 5 * need * sizeof(float), s));   // (levels 4 and 5 start cleared; afterwards every frame clears the next one's)
            if (!sl.dactive) {
                if ((rc = sl.dactive.alloc(2))) return rc;
                HIP_TRY(hipMemsetAsync(sl.dactive, 0, 2 * sizeof(uint32_t), s));   // (on the frame's stream: a null-stream memset is not ordered against it)
            }
        }
        if (j.phase != 2) sl.dpar ^= 1;
        j.dpar = sl.dpar;
    }
    j.target = a.out;
    j.format = c->target_format;
    const size_t bpp = (size_t)gsr_format_pixel_bytes(j.format);
    // (a packed target, front-slab frame: phase 2 continues from phase 1's f32 pixels, kept in a buffer of the slot's own)
    // (... and so does a frame over a background in any format: the target holds composited pixels)
    if ((j.format != GSR_TARGET_RGBA32F || a.bg.kind != 0) && j.phase == 1 && (rc = sl.fb32.ensure_drained(s, j.out_px * 4))) return rc;
    // Host targets: the band is composited into the slot's staging image -- and plane, with the depth AOV -- and copied back by
    // queue_frame_end.  Padding rows read as zeros (StageBuf): the image is cleared per band shape and format, the plane per band shape.
    int band[6];
    tile_sig(f, band);
    if (!a.out_is_device) {
        band[5] = j.format;
        if ((rc = sl.fb.ensure(s, j.out_px * bpp)) || (rc = sl.fb.clear_if_reshaped(s, band, j.out_px * bpp))) return rc;
        j.target = reinterpret_cast<float*>(sl.fb.p.get());
    }
    if (a.aov != 0 && a.aov_out != nullptr) {
        j.aov_target = reinterpret_cast<float2*>(a.aov_out);
        if (!a.out_is_device) {
            band[5] = 0;
            if ((rc = sl.aovb.ensure(s, j.out_px * sizeof(float2))) || (rc = sl.aovb.clear_if_reshaped(s, band, j.out_px * sizeof(float2)))) return rc;
            j.aov_target = reinterpret_cast<float2*>(sl.aovb.p.get());
        }
    }
    return GSR_OK;
}

// The position-keyed order (the reference's rule, src/GSplatRenderer.C:165-186): dropped when the position moved, built the second
// time a position is seen
static int queue_pos_order(gsr_context* c, FrameSlot& sl, FrontEnd& fe)
{
    if (fe.p.want_pos && !fe.pos_match) {
        c->pos_valid = false;
        if (const int rc = fe.p.ordered ? build_pos_order(c, sl, sl.job.f, fe.p.key_bits) : GSR_OK) return rc;
    }
    std::memcpy(c->last_cam, sl.job.args.cam.cam_pos, sizeof c->last_cam);
    c->last_cam_set = true;
    return GSR_OK;
}

// cluster culling (k_cluster.h): which clusters of 64 storage-ordered splats can draw anything in this frame
static int queue_cull(gsr_context* c, FrameSlot& sl, FrontEnd& fe)
{
    FrameJob& j = sl.job;
    const GsrFrame& f = j.f;
    const GsrFramePlan& p = fe.p;
    hipStream_t s = sl.stream;
    if (j.n == 0) return GSR_OK;
    cluster_grid(c->nclus, &fe.rounds, &fe.ngroups);
    if ((c->opt_flags & GSR_FLAG_CULL_ROUNDS) && c->nclus > 0) {   // (test hook: the several-rounds-per-workgroup form clouds beyond 33 M splats take)
        fe.rounds = std::max(fe.rounds, 3);
        fe.ngroups = div_up(c->nclus, (uint32_t)CC_THREADS * (uint32_t)fe.rounds);
    }
    // (front-slab frames: phase 1 leaves a histogram of the survivors' nearest keys and k_slab_pick takes the slab key from it;
    //  phase 2 culls against the tiles phase 1 finished)
    fe.hist_shift = p.key_bits > 10 ? p.key_bits - 10 : 0;
    const float* pyr = j.phase == 2 ? sl.hpyr2 : ((j.cull && !p.ordered) ? sl.hpyr : (const float*)nullptr);
    const GsrSlabPick pk{(uint32_t)c->slab_min, (uint32_t)c->slab_max, (uint32_t)c->slab_frac, f.key_max - f.key_min};
    // depth-tested frames: the opaque pass's tile-max depth pyramid -- where the previous depth-tested frame found opaque geometry in
    // its buffer, in a launch of its own in front of everything (k_cluster_cull and K1 cull against it); otherwise -- a buffer
    // cleared to the far plane, the common case -- NO pyramid: the first workgroups of k_cluster_cull's launch only look whether a
    // pixel is covered at all (k_cluster.h: gsr_depth_detect_block), and a frame in which geometry appears goes without depth culling.
    // Whatever the guess, the pixels are the same: the tests are conservative and k_blend compares every fragment.
    GsrDepthPyrArgs& dp = fe.dp;
    if (j.dcull) {
        float* const dp0 = sl.dpyr + (size_t)(2 * j.dpar) * sl.dpyr.cap();
        float* const dq0 = sl.dpyr + (size_t)(2 * (j.dpar ^ 1)) * sl.dpyr.cap();
        fe.dc_k1 = GsrDepthCull{dp0, j.phase == 2 ? (const float*)nullptr : dp0 + sl.dpyr.cap(), sl.dactive + j.dpar};
        if (j.phase == 2 && !sl.dpyr_built) { fe.dc_k1 = GsrDepthCull{nullptr, nullptr, nullptr}; j.dblind = true; }   // (phase 1 built none)
        if (j.phase != 2) {
            dp.depth = j.d_depth; dp.pyr = dp0; dp.pyrc = dp0 + sl.dpyr.cap(); dp.pyr_next = dq0; dp.pyrc_next = dq0 + sl.dpyr.cap(); dp.active = sl.dactive; dp.par = j.dpar;
            dp.tcov = sl.dpyr + 4 * sl.dpyr.cap();
            // (a culled frame: the tiles that were classic when the horizons were left get no depth clause)
            dp.stat = (j.cull && sl.hstat_valid) ? sl.hstat : (const float*)nullptr;
            j.dstat = dp.stat != nullptr;
            dp.width = f.width; dp.height = f.height; dp.tiles_x = f.tiles_x; dp.tiles_y = f.tiles_y;
            for (int l = 0; l < GSR_PYR_LEVELS; ++l) dp.off[l] = f.pyr_off[l];
            if (c->depth_active) {
                // (measured and rejected, round 6: the pass inside k_cluster_cull's launch here too, the cluster workgroups waiting on a
                //  count of finished pyramid workgroups before their depth tests: 3650 fps against 4245 -- LAB_NOTES.md)
                hipLaunchKernelGGL(k_depth_pyramid, dim3((uint32_t)gsr_depth_pyramid_blocks(f.tiles_x, f.tiles_y)), dim3(1024), 0, s, dp);
                if (c->opt_cluster && !p.ordered) fe.dc_clus = fe.dc_k1;
                sl.dpyr_built = true;
            } else {
                fe.n_dp = (uint32_t)gsr_depth_detect_blocks(f.width, f.height);
                j.dblind = true;
                j.dstat = false;
                sl.dpyr_built = false;
                fe.dc_k1 = GsrDepthCull{nullptr, nullptr, nullptr};
            }
        } else if (c->opt_cluster && sl.dpyr_built) {
            fe.dc_clus = fe.dc_k1;       // (phase 1 built it)
        }
    }
    if (j.phase == 1) {   // a first pass for the histogram alone (the pass below takes the slab key from it and keeps the slab's clusters only)
        // (the histogram is cleared by phase 2's cull pass; a phase 1 that never got its phase 2 -- its small-frame sort gave a bucket
        //  up, an error in between -- left its counts behind: they would skew this frame's slab key, never its pixels)
        if (sl.slab_dirty && hipMemsetAsync(sl.slab, 0, (size_t)GSR_SLAB_BINS * sizeof(uint32_t), s) != hipSuccess)
            return set_err(GSR_E_HIP, "gsr_render: clearing the slab histogram failed");
        sl.slab_dirty = true;
        const int n45 = gsr_pyr_dim(f.tiles_x, 4) * gsr_pyr_dim(f.tiles_y, 4) + gsr_pyr_dim(f.tiles_x, 5) * gsr_pyr_dim(f.tiles_y, 5);
        hipLaunchKernelGGL(j.dcull ? k_cluster_cull<true> : k_cluster_cull<false>, dim3(fe.ngroups + fe.n_dp), dim3(CC_THREADS), 0, s, f, c->clusA, c->clusB, c->nclus, fe.rounds, c->opt_cluster,
                           (const float*)nullptr, sl.cseg, sl.ccnt, 1, sl.slab, fe.hist_shift, sl.slab + GSR_SLAB_BINS, pk, sl.hpyr2 + f.pyr_off[4], n45,
                           (uint32_t*)nullptr, (uint32_t*)nullptr, dp, fe.n_dp, fe.dc_clus);
        fe.n_dp = 0;      // (looked at: not again in the pass below)
    }
    if (j.phase == 2) sl.slab_dirty = false;   // (mode 3 below clears the histogram for the slot's next front-slab frame)
    hipLaunchKernelGGL(j.dcull ? k_cluster_cull<true> : k_cluster_cull<false>, dim3(fe.ngroups + fe.n_dp), dim3(CC_THREADS), 0, s, f, c->clusA, c->clusB, c->nclus, fe.rounds, p.ordered ? 0 : c->opt_cluster,
                       pyr, sl.cseg, sl.ccnt,   // (ordered: slots, not clusters -- all of them)
                       j.phase == 1 ? 2 : (j.phase == 2 ? 3 : 0), sl.slab, fe.hist_shift, sl.slab + GSR_SLAB_BINS, pk, (float*)nullptr, 0,
                       j.local_sort ? sl.bkt_cnt : (uint32_t*)nullptr, sl.d_counts + 2, dp, fe.n_dp, fe.dc_clus);
    sl.last_cc_groups = p.ordered ? 0u : fe.ngroups;
    sl.last_cc_per = (uint32_t)CC_THREADS * (uint32_t)fe.rounds;
    return GSR_OK;
}

// K1 over the survivors (the plan's grid: a frame that keeps more loops); on a cache hit (identical frame description) the sorted
// (keyA, valA) are kept and K1's key/payload output goes to the scratch buffers
static int queue_preprocess(gsr_context* c, FrameSlot& sl, FrontEnd& fe)
{
    const FrameJob& j = sl.job;
    const GsrFrame& f = j.f;
    const GsrFramePlan& p = fe.p;
    if (j.n == 0) return GSR_OK;
    // The small-frame sort's bucket pass runs inside K1 (a key's place in its bucket = one atomic), over the plan's buckets; front-slab
    // phases: over the phase's own range, which k_slab_pick left on the device
    GsrK1Scatter& scat = fe.scat;
    if (p.k1_scatters) {
        scat.key = sl.bkt_key; scat.val = sl.bkt_val; scat.cnt = sl.bkt_cnt; scat.failed = sl.d_counts + 2;
        scat.range_dev = p.local_phase ? sl.slab + GSR_SLAB_BINS + (j.phase == 1 ? 2 : 4) : (const uint32_t*)nullptr;
        scat.lo = p.bk_lo; scat.shift = p.bk_shift;
    }
    // (two instantiations: the one that leaves the colours pending has no SH evaluation in it and runs at 8 waves per SIMD instead of 6)
    // (a frame with the depth AOV takes the depth-tested twins for the window depths they write; without a depth buffer it brings no
    //  pyramids -- dc_k1 is empty -- so nothing is culled against a depth that is not there)
    const bool k1_zwin = j.d_depth != nullptr || j.aov_target != nullptr;
    hipLaunchKernelGGL(k1_zwin ? (j.lazy ? k_preprocess_lazy_depth : k_preprocess_depth) : (j.lazy ? k_preprocess_lazy : k_preprocess), dim3(j.k1_grid ? j.k1_grid : 1u), dim3(GSR_K1_THREADS), 0, sl.stream, j.n, c->cap, f, c->geoA, c->geoB, c->col,
                       sl.rec, (p.cache_hit || p.ordered) ? sl.keyB : sl.keyA, (p.cache_hit || p.ordered) ? sl.valB : sl.valA,
                       k1_zwin ? sl.zwin : (float*)nullptr, j.phase == 2 ? sl.hpyr2 : (j.cull ? sl.hpyr : (const float*)nullptr), sl.blk_cnt,
                       sl.cseg, sl.ccnt, fe.ngroups, (uint32_t)CC_THREADS * (uint32_t)fe.rounds, sl.d_counts, scat,
                       // (the count of sorted splats starts at zero: a frame whose clusters are ALL culled runs no sort workgroup that
                       //  could say so, and the binning kernels would walk the previous frame's order; a static redraw keeps its order)
                       p.cache_hit ? (uint32_t*)nullptr : sl.d_n,
                       p.ordered ? c->pos_order : (const uint32_t*)nullptr, sl.slab + GSR_SLAB_BINS, fe.dc_k1);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GSR_OK : set_err(GSR_E_HIP, "k_preprocess: %s", hipGetErrorString(e));
}

// The small-frame sort's launches (k_sort.h) on operands given one by one: what queue_local_sort queues for a frame and what
// gsr_debug_sort_frame queues for a test's arrays.  K1's compacted slots (keys, vals: cnt[b] items at the head of block b, *slots_dev
// slots filled, n_slots at most) -> the bucket regions (bkt_cnt zero on entry) -> sorted, in place of the slots; *n_out = their number.
enum LocalScatter { LS_IN_K1 = 0, LS_DIRECT = 1, LS_PER_WAVE = 2, LS_GATHER = 3 };
struct LocalSortOps {
    uint32_t* keys; uint2* vals;       // K1's slots in, the sorted frame out
    const uint32_t* cnt;               // per 256-slot block
    const uint32_t* slots_dev;
    uint32_t n_slots;
    LocalScatter scatter;              // which kernel fills the buckets (LS_IN_K1: K1 did)
    uint32_t wave_grid;                // LS_PER_WAVE: workgroups (a grid below div_up(blocks, 4) loops)
    int shift; uint32_t lo; int key_bits;
    const uint32_t* range;             // or: { lo, shift } on the device (LS_PER_WAVE and the local kernel read them there)
    uint32_t* bkt_cnt; uint32_t* bkt_key; uint2* bkt_val;
    uint32_t* failed; uint32_t* n_out;
};
static int launch_local_sort(hipStream_t s, const LocalSortOps& o)
{
    if (o.scatter == LS_DIRECT)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bucket_scatter_direct<uint2>), dim3(o.n_slots / RS_SRC_BLOCK), dim3(RS_SRC_BLOCK), 0, s, o.keys, o.vals,
                           o.slots_dev, o.shift, o.lo, o.cnt, o.bkt_cnt, o.bkt_key, o.bkt_val, o.failed);
    else if (o.scatter == LS_PER_WAVE)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bucket_scatter_k1<uint2>), dim3(o.wave_grid), dim3(256), 0, s, o.keys, o.vals,
                           o.n_slots / RS_SRC_BLOCK, o.slots_dev, o.shift, o.lo, o.cnt, o.bkt_cnt, o.bkt_key, o.bkt_val, o.failed, o.range);
    else if (o.scatter == LS_GATHER)   // (A/B: the general gathering scatter, 2048 slots per workgroup)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bucket_scatter<uint2, true>), dim3(div_up(o.n_slots, RS_TILE)), dim3(RS_THREADS), 0, s, o.keys, o.vals, o.n_slots, o.slots_dev,
                           o.shift, o.lo, o.cnt, o.bkt_cnt, o.bkt_key, o.bkt_val, (uint32_t*)nullptr, o.failed);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radix_local<uint2>), dim3(BK_BUCKETS), dim3(RL_THREADS), 0, s, o.bkt_cnt, o.shift, o.key_bits, o.lo,
                       o.bkt_key, o.bkt_val, o.keys, o.vals, o.failed, o.n_out, o.range);
    return hipGetLastError() == hipSuccess ? GSR_OK : set_err(GSR_E_HIP, "small-frame sort: launch failed");
}

// the small-frame sort of a frame: K1's compacted slots -> bucket regions (counters and *d_n were cleared by K1) -> sorted (keyA, valA),
// over the plan's buckets; a front-slab phase: over the phase's own key range, which k_slab_pick left on the device
static int queue_local_sort(gsr_context* c, FrameSlot& sl, const FrontEnd& fe)
{
    const FrameJob& j = sl.job;
    const GsrFramePlan& p = fe.p;
    LocalSortOps o{};
    o.keys = sl.keyA; o.vals = sl.valA; o.cnt = sl.blk_cnt; o.slots_dev = sl.d_counts; o.n_slots = p.n_slots;
    o.scatter = p.k1_scatters ? LS_IN_K1
              : (p.scatter_direct && !p.local_phase) ? LS_DIRECT
              : (c->opt_scatter_direct >= 0 || p.local_phase) ? LS_PER_WAVE : LS_GATHER;
    // (grid: K1's own estimate of its workgroup-iterations, four per workgroup here)
    o.wave_grid = std::max(1u, std::min(div_up(p.n_slots / RS_SRC_BLOCK, 4u), div_up(j.k1_grid, 4u) + 16u));
    o.range = p.local_phase ? sl.slab + GSR_SLAB_BINS + (j.phase == 1 ? 2 : 4) : (const uint32_t*)nullptr;
    o.lo = p.local_phase ? 0u : p.bk_lo;
    o.shift = p.local_phase ? 0 : p.bk_shift;
    o.key_bits = p.key_bits;
    o.bkt_cnt = sl.bkt_cnt; o.bkt_key = sl.bkt_key; o.bkt_val = sl.bkt_val;
    o.failed = sl.d_counts + 2; o.n_out = sl.d_n;
    return launch_local_sort(sl.stream, o);
}

// The position-keyed order's launches: the heads of K1's 256-slot blocks (cnt[k] items each, *slots_dev slots filled, 256 m_max at
// most), one after the other -> dense (keys_out, vals_out); *n_out = their number.  pre: m_max words of scratch.
static int launch_ordered_compact(hipStream_t s, const uint32_t* keys_in, const uint2* vals_in, const uint32_t* cnt, const uint32_t* slots_dev,
                                  uint32_t m_max, uint32_t* pre, uint32_t* keys_out, uint2* vals_out, uint32_t* n_out)
{
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, cnt, slots_dev, pre, n_out);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_compact_blocks<uint2>), dim3(m_max), dim3(RS_SRC_BLOCK), 0, s, keys_in, vals_in, cnt, pre,
                       slots_dev, keys_out, vals_out);
    return hipGetLastError() == hipSuccess ? GSR_OK : set_err(GSR_E_HIP, "position-keyed order: launch failed");
}

// the frame's depth order in (keyA, valA): kept (a static redraw), compacted from K1's blocks (the position-keyed order), or sorted
static int queue_sort(gsr_context* c, FrameSlot& sl, FrontEnd& fe)
{
    FrameJob& j = sl.job;
    const GsrFramePlan& p = fe.p;
    hipStream_t s = sl.stream;
    int rc;
    if (p.cache_hit) {
        c->st.sorts_skipped += 1;
        return GSR_OK;
    }
    if (p.ordered) {
        // K1 walked the splats nearest first: the heads of its 256-slot blocks, one after the other, ARE the sorted frame
        const uint32_t m_max = p.n_slots / RS_SRC_BLOCK;
        if ((rc = ensure_counts(c->blk_pre, (size_t)m_max + 8))) return rc;
        if ((rc = launch_ordered_compact(s, sl.keyB, sl.valB, sl.blk_cnt, sl.d_counts, m_max, c->blk_pre, sl.keyA, sl.valA, sl.d_n))) return rc;
        c->st.sorts_skipped += 1;
        sl.key_min = j.f.key_min;
        sl.sort_valid = false;       // (what the slot holds is this frame's kept set only)
        sl.sorted_culled = j.cull;
        return GSR_OK;
    }
    if (p.local_phase || p.local) {
        rc = queue_local_sort(c, sl, fe);
    } else {
        uint32_t *kA = sl.keyA, *kB = sl.keyB;
        uint2 *vA = sl.valA, *vB = sl.valB;
        rc = radix_sort(sl, kA, vA, kB, vB, p.n_slots, p.key_bits, !(c->opt_flags & GSR_FLAG_FULL_KEYS), sl.d_n, RS_XCD_DEPTH != 0, sl.blk_cnt, sl.d_counts, p.mid_sort);
        if (kA != sl.keyA) { sl.keyA.swap(sl.keyB); sl.valA.swap(sl.valB); }   // (the handles follow the pairs' ping-pong: the result is in the A pair)
    }
    if (rc) return rc;
    sl.key_min = j.f.key_min;
    sl.sort_valid = j.phase == 0;    // (a phase's order holds a part of the frame only)
    sl.sort_key = fe.key_now;
    sl.sorted_culled = j.cull;
    sl.sorted_dculled = j.dcull;     // (until the frame's mailbox says that its depth buffer culled nothing: frame_finish)
    j.sort_fresh = true;
    return GSR_OK;
}

// coarse binning as a counting sort (k_binning.h): count -> scan -> ranges -> [pair count to the host] -> place; then the back end,
// speculatively where a list buffer exists, and a deferred frame's end
static int queue_binning(gsr_context* c, FrameSlot& sl, FrontEnd& fe)
{
    FrameJob& j = sl.job;
    const GsrFrame& f = j.f;
    hipStream_t s = sl.stream;
    int rc;
    hipError_t e = hipSuccess;
    if (j.n > 0) {
        const uint32_t bn_tile = (uint32_t)BN_THREADS * (uint32_t)j.bn_items;
        const uint32_t nblk = fe.p.bn_blocks;
        if ((rc = ensure_counts(sl.hist, (size_t)BN_BINS * nblk + 8))) return rc;
        const GsrShard shd = gsr_frame_shard(f, f.rect_shift);
        // (+ the extra work items of the blocks that are split by rows of super-tiles: k_binning.h, BN_SPLIT_TILES)
        const uint32_t bn_extra = (uint32_t)BN_SPLIT_TILES * (uint32_t)std::max(f.stiles_y - 1, 0);
#define GSR_COUNT(I) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bin_count<I>), dim3(j.bn_grid + bn_extra), dim3(BN_THREADS), 0, s, sl.valA, sl.d_n, f.super_shift - f.rect_shift, \
                                        shd, f.stiles_x, f.stiles_y, sl.hist, nblk)
        if (j.bn_items == 1) GSR_COUNT(1); else if (j.bn_items == 2) GSR_COUNT(2); else GSR_COUNT(4);
#undef GSR_COUNT
        hipLaunchKernelGGL(k_scan_rows, dim3(BN_BINS), dim3(SC_THREADS), 0, s, sl.hist, nblk, sl.totals, sl.d_n, j.n, bn_tile);
        // the list ranges and the pair count: formed by k_bin_place itself (queue_back_end) when the back end is queued
        // speculatively; a frame without a list buffer needs the count first
        if (!(sl.pvA.cap() > 0)) hipLaunchKernelGGL(k_bin_ranges, dim3(1), dim3(BN_BINS), 0, s, range_args(c, sl));
        e = hipGetLastError();
    } else {
        e = hipMemsetAsync(sl.tiles.sstart, 0, ((size_t)j.n_super + 1) * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(sl.tiles.send, 0, ((size_t)j.n_super + 1) * 4, s);
    }
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_render: binning: %s", hipGetErrorString(e));
    j.speculative = j.n > 0 && sl.pvA.cap() > 0;
    j.ranges_folded = j.speculative;
    if (j.speculative || j.n == 0) {
        if ((rc = queue_back_end(c, sl))) return rc;
    } else {
        j.deferred = false;   // no list buffer yet (first frame): the host has to size it before anything is composited
    }
    if (j.deferred && (rc = queue_frame_end(c, sl))) return rc;
    sl.last_supers = j.n_super;
    sl.last_tiles_x = f.tiles_x;
    sl.last_local_ty = f.local_tiles_y;
    sl.super_tile = f.super; sl.stiles_x = f.stiles_x; sl.stiles_y = f.stiles_y;
    c->st.frames += 1;
    c->frame_no += 1;
    sl.frame_id = c->frame_no;
    // (the frame's counters are written to the host mirror by k_sum_work; they are read in gsr_get_stats)
    return GSR_OK;
}

#ifdef GSR_HOST_TIMING
// the host's share of a frame, from the previous frame's verdict (frame_check) to K1's launch, averaged over 100 frames
static void host_timing_note(double t_enter, double t_pre)
{
    if (!(g_t_verdict > 0)) return;
    g_acc_py += t_enter - g_t_verdict; g_acc_pre += t_pre - t_enter; g_acc_launch += now_us() - t_pre; ++g_acc_n;
    if (g_acc_n % 100 == 0)
        fprintf(stderr, "[host timing] verdict -> gsr_render %.1f us, frame_begin before K1 %.1f us, K1 launch %.1f us (avg of %ld)\n",
                g_acc_py / g_acc_n, g_acc_pre / g_acc_n, g_acc_launch / g_acc_n, g_acc_n);
    g_t_verdict = 0;
}
#endif

static int frame_begin(gsr_context* c, const FrameArgs& a, FrameSlot** used, bool allow_cull, int phase_in /* 2 = the second phase of a front-slab frame */)
{
#ifdef GSR_HOST_TIMING
    const double t_enter = now_us();
#endif
    FrameSlot* slot = nullptr;
    FrontEnd fe;
    int rc = frame_open(c, a, slot);
    if (used && slot) *used = slot;
    if (rc) return rc;
    FrameSlot& sl = *slot;
    plan_frame(c, sl, fe, allow_cull, phase_in);
    if ((rc = stage_frame_buffers(c, sl))) return rc;

    // THE BOUNDARY.  Up to here nothing of the frame is in the stream and a stage's error is returned as it is.  From here on kernels
    // are queued, some of which write the caller's buffers: the stages below return their error and frame_abort drains the stream.
    sl.job.open = true;
    rc = mark(sl, 0);
    if (!rc) rc = queue_pos_order(c, sl, fe);
#ifdef GSR_HOST_TIMING
    const double t_pre = now_us();
#endif
    if (!rc) rc = queue_cull(c, sl, fe);
    if (!rc) rc = queue_preprocess(c, sl, fe);
#ifdef GSR_HOST_TIMING
    if (sl.job.n > 0) host_timing_note(t_enter, t_pre);
#endif
    if (!rc) rc = mark(sl, 1);
    if (!rc) rc = queue_sort(c, sl, fe);
    if (!rc) rc = mark(sl, 2);
    if (!rc) rc = queue_binning(c, sl, fe);
    return rc ? frame_abort(sl, rc) : GSR_OK;
}

static FrameSlot* latest_slot(gsr_context* c);
// a culled frame is handed over only once it has checked itself; one that broke a horizon is rendered again, complete
static int frame_check(gsr_context* c, FrameSlot& first, const FrameArgs& a)
{
    // A frame that is rendered again is checked again: the repair of a culled frame may itself meet a bucket its small-frame sort
    // gives up, or -- as a front-slab frame -- a list buffer its second phase overruns.  Every reason removes itself (the re-sort
    // takes the global passes, the redo finds the buffer grown, the repair does not cull), so a handful of rounds is the most a
    // frame can need; found by tools/fuzz_parity.py: the second re-render used to be handed over unchecked.
    FrameSlot* cur = &first;
    for (int round = 0; round < 8; ++round) {
        FrameSlot& slot = *cur;
        int rc;
        if (slot.job.sort_failed || slot.job.redo) {
            // the small-frame sort met a bucket far beyond its prediction and left it unsorted: the frame again, with the global sort
            // (and without culling: a prediction that far off means the view jumped, and the horizons with it) -- or the attempt was
            // abandoned for a reason of its own (frame_finish): the frame again, as it was
            if (slot.job.sort_failed) {
                c->st.frames_resorted += 1;
                c->classic_once = true;
            }
            if ((rc = render_again(c, a, 0, &cur))) return rc;
            continue;
        }
        if (!slot.job.cull) return GSR_OK;
        bool broke = false;
        if ((rc = frame_verdict(c, slot, &broke))) return rc;
        if (!broke) {
            c->cull_pol.on_frame_held();
#ifdef GSR_HOST_TIMING
            g_t_verdict = now_us();
#endif
            return GSR_OK;
        }
        c->st.frames_repaired += 1;
        if (slot.dbg_viol) {
            uint32_t hv[80];
            (void)hipStreamSynchronize(slot.stream);
            if (hipMemcpy(hv, slot.dbg_viol, sizeof hv, hipMemcpyDeviceToHost) == hipSuccess) {
                fprintf(stderr, "[viol] frame %llu: %u tile(s) broke their promise\n", (unsigned long long)c->frame_no, hv[0]);
                for (uint32_t k = 0; k < std::min(hv[0], 8u); ++k) {
                    const uint32_t* o = hv + 1 + 8 * k;
                    float hold, kl; std::memcpy(&hold, o + 4, 4); std::memcpy(&kl, o + 5, 4);
                    fprintf(stderr, "   tile (%u, %u): w.w %#x (opaque %u, met %u, u_all %u, steps all %u / u %u) entries read %u, checked depth %u, hold %.4f, last key %.4f, predicted classic %u, kept %u, c1 %u, classic now %u\n",
                            o[0], o[1], o[2], o[2] & 1u, (o[2] >> 14) & 1u, (o[2] >> 15) & 1u, (o[2] >> 16) & 0xffu, o[2] >> 24, o[3], o[7], std::sqrt(hold), std::sqrt(kl), o[6] & 1u, (o[6] >> 1) & 1u, (o[6] >> 2) & 1u, (o[6] >> 3) & 1u);
                }
            }
        }
        // The view is changing faster than the horizons follow.  First answer: compare rects with the horizons of a wider
        // neighbourhood from now on (the repaired frame leaves fresh horizons, and the radius shrinks back while frames hold);
        // only when that is exhausted, leave culling alone for a while (8, 32, 128, 512, 1024 frames).
        c->cull_pol.on_horizon_broke();
        if ((rc = render_again(c, a, 0, &cur))) return rc;
    }
    return set_err(GSR_E_HIP, "gsr_render: the frame did not settle after eight attempts");
}

static bool target_aligned(const gsr_context* c, const void* p) { return (uintptr_t)p % (uintptr_t)gsr_format_pixel_bytes(c->target_format) == 0; }

static int render_frame(gsr_context* c, const FrameArgs& a);

extern "C" int gsr_render(gsr_context* c, const gsr_camera* cam, float* rgba_out, int out_is_device)
{
    return gsr_render_depth(c, cam, nullptr, 0, rgba_out, out_is_device);
}

extern "C" int gsr_render_depth(gsr_context* c, const gsr_camera* cam, const float* depth, int depth_is_device,
                                float* rgba_out, int out_is_device)
{
    return gsr_render_aov(c, cam, depth, depth_is_device, rgba_out, out_is_device, 0, nullptr);
}

// gsr_render_depth + one AOV plane beside the image (aov = 0 or aov_out = NULL: gsr_render_depth itself)
extern "C" int gsr_render_aov(gsr_context* c, const gsr_camera* cam, const float* depth, int depth_is_device,
                              float* rgba_out, int out_is_device, int aov, float* aov_out)
{
    if (!c || !cam || !rgba_out) return set_err(GSR_E_INVALID, "gsr_render: NULL argument");
    if (out_is_device && !target_aligned(c, rgba_out)) return set_err(GSR_E_INVALID, "gsr_render: the device target is not aligned to its %d-byte pixel", gsr_format_pixel_bytes(c->target_format));
    if (aov != 0 && aov != GSR_AOV_DEPTH) return set_err(GSR_E_INVALID, "gsr_render_aov: unknown AOV %d", aov);
    if (aov_out == nullptr) aov = 0;
    if (aov && out_is_device && (uintptr_t)aov_out % 8u != 0) return set_err(GSR_E_INVALID, "gsr_render_aov: the device plane is not aligned to its 8-byte pixel");
    return render_frame(c, FrameArgs{*cam, depth, depth_is_device != 0, rgba_out, out_is_device != 0, aov, aov ? aov_out : nullptr});
}

// one frame from begin to hand-over (gsr_render_aov, gsr_render_over)
static int render_frame(gsr_context* c, const FrameArgs& a)
{
    FrameSlot* sl = nullptr;
    if (c->band_tile_rows == 0) return GSR_OK;   // (gsr_set_row_band: a rank that owns nothing -- no frame, nothing written)
#ifdef GSR_HOST_PHASES
    static double acc[4] = {0, 0, 0, 0}, t_last_exit = 0; static long cnt = 0;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
#endif
    int rc = frame_begin(c, a, &sl, true);
    if (rc) return rc;
    if (sl->job.deferred) return GSR_OK;   // GSR_OPT_DEFERRED_CHECK: the pair count is looked at by the next call that syncs
#ifdef GSR_HOST_PHASES
    const double t1 = now();
#endif
    if ((rc = frame_finish(c, *sl))) return rc;
#ifdef GSR_HOST_PHASES
    const double t2 = now();
#endif
    rc = frame_check(c, *sl, a);
#ifdef GSR_HOST_PHASES
    const double t3 = now();
    acc[0] += t1 - t0; acc[1] += t2 - t1; acc[2] += t3 - t2; if (t_last_exit > 0) acc[3] += t0 - t_last_exit;
    t_last_exit = t3;
    if (++cnt % 50 == 0) { fprintf(stderr, "[host phases] begin %.1f  finish(pair wait + frame end) %.1f  check(verdict wait) %.1f  outside gsr_render %.1f us\n", acc[0] / 50, acc[1] / 50, acc[2] / 50, acc[3] / 50); acc[0] = acc[1] = acc[2] = acc[3] = 0; }
#endif
    return rc;
}

// ---- background (gsr_device.h: gsr_composite_over_pixel) ----
static const char* background_error(const gsr_background* bg)
{
    if (bg->kind != GSR_BG_COLOUR && bg->kind != GSR_BG_IMAGE) return "unknown background kind";
    if (bg->kind == GSR_BG_IMAGE) {
        if (!gsr_format_pixel_bytes(bg->format)) return "unknown image format";
        if (!bg->image) return "the image is NULL";
    }
    return nullptr;
}

// gsr_render_depth over a background (bg = NULL or kind 0: gsr_render_depth itself, the same launches)
extern "C" int gsr_render_over(gsr_context* c, const gsr_camera* cam, const float* depth, int depth_is_device,
                               const gsr_background* bg, float* rgba_out, int out_is_device)
{
    if (!bg || bg->kind == 0) return gsr_render_depth(c, cam, depth, depth_is_device, rgba_out, out_is_device);
    if (!c || !cam || !rgba_out) return set_err(GSR_E_INVALID, "gsr_render_over: NULL argument");
    if (out_is_device && !target_aligned(c, rgba_out)) return set_err(GSR_E_INVALID, "gsr_render_over: the device target is not aligned to its %d-byte pixel", gsr_format_pixel_bytes(c->target_format));
    if (const char* why = background_error(bg)) return set_err(GSR_E_INVALID, "gsr_render_over: %s", why);
    if (bg->kind == GSR_BG_IMAGE && bg->image_is_device) {
        const size_t ibpp = (size_t)gsr_format_pixel_bytes(bg->format);
        if ((uintptr_t)bg->image % ibpp != 0) return set_err(GSR_E_INVALID, "gsr_render_over: the device image is not aligned to its %d-byte pixel", (int)ibpp);
        if (out_is_device && cam->width > 0 && cam->height > 0 && cam->width <= GSR_MAX_DIM && cam->height <= GSR_MAX_DIM) {
            // (no in-place form: an attempt that is composited again -- a repair, a re-queue -- must read the original background)
            const int rows = ctx_band_rows(c, cam->height);
            const uintptr_t i0 = (uintptr_t)bg->image, i1 = i0 + (size_t)cam->width * cam->height * ibpp;
            const uintptr_t o0 = (uintptr_t)rgba_out, o1 = o0 + (size_t)cam->width * rows * (size_t)gsr_format_pixel_bytes(c->target_format);
            if (i0 < o1 && o0 < i1) return set_err(GSR_E_INVALID, "gsr_render_over: the device image overlaps the device target (there is no in-place form)");
        }
    }
    FrameArgs a{*cam, depth, depth_is_device != 0, rgba_out, out_is_device != 0, 0, nullptr};
    a.bg = *bg;
    return render_frame(c, a);
}

// the rule on the host, through the same functions as the kernel's epilogue: no context, no GPU
extern "C" int gsr_composite_over(const float* rgba32f, int64_t n_pixels, const gsr_background* bg, int out_format, void* out)
{
    if (!gsr_format_pixel_bytes(out_format)) return set_err(GSR_E_INVALID, "gsr_composite_over: unknown output format %d", out_format);
    if (!bg || n_pixels < 0 || (n_pixels > 0 && (!rgba32f || !out))) return set_err(GSR_E_INVALID, "gsr_composite_over: bad argument");
    if (const char* why = background_error(bg)) return set_err(GSR_E_INVALID, "gsr_composite_over: %s", why);
    if (bg->kind == GSR_BG_IMAGE && bg->image_is_device) return set_err(GSR_E_INVALID, "gsr_composite_over: the image must be in host memory");
    for (int64_t i = 0; i < n_pixels; ++i) {
        const float4 S = make_float4(rgba32f[4 * i], rgba32f[4 * i + 1], rgba32f[4 * i + 2], rgba32f[4 * i + 3]);
        const float4 B = bg->kind == GSR_BG_IMAGE ? gsr_background_pixel(bg->image, bg->format, (size_t)i)
                                                  : make_float4(bg->rgba[0], bg->rgba[1], bg->rgba[2], bg->rgba[3]);
        const float4 o = gsr_composite_over_pixel(S, B);
        if (out_format == GSR_TARGET_RGBA32F) {
            const float v[4] = {o.x, o.y, o.z, o.w};
            std::memcpy(static_cast<char*>(out) + 16 * i, v, 16);
        } else if (out_format == GSR_TARGET_RGBA16F) {
            const uint2 v = gsr_pack_rgba16f(o.x, o.y, o.z, o.w);
            std::memcpy(static_cast<char*>(out) + 8 * i, &v, 8);
        } else {
            const uint32_t v = gsr_pack_rgba8(o.x, o.y, o.z, o.w);
            std::memcpy(static_cast<char*>(out) + 4 * i, &v, 4);
        }
    }
    return GSR_OK;
}

// ---- depth AOV -> window depth (gsr_device.h: gsr_resolve_depth_pixel) ----
extern "C" int gsr_resolve_depth(const float* aov, int64_t n_pixels, float cov_min, float* depth_out)
{
    if (n_pixels < 0 || !aov || !depth_out) return set_err(GSR_E_INVALID, "gsr_resolve_depth: bad argument");
    for (int64_t i = 0; i < n_pixels; ++i) depth_out[i] = gsr_resolve_depth_pixel(aov[2 * i], aov[2 * i + 1], cov_min);
    return GSR_OK;
}

__global__ void __launch_bounds__(256)
k_resolve_depth(const float2* __restrict__ aov, int64_t n, float cov_min, float* __restrict__ depth_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const float2 v = aov[i]; depth_out[i] = gsr_resolve_depth_pixel(v.x, v.y, cov_min); }
}

extern "C" int gsr_resolve_depth_device(gsr_context* c, const float* aov, int64_t n_pixels, float cov_min, float* depth_out)
{
    if (!c || n_pixels < 0 || !aov || !depth_out) return set_err(GSR_E_INVALID, "gsr_resolve_depth_device: bad argument");
    if ((uintptr_t)aov % 8u != 0) return set_err(GSR_E_INVALID, "gsr_resolve_depth_device: the plane is not aligned to its 8-byte pixel");
    if (n_pixels > (int64_t)GSR_MAX_DIM * GSR_MAX_DIM) return set_err(GSR_E_INVALID, "gsr_resolve_depth_device: more pixels than the largest frame");
    if (n_pixels == 0) return GSR_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_resolve_depth, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, c->stream, reinterpret_cast<const float2*>(aov), n_pixels, cov_min, depth_out);
    HIP_TRY(hipGetLastError());
    return GSR_OK;
}

// split form for callers that drive several contexts from one thread (gsr_multi.cpp)
__attribute__((visibility("hidden"))) int gsr_internal_frame_begin(gsr_context* c, const gsr_camera* cam, const float* depth,
                                                                    int depth_is_device, float* out_dev)
{
    if (!c || !cam || !out_dev) return set_err(GSR_E_INVALID, "gsr_render: NULL argument");
    if (!target_aligned(c, out_dev)) return set_err(GSR_E_INVALID, "gsr_render: the device target is not aligned to its %d-byte pixel", gsr_format_pixel_bytes(c->target_format));
    if (c->band_tile_rows == 0) return GSR_OK;   // (an empty explicit band: no frame)
    return frame_begin(c, FrameArgs{*cam, depth, depth_is_device != 0, out_dev, true}, nullptr, true);
}
__attribute__((visibility("hidden"))) int gsr_internal_frame_finish(gsr_context* c) { return c ? finish_open_frames(c) : GSR_OK; }
// third step of the split form: the newest frame's occlusion-culling verdict (and the repair, if it broke a horizon)
__attribute__((visibility("hidden"))) int gsr_internal_frame_check(gsr_context* c, const gsr_camera* cam, const float* depth,
                                                                    int depth_is_device, float* out_dev)
{
    FrameSlot* sl = c ? latest_slot(c) : nullptr;
    if (!sl || c->band_tile_rows == 0) return GSR_OK;
    if (!cam || !out_dev) return set_err(GSR_E_INVALID, "gsr_render: NULL argument");
    return frame_check(c, *sl, FrameArgs{*cam, depth, depth_is_device != 0, out_dev, true});
}
__attribute__((visibility("hidden"))) void* gsr_internal_stream(gsr_context* c) { return c ? (void*)c->stream : nullptr; }
__attribute__((visibility("hidden"))) int gsr_internal_device(gsr_context* c) { return c ? c->device : -1; }

// Wireframe overlay: synchronous, not on the per-frame beauty path.
static int render_wire(gsr_context* c, const gsr_camera* cam, float* rgba_out, int out_is_device, int over);
extern "C" int gsr_render_wire(gsr_context* c, const gsr_camera* cam, float* rgba_out, int out_is_device) { return render_wire(c, cam, rgba_out, out_is_device, 0); }
// wire-over display (the reference draws the outlines AND keeps the primitive in the splat pass, src/GR_GSplat.C:471-486): the outlines
// go on top of the frame that is already in rgba_inout; pixels no outline covers are left as they are
extern "C" int gsr_render_wire_over(gsr_context* c, const gsr_camera* cam, float* rgba_inout, int is_device) { return render_wire(c, cam, rgba_inout, is_device, 1); }
// (gsr_render_marks, the selection overlay, shares this z-buffer and staging image; its body is at the end of the file, behind the
// mask intake and the pointer check it takes from the resident edits)
static int render_wire(gsr_context* c, const gsr_camera* cam, float* rgba_out, int out_is_device, int over)
{
    if (!c || !cam || !rgba_out) return set_err(GSR_E_INVALID, "gsr_render_wire: NULL argument");
    if (c->uploading) return set_err(GSR_E_INVALID, "gsr_render_wire: upload in progress");
    if (cam->width <= 0 || cam->height <= 0 || cam->width > GSR_MAX_DIM || cam->height > GSR_MAX_DIM)
        return set_err(GSR_E_INVALID, "gsr_render_wire: bad framebuffer size %dx%d", cam->width, cam->height);
    if (!c->has_geometry) return set_err(GSR_E_NO_GEOMETRY, "gsr_render_wire: nothing uploaded");
    if (out_is_device && !target_aligned(c, rgba_out)) return set_err(GSR_E_INVALID, "gsr_render_wire: the device target is not aligned to its %d-byte pixel", gsr_format_pixel_bytes(c->target_format));
    const size_t bpp = (size_t)gsr_format_pixel_bytes(c->target_format);
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    hipStream_t s = c->slot[0].own;
    GsrFrame f;
    build_frame(c, cam, &f);
    const size_t npix = (size_t)cam->width * cam->height;
    // the z-buffer (and the staging image for a host target) are kept between calls: an overlay redraw allocates nothing
    if ((rc = c->wire.ensure(npix))) return rc;
    // outlines at the same depth are drawn in UPLOAD order (k_wire.h): with spatially ordered storage the resolve pass goes back
    // from the winner's upload index to its slot through the inverse of the storage permutation, built once per geometry (gsr_update shares it)
    if ((rc = ensure_inverse_perm(c))) return rc;
    const uint32_t* const inv = (c->perm && c->n > 0) ? c->wire_inv : (const uint32_t*)nullptr;
    unsigned long long* zbuf = c->wire.zbuf;
    float* target = out_is_device ? rgba_out : c->wire.out;
    hipError_t e = hipMemsetAsync(zbuf, 0xff, npix * 8, s);
    if (e == hipSuccess && over && !out_is_device) e = hipMemcpyAsync(c->wire.out, rgba_out, npix * bpp, hipMemcpyHostToDevice, s);   // (the frame underneath)
    if (e == hipSuccess && c->n > 0)
        hipLaunchKernelGGL(k_wire_splats, dim3(div_up(c->n, 256)), dim3(256), 0, s, c->n, f, c->geoA, c->geoB, zbuf, inv ? c->perm : (const uint32_t*)nullptr);
    if (e == hipSuccess)
        hipLaunchKernelGGL(k_wire_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, zbuf, npix, c->col,
                           target, c->target_format, inv, over);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !out_is_device) e = hipMemcpyAsync(rgba_out, c->wire.out, npix * bpp, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_render_wire: %s", hipGetErrorString(e));
    return GSR_OK;
}

// test door of the policies (gsr_policy.h): a pure function (state, event, a, b) -> state; needs no context and no GPU
extern "C" int gsr_debug_policy(int32_t* state16, int event, long long a, long long b)
{
    if (!state16) return set_err(GSR_E_INVALID, "gsr_debug_policy: NULL state");
    gsr_policy_apply(state16, event, a, b);
    return state16[11] < 0 ? set_err(GSR_E_INVALID, "gsr_debug_policy: unknown event %d", event) : GSR_OK;
}
// test door of the frame driver's decisions (gsr_frame_plan.h: the flat layouts): which = 0 the plan of a frame, 1 the outcome of an attempt
extern "C" int gsr_debug_frame_plan(int which, const int32_t* in, int32_t* policy16, int32_t* out)
{
    if (!in || !out || (which == 0 && !policy16)) return set_err(GSR_E_INVALID, "gsr_debug_frame_plan: NULL argument");
    return gsr_frame_plan_apply(which, in, policy16, out) ? set_err(GSR_E_INVALID, "gsr_debug_frame_plan: unknown selector %d", which) : GSR_OK;
}
// ... and the live policy state of a context, in the same layout ([12] = frames the slot's local-sort policy is for: slot 0)
extern "C" int gsr_debug_policy_state(gsr_context* c, int32_t* state16)
{
    if (!c || !state16) return set_err(GSR_E_INVALID, "gsr_debug_policy_state: NULL argument");
    const GsrCullPolicy& p = c->cull_pol;
    const int32_t v[GSR_POLICY_STATE_INTS] = {p.pays, p.weak, (int32_t)p.vis_unculled, p.holdoff, p.backoff, p.streak, p.dilate, p.opt_dilate,
                                              c->slab_pol.holdoff, c->slot[0].local_pol.fails, c->slot[0].local_pol.holdoff, 0, 0, 0, 0, 0};
    std::memcpy(state16, v, sizeof v);
    return GSR_OK;
}

extern "C" int gsr_synchronize(gsr_context* c)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_synchronize: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    return rc ? rc : gsr_internal_comm_sync(c);   // (... and the gather in flight, if the context has a communicator)
}

// the frame summaries live in device memory (no PCIe writes on the per-frame path); callers have synchronised
static void fetch_counters(gsr_context* c)
{
    for (int k = 0; k < GSR_MAX_SLOTS; ++k)
        if (c->slot[k].d_frame && c->slot[k].h_counters)
            (void)hipMemcpy(c->slot[k].h_counters, c->slot[k].d_frame, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}

// the slot that rendered the most recent frame (NULL before the first frame)
static FrameSlot* latest_slot(gsr_context* c)
{
    FrameSlot* best = nullptr;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k)
        if (c->slot[k].frame_id && (!best || c->slot[k].frame_id > best->frame_id)) best = &c->slot[k];
    return best;
}

extern "C" int gsr_get_stats(gsr_context* c, gsr_stats* out)
{
    if (!c || !out) return set_err(GSR_E_INVALID, "gsr_get_stats: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    fetch_counters(c);
    // harvest in submission order so that "last frame" fields end up describing the newest frame
    FrameSlot* last = latest_slot(c);
    for (int k = 0; k < GSR_MAX_SLOTS; ++k)
        if (&c->slot[k] != last) harvest_slot(c, c->slot[k]);
    if (last) {
        harvest_slot(c, *last);
        FrameSlot& sl = *last;
        c->st.n_visible = (int64_t)(sl.h_counters[6] & 0xffffffffull);
        c->st.lazy_redo_tiles = sl.last_lazy ? (int64_t)(sl.h_counters[7] & 0xffffffffull) : 0;
        c->st.pairs_consumed = (int64_t)sl.h_counters[1];
        c->st.entries_scanned = (int64_t)sl.h_counters[3];
        c->st.pairs_total = sl.last_pairs;
        c->st.clusters_total = c->nclus;
        c->st.clusters_kept = sl.hints.surv_hint;
        c->st.policy_bits = (c->lazy_pays ? 1 : 0) | (c->order_pays ? 2 : 0) | (c->cull_pol.pays ? 4 : 0) | (c->cull_pol.weak ? 8 : 0) | (c->prefix_cheaper ? 16 : 0) | (c->depth_active ? 32 : 0);
        c->st.cull_dilate = c->cull_pol.dilate;
        c->st.cull_holdoff = c->cull_pol.holdoff;
        c->st.tiles_x = sl.last_tiles_x;
        c->st.tiles_y = sl.last_local_ty;
        c->st.super_tile = sl.super_tile;
        c->st.stiles_x = sl.stiles_x;
        c->st.stiles_y = sl.stiles_y;
        // running totals live per slot
        int64_t rec_tot = 0, ent_tot = 0, ev_tot = 0;
        for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
            if (!c->slot[k].frame_id) continue;
            rec_tot += (int64_t)c->slot[k].h_counters[2];
            ent_tot += (int64_t)c->slot[k].h_counters[4];
            ev_tot += (int64_t)c->slot[k].h_counters[5];
        }
        c->st.blend_pairs_consumed_total = rec_tot;
        c->st.blend_entries_scanned_total = ent_tot;
        c->st.blend_wave_evals_total = ev_tot;
        {   // colours evaluated ahead of time (device-side running counters, one per slot)
            unsigned long long tot = 0, v = 0;
            for (int k = 0; k < GSR_MAX_SLOTS; ++k)
                if (c->slot[k].lazy_ctr && hipMemcpy(&v, c->slot[k].lazy_ctr + 1, 8, hipMemcpyDeviceToHost) == hipSuccess) tot += v;
            c->st.lazy_colours_total = (int64_t)tot - c->lazy_base;
        }
    }
    *out = c->st;
    return GSR_OK;
}

// the newest complete set of row sums among the slots' mailboxes (no synchronisation: a set that is being written, or torn, is skipped).
// A slot's words belong to its last frame when they carry the ticket of the slot's last attempt (rows_ticket == ticket).  -> 0, or 1: none
static int peek_row_work(gsr_context* c, uint32_t* out, int n_rows, int64_t* frame_out)
{
    int order[GSR_MAX_SLOTS];
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) order[k] = k;
    std::sort(order, order + GSR_MAX_SLOTS, [&](int a, int b) { return c->slot[a].frame_id > c->slot[b].frame_id; });
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
        const FrameSlot& sl = c->slot[order[k]];
        if (!sl.h_rows || !sl.frame_id || !sl.rows_ticket || sl.rows_ticket != sl.ticket || sl.rows_tiles_y != n_rows) continue;
        const volatile unsigned long long* box = sl.h_rows;
        bool whole = true;
        for (int r = 0; r < n_rows && whole; ++r) {
            const unsigned long long v = box[r];
            whole = (uint32_t)(v >> 32) == sl.rows_ticket;
            out[r] = (uint32_t)v;
        }
        if (!whole) continue;
        if (frame_out) *frame_out = (int64_t)sl.frame_id;
        return 0;
    }
    return 1;
}
// gsr_multi's balancer: whatever set is complete now, without a wait (1: none)
__attribute__((visibility("hidden"))) int gsr_internal_peek_row_work(gsr_context* c, uint32_t* out, int n_rows, int64_t* frame_out)
{
    if (!c || !out || !c->opt_row_work || n_rows < 1 || n_rows > GSR_MAX_TILES_SIDE) return 1;
    return peek_row_work(c, out, n_rows, frame_out);
}

extern "C" int gsr_read_row_work(gsr_context* c, uint32_t* out, int n_rows, int64_t* frame_out)
{
    if (!c || !out) return set_err(GSR_E_INVALID, "gsr_read_row_work: NULL argument");
    if (!c->opt_row_work) return set_err(GSR_E_INVALID, "gsr_read_row_work: GSR_OPT_ROW_WORK is off");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    FrameSlot* sl = latest_slot(c);
    if (!sl || !sl->rows_ticket) return set_err(GSR_E_INVALID, "gsr_read_row_work: no frame has run with GSR_OPT_ROW_WORK on");
    if (n_rows != sl->rows_tiles_y) return set_err(GSR_E_INVALID, "gsr_read_row_work: expected %d tile rows", sl->rows_tiles_y);
    if (peek_row_work(c, out, n_rows, frame_out)) return set_err(GSR_E_HIP, "gsr_read_row_work: the frame finished without delivering its row sums");
    return GSR_OK;
}

extern "C" int gsr_stats_reset(gsr_context* c)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_stats_reset: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) {
        harvest_slot(c, c->slot[k]);
        HIP_TRY(hipMemset(c->slot[k].counters, 0, 8 * sizeof(unsigned long long)));
        for (int j = 0; j < 8; ++j) c->slot[k].h_counters[j] = 0;
        HIP_TRY(hipMemset(c->slot[k].d_frame, 0, 8 * sizeof(unsigned long long)));
    }
    const int64_t ns = c->st.n_splats;
    {
        unsigned long long tot = 0, v = 0;
        for (int k = 0; k < GSR_MAX_SLOTS; ++k)
            if (c->slot[k].lazy_ctr && hipMemcpy(&v, c->slot[k].lazy_ctr + 1, 8, hipMemcpyDeviceToHost) == hipSuccess) tot += v;
        c->lazy_base = (int64_t)tot;
    }
    const int64_t ups = c->st.uploads, mvs = c->st.moves;
    double upm[6], mvm[4];
    std::memcpy(upm, c->st.upload_ms, sizeof upm);      // (the last upload's figures describe the resident cloud: they outlive a reset)
    std::memcpy(mvm, c->st.move_ms, sizeof mvm);        // (... and so do the moves': both are treated alike)
    c->st = gsr_stats{};
    c->st.uploads = ups; c->st.moves = mvs;
    std::memcpy(c->st.upload_ms, upm, sizeof upm);
    std::memcpy(c->st.move_ms, mvm, sizeof mvm);
    c->st.n_splats = ns;
    c->st.record_bytes = (int32_t)sizeof(GsrRecord);
    c->st.pair_bytes = 8;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// debug / test access: intermediates of the most recent frame, the pipeline's sorts on a test's arrays (HERE: it places two kernel templates)
#include "gsr_debug_read.h"

// ---------------------------------------------------------------------------
// Edits of the resident cloud without a re-upload: update, move, the device sources, visibility, remove, add.
// (Behind everything else: the kernel templates they launch first keep their places at the end of the code object.)
#include "gsr_resident_edit.h"
// ... and read back in upload order: it shares the edits' refusals and pointer check, and k_unpack comes last of all.
#include "gsr_resident_read.h"
// ... and selected by screen region: read's contract, and k_select behind k_unpack; by attribute (3.14) and by
// density (3.17) and by connectivity (3.18): the two verbs of the four that borrow the upload sort's scratch and wait for the frames
// in flight.
#include "gsr_resident_select.h"
// ... and measured: select's contract; k_measure and k_measure_fold behind k_select_attrs.
#include "gsr_resident_measure.h"

// ---------------------------------------------------------------------------
// Selection overlay (k_marks.h): the splats a mask selects drawn into a finished frame.  render_wire(over = 1)'s
// shape -- the same z-buffer, the same staging image for a host target, the same waits -- with gsr_select's intake in front of it:
// the mask through MaskArg, every device pointer through check_device_source before anything is launched, what comes from host
// memory copied when the call is made.  Writes nothing the context keeps but its own tally.
static_assert(GSR_MARK_DOT == GSR_MARKK_DOT && GSR_MARK_OUTLINE == GSR_MARKK_OUTLINE && GSR_MARK_COLOUR_FIXED == GSR_MARKC_FIXED &&
              GSR_MARK_COLOUR_CD == GSR_MARKC_CD && GSR_MARK_ANY_OPACITY == GSR_SELF_ANY_OPACITY, "the header's shapes, colour modes and flags are the kernels'");

// what is wrong with the caller's camera or style (NULL: nothing)
static const char* mark_style_error(const gsr_camera* cam, const gsr_mark_style* s)
{
    if (cam->width < 1 || cam->height < 1 || cam->width > GSR_MAX_DIM || cam->height > GSR_MAX_DIM) return "width or height is not within 1..GSR_MAX_DIM";
    if (s->shape != GSR_MARK_DOT && s->shape != GSR_MARK_OUTLINE) return "unknown shape";
    if (s->radius < 0 || s->radius > (s->shape == GSR_MARK_DOT ? GSR_MARK_MAX_RADIUS : 0)) return "radius is not within 0..8 (DOT) or not 0 (OUTLINE)";
    if (s->colour_mode != GSR_MARK_COLOUR_FIXED && s->colour_mode != GSR_MARK_COLOUR_CD) return "unknown colour mode";
    if (s->flags & ~GSR_MARK_ANY_OPACITY) return "unknown flag bits";
    if (s->reserved_ != 0) return "reserved_ is not 0";
    if (s->colour_mode == GSR_MARK_COLOUR_FIXED) {
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(s->rgba[k])) return "rgba is not finite";
        if (!(s->rgba[3] >= 0.0f && s->rgba[3] <= 1.0f)) return "the colour's alpha is not within [0, 1]";
    }
    return nullptr;
}

extern "C" int gsr_get_marks(gsr_context* c, int64_t* calls, int64_t* pixels_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_marks: ctx is NULL");
    return c->marks.report(calls, pixels_last, ms);
}

extern "C" int gsr_render_marks(gsr_context* c, const gsr_camera* cam, const uint32_t* mask, int mask_is_device, const gsr_mark_style* st,
                                void* rgba_inout, int is_device, int64_t* n_pixels)
{
    const char* const who = "gsr_render_marks";
    if (!c || !cam || !st || !rgba_inout) return set_err(GSR_E_INVALID, "gsr_render_marks: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const char* bad = mark_style_error(cam, st);
    if (bad) return set_err(GSR_E_INVALID, "gsr_render_marks: %s", bad);
    if (is_device && !target_aligned(c, rgba_inout))
        return set_err(GSR_E_INVALID, "gsr_render_marks: the device target is not aligned to its %d-byte pixel", gsr_format_pixel_bytes(c->target_format));
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask exists, and nothing is drawn
        if (n_pixels) *n_pixels = 0;
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)cam->width * (size_t)cam->height, bpp = (size_t)gsr_format_pixel_bytes(c->target_format);
    const MaskArg mk{mask, mask_is_device != 0, n};
    const bool depth_host = st->depth && !st->depth_is_device;
    // every device pointer, with its exact size, before anything is launched: a wrong pointer must never be found out by a kernel
    if ((rc = mk.check(c, who))) return rc;
    if (st->depth && st->depth_is_device && (rc = check_device_source(c, st->depth, npix * 4, who, "depth"))) return rc;
    if (is_device && (rc = check_device_source(c, rgba_inout, npix * bpp, who, "the target"))) return rc;
    // the frames in flight (the frame underneath may be one of them) and the public stream (whoever produced a device source there)
    if ((rc = sync_all(c))) return rc;
    // ---- everything the call needs, before the first launch: a host mask and a host depth buffer are staged in the arena
    const size_t oDepth = pad256(mk.stage_bytes());
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    if ((rc = ensure_stage(c, oDepth + (depth_host ? npix * 4 : 0))) || (rc = c->wire.ensure(npix)) || (rc = ensure_inverse_perm(c)) ||
        (rc = ensure_up_events(c, 3, who, true)) || (rc = ensure_sel_counters(c, who)))
        return rc;
    hipStream_t s = c->slot[0].own;
    double copy_ms = 0.0;
    const uint32_t* dmask = nullptr;
    const float* ddepth = st->depth;
    void* const target = is_device ? rgba_inout : (void*)(float*)c->wire.out;
    hipError_t e = mk.to_device(c, s, 0, &copy_ms, &dmask);
    if (e == hipSuccess && (depth_host || !is_device)) {
        const double t0 = up_now_ms();
        if (depth_host) {
            float* d = reinterpret_cast<float*>(c->stage + oDepth);
            e = hipMemcpyAsync(d, st->depth, npix * 4, hipMemcpyHostToDevice, s);
            ddepth = d;
        }
        if (e == hipSuccess && !is_device) e = hipMemcpyAsync(target, rgba_inout, npix * bpp, hipMemcpyHostToDevice, s);   // (the frame underneath)
        if (e == hipSuccess) e = hipStreamSynchronize(s);                      // the caller's depth buffer may be freed on return
        copy_ms += up_now_ms() - t0;
    }
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_render_marks: %s", hipGetErrorString(e));
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    unsigned long long* const zbuf = c->wire.zbuf;
    const int any = (st->flags & GSR_MARK_ANY_OPACITY) ? 1 : 0;
    e = hipMemsetAsync(c->sel_counters, 0, cwords * 8, s);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[0], s);
    if (e == hipSuccess) e = hipMemsetAsync(zbuf, 0xff, npix * 8, s);          // GSR_WIRE_EMPTY, per call
    if (e == hipSuccess) {
        const dim3 grid(div_up(n, GSR_MARK_THREADS)), block(GSR_MARK_THREADS);
        if (st->shape == GSR_MARK_DOT) {
            gsr_select_region everywhere{};
            everywhere.x0 = everywhere.y0 = -INFINITY;
            everywhere.x1 = everywhere.y1 = INFINITY;
            everywhere.flags = any ? GSR_SELECT_ANY_OPACITY : 0;
            const GsrSelectRule rule = select_rule(cam, c->origin, &everywhere);
            hipLaunchKernelGGL(k_mark<GSR_MARKK_DOT>, grid, block, 0, s, n, dmask, inv, c->geoA, c->geoB, rule, any, (int)st->radius, zbuf);
        } else {
            GsrFrame f;
            build_frame(c, cam, &f);
            hipLaunchKernelGGL(k_mark<GSR_MARKK_OUTLINE>, grid, block, 0, s, n, dmask, inv, c->geoA, c->geoB, f, any, 0, zbuf);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_mark_resolve, dim3((unsigned)((npix + GSR_MARK_THREADS - 1) / GSR_MARK_THREADS)), dim3(GSR_MARK_THREADS), 0, s, zbuf, npix,
                           c->col, inv, (int)st->colour_mode, make_float4(st->rgba[0], st->rgba[1], st->rgba[2], st->rgba[3]), ddepth,
                           st->depth_bias, target, c->target_format, c->sel_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->sel_h_counters, c->sel_counters, cwords * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !is_device) e = hipMemcpyAsync(rgba_inout, target, npix * bpp, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_render_marks: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    unsigned long long wrote = 0, unused = 0;
    sum_sel_counters(c, &wrote, &unused);
    if (n_pixels) *n_pixels = (int64_t)wrote;
    float ms = 0.0f;
    c->marks.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->marks.ms[1] = hipEventElapsedTime(&ms, c->up_ev[1], c->up_ev[2]) == hipSuccess ? (double)ms : 0.0;
    c->marks.ms[2] = copy_ms;
    c->marks.ms[3] = up_now_ms() - t_begin;
    c->marks.calls += 1;
    c->marks.last = (int64_t)wrote;
    return GSR_OK;
}
