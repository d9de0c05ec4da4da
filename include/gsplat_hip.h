/*
 * gsplat_hip.h -- C ABI of libgsplat_hip.so, the MI355X (gfx950) Gaussian-splat
 * rasterizer that replaces the device half (and the per-camera-move CPU sort)
 * of the reference's GSplatRenderer.  No HDK, GL or torch types cross this
 * boundary: plain pointers, sizes and PODs only.  Every function returns 0 on
 * success or a negative GSR_E_* code and never throws; gsr_last_error() gives
 * the text.  A context is bound to one GPU and is NOT thread-safe (the
 * reference runs everything on Houdini's single draw thread).
 *
 * Reference interfaces replaced (paths relative to /root/reference/gsplat_plugin):
 *   gsr_upload*        <- GSplatRenderer::generateRenderGeometry  src/GSplatRenderer.C:420-532
 *                         (TBB pack into 1 RGBA32F + 2 RGB16F textures, setTexture x3)
 *   gsr_render         <- GSplatRenderer::render                  src/GSplatRenderer.C:534-658
 *                         = argsortByDistance :176-216 (CPU, TBB) + index-texture upload :586-592
 *                         + GL state/uniforms :605-645 + drawInstanced :647, which runs
 *                         shaders/GSplatShaderSource.h:190-288 (VS), :304-312 (FS)
 *                         and the fixed-function blend :613-621
 *   gsr_camera         <- the uniform block of the main program   shaders/GSplatShaderSource.h:119-133,153-159
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK                0
#define GSR_E_INVALID        -1   /* bad argument */
#define GSR_E_HIP            -2   /* a HIP runtime call failed */
#define GSR_E_NO_DEVICE      -3   /* no gfx950 device / device ordinal out of range */
#define GSR_E_NO_GEOMETRY    -4   /* render before any upload */
#define GSR_E_TOO_MANY_PAIRS -5   /* (tile, splat) pair count exceeds GSR_MAX_PAIRS */
#define GSR_E_OOM            -6
#define GSR_E_COMM           -7   /* RCCL could not be loaded, or a communicator call failed */

#define GSR_TILE              16          /* tile edge in pixels */
#define GSR_MAX_DIM           16384       /* max framebuffer width/height (1024 x 1024 tiles) */
#define GSR_MAX_PAIRS         0x7fffff00ll

typedef struct gsr_context gsr_context;

/* Per-frame uniforms.  Field names = the GLSL uniforms of the reference's main
 * program.  Matrices: 16 floats, GL column-major (m[c*4+r]); this is the byte
 * layout of Houdini's UT_Matrix4F::data(), so HDK glue passes them through. */
typedef struct gsr_camera {
    float obj_view[16];    /* glH_ObjViewMatrix    */
    float object[16];      /* glH_ObjectMatrix     */
    float inv_object[16];  /* glH_InvObjectMatrix  */
    float view[16];        /* glH_ViewMatrix       */
    float proj[16];        /* glH_ProjectMatrix    */
    float cam_pos[3];      /* WorldSpaceCameraPos: sort reference point and SH eye
                              (src/GSplatRenderer.C:551-563) */
    int32_t width;         /* glH_ScreenSize.x  (<= GSR_MAX_DIM) */
    int32_t height;        /* glH_ScreenSize.y  (<= GSR_MAX_DIM) */
    int32_t sh_order;      /* GSplatShOrder 0..3; forced to 0 when no SH was uploaded
                              (doSH gate, src/GSplatRenderer.C:623,628) */
} gsr_camera;

/* Counters and timings of the most recent gsr_render plus running totals
 * (totals feed bench.py's roofline: blend_ms_total / blend_launches). */
typedef struct gsr_stats {
    int64_t n_splats;          /* uploaded */
    int64_t n_visible;         /* survived w/z culling and have >=1 tile */
    int64_t pairs_total;       /* D: (super-tile, splat) list entries of the frame */
    int64_t pairs_consumed;    /* records gathered by the blend kernel before early-out */
    int32_t tiles_x, tiles_y;  /* tile grid of this context's shard */
    int32_t record_bytes;      /* bytes of one projected record as gathered by the blend kernel (48) */
    int32_t pair_bytes;        /* bytes of one list entry as scanned by the blend kernel (idx + rect = 8) */
    float ms_preprocess, ms_depth_sort, ms_emit, ms_tile_sort, ms_blend, ms_total; /* last frame, HIP events (timing
                                  level 2; level 1 fills ms_blend only): ms_emit = binning count + scans + pair count
                                  to the host, ms_tile_sort = binning placement */
    double blend_ms_total;     /* sum over all frames since gsr_stats_reset */
    int64_t blend_launches;
    int64_t blend_pairs_consumed_total;
    double frame_ms_total;
    int64_t frames;
    int64_t entries_scanned;               /* list entries (idx+rect) read by the blend kernel, last frame */
    int64_t blend_entries_scanned_total;   /* ... running total */
    int32_t super_tile;                    /* super-tile edge in tiles */
    int32_t stiles_x, stiles_y;            /* super-tile grid (whole image) */
    int32_t reserved_;
    int64_t blend_wave_evals_total;        /* (wave, record) evaluations by the blend kernel = 64 pixel evaluations each, running total */
    double stage_ms_total[5];              /* timing level 2: running totals of ms_preprocess, ms_depth_sort, ms_emit,
                                              ms_tile_sort, ms_blend over stage_frames frames */
    int64_t stage_frames;
    int64_t sorts_skipped;                 /* frames that reused the cached depth order (GSR_OPT_SORT_CACHE) */
    int64_t frames_requeued;               /* frames whose back end ran twice: the pair count outgrew the list buffer */
    int64_t lazy_redo_tiles;               /* lazy colour, last frame: tiles composited by the on-demand fallback */
    int64_t lazy_colours_total;            /* lazy colour: SH evaluations by the ahead-of-time pass, running total */
    int64_t frames_truncated;              /* GSR_OPT_DEFERRED_CHECK only: frames handed over with clamped lists (must stay 0
                                              for exact pixels; the buffer is regrown for the following frames) */
    int64_t frames_culled;                 /* GSR_OPT_OCCLUSION_CULL: frames rendered against the previous frame's depth horizons */
    int64_t frames_repaired;               /* ... of which this many broke a horizon and were rendered again without culling */
    int64_t clusters_total;                /* clusters of 64 storage-ordered splats (k_cluster.h) */
    int64_t clusters_kept;                 /* ... that survived the cluster culling of the last frame whose count reached the host */
    int32_t policy_bits;                   /* what the kernels told the host about the last frames: 1 = lazy colour pays, 2 = a heaviest-first
                                              tile order pays, 4 = occlusion culling has something to work with, 8 = the last culled frame
                                              kept more than 70 % of what an unculled one keeps (culling suspended), 16 = colouring list prefixes is
                                              cheaper than colouring every kept splat */
    int32_t cull_dilate;                   /* occlusion culling: current dilation radius in tiles (GSR_OPT_CULL_DILATE, grown by repairs) */
    int32_t cull_holdoff;                  /* ... frames for which it stays switched off */
    int32_t reserved2_;
    int64_t frames_resorted;               /* GSR_OPT_LOCAL_SORT: frames whose small-frame sort met a bucket far beyond its prediction and were
                                              rendered again with the three global passes */
    int64_t frames_slab;                   /* GSR_OPT_FRONT_SLAB: frames rendered in two phases (front slab, then the rest behind the tiles still open) */
    int64_t frames_jumped;                 /* frames whose camera had jumped since the frame that left the depth horizons: rendered without them (policy mode only) */
    int64_t frames_lazy;                   /* frames whose K1 left the SH colours pending (k_colour.h: list prefixes + on-demand fallback); the others shaded in K1 */
    int64_t uploads;                       /* complete uploads (gsr_upload_end) since gsr_create / gsr_stats_reset */
    double upload_ms[6];                   /* the LAST upload: [0] host -> device copies (wall clock spent inside gsr_upload_append*, quantisation of raw
                                              attributes included), [1] bounding box + Morton codes + their sort (HIP events), [2] k_pack: the arrays into
                                              storage order + cluster bounds (HIP events), [3] wall clock gsr_upload_begin .. gsr_upload_end; the LAST gsr_update: [4] its host ->
                                              device copies (wall clock), [5] its kernels (k_update + the cluster bounds, HIP events); 0 before the first one */
    int64_t moves;                         /* gsr_move calls that moved splats (uploads does not count them); kept by gsr_stats_reset as uploads is */
    double move_ms[4];                     /* the LAST gsr_move: [0] host -> device copies (the P rows, and the arrays of u; wall clock), [1] the new rows into
                                              place + every position in upload order + bounding box + Morton codes + their sort (HIP events), [2] k_repack:
                                              the planes into the new storage order + cluster bounds (HIP events), [3] wall clock of the call */
} gsr_stats;

/* ---- lifetime ----------------------------------------------------------- */
int  gsr_device_count(void);                              /* 0 if no GPU is visible */
int  gsr_create(int device, gsr_context** out);           /* owns a HIP stream on `device` */
void gsr_destroy(gsr_context* ctx);
const char* gsr_last_error(void);                         /* thread-local, never NULL */
const char* gsr_version(void);

/* The context's PUBLIC stream: gsr_render orders its result on it (work queued there afterwards sees
 * the finished frame; the frame's output write waits for work queued there before).  Internally the
 * kernels run on per-frame-slot streams.  Pass a caller-owned hipStream_t (e.g. torch's current
 * stream); NULL restores the context's own stream. */
int  gsr_set_stream(gsr_context* ctx, void* hip_stream);

/* ---- target format ------------------------------------------------------ */
/* What one pixel of every target of the context is: gsr_render* frames, the band images of a sharded context, what
 * gsr_stitch_bands and the gsr_multi / gsr_comm gather move, and the wire overlay.  The f32 pixel is formed exactly as ever; the
 * format only decides how the blend kernel STORES it (no conversion pass runs behind it):
 *   RGBA32F  16 bytes  the f32 pixel itself (default; bit-identical to a context that never heard of formats)
 *   RGBA16F   8 bytes  binary16 of every channel, round to nearest even, overflow to infinity (the rule of gsplat_quantize_half)
 *   RGBA8     4 bytes  c = x clamped to [0, 1] (NaN -> 0); byte = (uint8_t)fmaf(c, 255, 0.5): one rounding, then truncation.
 *                      Linear, premultiplied; no sRGB curve -- that belongs to whoever owns the display transform.
 * A packed target holds the rounded FINAL pixel (the reference's GL blend into such a target rounds after every fragment).
 * NaN: a channel that is NaN in an RGBA32F or RGBA16F target is NaN in gsr_convert_pixels' result and vice versa, with sign and payload
 * unspecified (x86 and gfx950 quiet and propagate NaNs differently); every other channel, infinities and signed zeros included, is
 * bit-exact between the two, and RGBA8 is bit-exact throughout (NaN -> 0).
 * The float* rgba_out parameters below keep their C type and mean "rows*width pixels of the context's target format"; a DEVICE
 * target must be aligned to the pixel size (GSR_E_INVALID otherwise).  This is not a GSR_OPT_* knob: those never change pixels. */
#define GSR_TARGET_RGBA32F    0
#define GSR_TARGET_RGBA16F    1
#define GSR_TARGET_RGBA8      2
int  gsr_target_pixel_bytes(int format);                  /* 16 / 8 / 4, GSR_E_INVALID for anything else; needs no context */
/* Takes effect with the next frame.  Synchronises the context and drops what is laid out for the old pixel size (the staging
 * images of host targets, a front-slab frame's intermediate buffer). */
int  gsr_set_target_format(gsr_context* ctx, int format);
int  gsr_get_target_format(gsr_context* ctx);
/* The same conversion on the host (no context, no GPU): n_pixels RGBA-f32 pixels -> `format`, through the very functions the
 * kernels store with.  For callers who keep f32 frames; also what the tests hold the GPU path to. */
int  gsr_convert_pixels(const float* rgba32f, int64_t n_pixels, int format, void* out);

/* ---- geometry staging (active set changed) ------------------------------ */
/* Arrays are HOST pointers in the reference's registerUpdate() layout
 * (include/GSplatRenderer.h:34-47): P float[3n]; Cd half[3n]; alpha float[n];
 * scale half[3n]; orient half[4n] (x,y,z,w); shx/shy/shz half[16n] (row-major
 * 4x4 per splat, coefficient j at (j/4, j%4)) or all three NULL.  halves are raw
 * binary16 bits.  Data is copied; the caller may free on return.
 * begin/append/end lets the shim concatenate several registry entries without a
 * host-side merge (src/GSplatRenderer.C:420-513). origin = GSplatOrigin. */
int  gsr_upload_begin(gsr_context* ctx, int64_t total_splats, int has_sh, const float origin[3]);
int  gsr_upload_append(gsr_context* ctx, int64_t n,
                       const float* P, const uint16_t* Cd, const float* alpha,
                       const uint16_t* scale, const uint16_t* orient,
                       const uint16_t* shx, const uint16_t* shy, const uint16_t* shz);
/* The same, from RAW float32 point attributes (what a Houdini detail holds): the GPU quantises to fp16 (round to nearest even,
 * overflow to infinity: HDK's fpreal16) and packs -- the work GR_PrimGsplat::update does in a tbb::parallel_for on the CPU
 * (src/GR_GSplat.C:302-372).  NULL Cd / alpha / scale / orient = the reference's defaults (0 / 1 / 1 / (0,0,0,1), :233-272,309-312).
 * SH in any of the three naming schemes (:93-189): sh_scheme 0 = none; 1 = sh_array: sh_vec3_per_point vec3 per point (the first 16
 * are used); 2 = sh_ptr[0..14] = sh1..sh15, float[3n] each; 3 = sh_ptr[0..44] = f_rest_0..44, float[n] each (channel-major: coefficient
 * j = (f_rest_j, f_rest_{j+15}, f_rest_{j+30})).  In schemes 2 and 3 the arrays after the first NULL one count as absent.
 * Attribute precedence (Alpha over opacity), which scheme applies and the gsplat__sh_order rule stay with the caller (GSplatPrim).
 * The SoA left in HBM is bit-identical to gsr_upload_append of the host-quantised arrays. */
typedef struct gsr_raw_attrs {
    const float* P;            /* float[3n], required */
    const float* Cd;           /* float[3n] or NULL */
    const float* alpha;        /* float[n] or NULL */
    const float* scale;        /* float[3n] or NULL */
    const float* orient;       /* float[4n] (x, y, z, w) or NULL */
    int32_t sh_scheme;
    int32_t sh_vec3_per_point;
    const float* sh_array;
    const float* const* sh_ptr;
} gsr_raw_attrs;
int  gsr_upload_append_raw(gsr_context* ctx, int64_t n, const gsr_raw_attrs* attrs);
int  gsr_upload_end(gsr_context* ctx);
/* gives up an upload that failed between begin and end: the context holds no geometry afterwards */
int  gsr_upload_abort(gsr_context* ctx);
/* begin + append + end for a single entry */
int  gsr_upload(gsr_context* ctx, int64_t n,
                const float* P, const uint16_t* Cd, const float* alpha,
                const uint16_t* scale, const uint16_t* orient,
                const uint16_t* shx, const uint16_t* shy, const uint16_t* shz,
                const float origin[3]);

/* ---- attribute update (the resident splats edited in place) --------------- */
/* New values for attributes of splats that are already resident, without a re-upload: what a colour grade, an opacity mask, a
 * rescale or an SH swap costs is the bytes of the arrays given, not the cloud.  Arrays are HOST pointers in the registerUpdate()
 * layout above, holding rows for the splats [first, first + n) only; first counts in UPLOAD order across all the entries that were
 * appended (so a caller who concatenated several entries addresses one of them by the running sum of their sizes).  NULL = that
 * attribute stays as it is.  shx / shy / shz come all three or not at all, and only for a cloud uploaded with SH.
 * There is NO P: a position decides the storage order, the bounding box and the cluster boxes -- moving a point is gsr_move below.
 * float32 sources in DEVICE memory, quantised on the GPU: gsr_update_device below.  Raw float32 HOST sources (gsr_raw_attrs) are
 * not covered: quantise on the host (gsplat_quantize_half), or re-upload.
 * Synchronous like gsr_upload_append (the arrays may be freed on return); it first waits for every frame of the context that is
 * still in flight, so no frame ever reads a half-written splat.
 * CONTRACT: after GSR_OK the resident geometry is bit for bit what a fresh context holds after gsr_upload of the edited arrays
 * (same P, origin, GSR_OPT_STORAGE_ORDER and SH presence), and so is every later frame, in every option mode.
 * GSR_E_INVALID, with the context untouched: NULL ctx or u; no geometry resident; an upload in progress; first < 0, n < 0 or
 * first + n beyond the resident count; one or two of the three SH arrays; SH arrays for a cloud without SH.
 * n == 0, or all seven pointers NULL: GSR_OK, nothing happens.  gsr_stats.uploads does not count updates; upload_ms[4], [5] time the last one. */
typedef struct gsr_attr_update {
    const uint16_t* Cd;               /* half[3n]  */
    const float*    alpha;            /* float[n]  */
    const uint16_t* scale;            /* half[3n]  */
    const uint16_t* orient;           /* half[4n] (x, y, z, w) */
    const uint16_t *shx, *shy, *shz;  /* half[16n] each */
} gsr_attr_update;
int  gsr_update(gsr_context* ctx, int64_t first, int64_t n, const gsr_attr_update* u);

/* ---- position update (resident splats moved, and re-ordered on the GPU) ----- */
/* New positions for the resident splats [first, first + n) (UPLOAD order, as gsr_update counts), and optionally new attributes for the
 * same rows in the same call.  P: float[3n] HOST pointer, required.  origin: float[3] = the new GSplatOrigin, or NULL = it stays.
 * u: as gsr_update takes it (rows for the same range), or NULL.  Synchronous like gsr_update; waits for every frame in flight first.
 * Only P (and the arrays of u) cross the link: 12 bytes per moved splat.  On the device the attributes are applied first (gsr_update
 * as it is), the new rows are written where the splats sit, all positions are put in upload order and go through the ordering of an
 * upload (bounding box, Morton codes, sort), and the resident planes are carried into the new storage order.
 * CONTRACT: after GSR_OK the resident geometry -- geoA, geoB, every colour chunk, the colour rows, the cluster bounds and the storage
 * order -- is bit for bit what a fresh context holds after gsr_upload of the edited arrays (same GSR_OPT_STORAGE_ORDER, same SH
 * presence, the origin now in force), and so is every later frame, in every option mode.  Whatever a frame of the cloud before left
 * (cached orders, horizons, hints, policies) is dropped as an upload drops it.
 * MEMORY: a context that moves splats under GSR_OPT_STORAGE_ORDER = 1 keeps a SECOND copy of the resident planes (the re-ordered
 * planes are written there and the two sets swapped): 16 + 16 + 16 x chunks (+ 128 with SH) bytes per splat of capacity -- about
 * 1.5 GB at 6 M splats with SH -- from the first move until the capacity changes or the context is destroyed.  With
 * GSR_OPT_STORAGE_ORDER = 0 the splats stay where they are; only the cluster bounds are formed again, and there is no second copy.
 * GSR_E_INVALID, with the context untouched: NULL ctx or P; no geometry resident; an upload in progress; a bad range; the gsr_update
 * rules for u.  n == 0: GSR_OK, nothing happens.  Everything is allocated before the first write: GSR_E_OOM leaves the context
 * untouched.  A HIP failure after that leaves NO geometry (gsr_render: GSR_E_NO_GEOMETRY until the next complete upload); with
 * attributes in u that includes ANY HIP failure of the gsr_update step, also one before its own first write.
 * gsr_stats.uploads does not count a move; moves and move_ms[] do.  float32 sources in DEVICE memory: gsr_move_device below.  Not
 * covered: raw float32 HOST sources for u.  A change of the splat count: fewer splats is gsr_remove below, more is gsr_add below. */
int  gsr_move(gsr_context* ctx, int64_t first, int64_t n, const float* P, const float origin[3], const gsr_attr_update* u);

/* ---- device sources (upload, update and move from float32 arrays in DEVICE memory) ------------------------------------------ */
/* For a caller whose splats already live on the GPU of the context, in the same process (a trainer's live view, a deformation
 * network, a simulation, a torch expression): the three verbs above from float32 arrays in device memory.  Nothing crosses the
 * link; Cd, scale, orient and sh are quantised on the GPU by the rule of gsplat_quantize_half (round to nearest even, overflow to
 * infinity), P and alpha stay float32, and SH slot j >= sh_vec3_per_point of a splat's 16 is a zero half.  Activations (0.5 + C0 dc,
 * sigmoid, exp) stay with the caller, as with gsr_raw_attrs.
 * NULL arrays.  gsr_upload_append_device: P is required; the others take the defaults of gsr_upload_append_raw (Cd 0, alpha 1,
 * scale 1, orient (0, 0, 0, 1)); sh is present exactly when the upload announced SH.  gsr_update_device: NULL = the attribute stays;
 * P must be NULL (a position is gsr_move_device); sh only for a cloud with SH.  gsr_move_device: P is required, everything else as
 * for gsr_update_device, applied in the same call; origin as in gsr_move.
 * CONTRACT: that of gsr_update / gsr_move.  After GSR_OK the resident geometry -- geoA, geoB, every colour chunk, the colour rows,
 * the cluster bounds and the storage order -- is bit for bit what a fresh context holds after gsr_upload of the same arrays
 * quantised on the host with gsplat_quantize_half, and so is every later frame, in every option mode; what the frames of the cloud
 * before may keep is decided as the host verbs decide it (a colour-only edit keeps horizons and policies; anything else is a new
 * cloud).  An attribute value that is NaN becomes a NaN half with unspecified sign and payload (the exception of the target
 * formats above); every other value is bit-exact.  Host-source and device-source entries may be mixed inside one gsr_upload_begin /
 * gsr_upload_end.
 * ORDERING: each verb first waits for the work queued on the context's public stream (gsr_set_stream) -- a producer kernel queued
 * there has finished; a producer on any other stream is the caller's to synchronise -- and for the context's frames in flight, as the
 * host verbs do.  The verbs are synchronous: on return the source arrays may be overwritten.
 * SOURCE POINTERS: every non-NULL array is checked before anything is written or launched.  It passes when it is 4-byte aligned,
 * the runtime calls it device memory of the context's device or pinned host memory (hipPointerGetAttributes), and, where the runtime
 * reports the allocation's range (hipMemGetAddressRange), all its bytes lie inside the allocation.  Pageable host memory, another
 * device's memory, managed memory and a range past the allocation's end are GSR_E_INVALID with the context untouched.
 * gsr_debug_check_device_source is that check as a pure query (no kernel, no copy, nothing written): GSR_OK or GSR_E_INVALID.
 * The other refusals are those of the host verbs (NULL ctx or struct, a bad range, an upload in progress or none, no geometry, SH
 * for a cloud without SH), plus P in an update and sh_vec3_per_point outside 1..16.  n == 0, or an update with nothing given:
 * GSR_OK, nothing happens.
 * gsr_stats: upload_ms[4] after gsr_update_device and move_ms[0] after gsr_move_device are 0.0 (nothing crossed the link), and
 * gsr_upload_append_device adds nothing to upload_ms[0]; the kernel and wall-clock entries, moves and uploads are the host verbs'.
 * Out of scope: gsr_multi_* (the cloud is replicated per GPU, a device pointer lives on one of them); the GSplatRenderer shim and
 * the HDK glue (their rows are borrowed host arrays that a re-stage uploads again: a device edit would be lost by it); the SH
 * naming schemes 2 and 3 of gsr_raw_attrs; asynchronous forms; half sources in device memory. */
typedef struct gsr_device_attrs {
    const float* P;        /* float[3n] */
    const float* Cd;       /* float[3n] */
    const float* alpha;    /* float[n]  */
    const float* scale;    /* float[3n] */
    const float* orient;   /* float[4n] (x, y, z, w) */
    const float* sh;       /* float[n * sh_vec3_per_point * 3]: coefficient j of point i at sh[(i * vpp + j) * 3 ..]
                              (gsr_raw_attrs' scheme 1; with vpp = 15 it is a trainer's features_rest (N, 15, 3)) */
    int32_t sh_vec3_per_point;   /* 1..16 when sh is given */
    int32_t reserved_;           /* 0 */
} gsr_device_attrs;
int  gsr_upload_append_device(gsr_context* ctx, int64_t n, const gsr_device_attrs* a);   /* between gsr_upload_begin and _end */
int  gsr_update_device(gsr_context* ctx, int64_t first, int64_t n, const gsr_device_attrs* a);
int  gsr_move_device(gsr_context* ctx, int64_t first, int64_t n, const float origin[3], const gsr_device_attrs* a);
int  gsr_debug_check_device_source(gsr_context* ctx, const void* p, int64_t bytes);

/* ---- visibility (resident splats hidden by crop volumes or a mask, without a re-upload) ---------------------------------------- */
/* Isolating an object, cutting floaters away with a box, hiding a group: the resident splats that fail the rule below get the
 * resident opacity +0.0f -- K1 drops such a splat before its covariance chain and the fragment test discards on the same value, so it
 * contributes nothing, exactly -- and the others keep their own alpha.  Nothing but the struct (and a mask's n / 8 bytes) crosses the
 * link; one streaming kernel evaluates the volumes on the GPU and rewrites the opacities that change.  No frame kernel knows about it,
 * and a context that never calls gsr_set_visibility runs exactly the launches it ran before.
 * THE RULE.  With (x, y, z) = the raw P bits of splat i as uploaded (upload space: before the GSplatOrigin round trip and the object
 * matrix) and m = to_unit of a volume, per axis r
 *     q.r = fmaf(m[4r], x, fmaf(m[4r+1], y, fmaf(m[4r+2], z, m[4r+3])))          (float32, exactly these three fused operations)
 * the splat is INSIDE the volume iff the comparison beside its kind holds (a NaN anywhere: not inside), it PASSES the volume iff
 * inside != invert, and it is VISIBLE iff it passes every volume and its mask bit is clear.  gsr_visibility_eval is this rule on the
 * host (no context, no GPU), through the very function the kernel evaluates: rows [0, n) of P are the splats [first, first + n) as far
 * as the mask is concerned; visible_out[k] = 1 / 0.
 * THE EFFECT, while a visibility is in force: the resident opacity of a hidden splat is +0.0f, that of a visible one its own alpha bit
 * for bit (alphas below 1/255, NaN and -0 included).
 * CONTRACT: after GSR_OK the resident geometry -- geoA, geoB, every colour chunk, the colour rows, the cluster bounds and the storage
 * order -- is bit for bit what a fresh context holds after gsr_upload of the same arrays with alpha[i] replaced by
 * visible(i) ? alpha[i] : +0.0f (same options, origin and SH presence), and so is every later frame, in every option mode, target
 * format, frame verb and band.  NULL, or no volume and no mask, makes everything visible again: the planes of a plain upload, exactly.
 * PERSISTENCE.  The volumes stay in force across gsr_update*, gsr_move* and complete uploads: an alpha update of a hidden splat is
 * remembered and shows when the splat becomes visible, a move evaluates the volumes at the new positions, gsr_upload_end applies them
 * to the new cloud.  The mask belongs to a cloud: it is copied when the call is made, kept by updates and moves, and dropped by every
 * complete upload.  Volumes without a mask may be set before any upload.
 * Synchronous like gsr_update: it first waits for every frame of the context that is still in flight.  What the frames of the cloud
 * may keep afterwards is decided as for an alpha update (horizons, hints and policies go) -- unless no resident bit changed.
 * MEMORY: from the first call the context keeps the true alphas aside, one float per splat of capacity (4 bytes: 24 MB at 6 M
 * splats), and with a mask ceil(n / 32) words, until the capacity changes or the context is destroyed.
 * GSR_E_INVALID, with the context untouched: NULL ctx; n_volumes outside 0..GSR_VIS_MAX_VOLUMES; an unknown kind; invert not 0 or 1;
 * reserved_ not 0; a mask with no geometry resident or with mask_splats != the resident count; an upload in progress.  Non-finite
 * matrix entries are the caller's data and follow the rule.  Everything is allocated before the first write: GSR_E_OOM leaves the
 * resident geometry and the visibility in force untouched (a buffer the call had already allocated by then stays with the context and
 * is used by the next call).  A HIP failure after the first write leaves NO geometry, as gsr_move documents, and no visibility.
 * gsr_get_visibility: the volumes in force (out->mask is always NULL; mask_splats = the splats a mask in force covers, else 0) and
 * how many resident splats the last application hid; either pointer may be NULL.
 * Out of scope: skipping wholly hidden clusters in k_cluster_cull (K1 still loads the 16 bytes of every hidden splat); the wire
 * overlay, which outlines every resident splat as before; a mask in device memory; a mask through the GSplatRenderer shim or the HDK
 * glue; gsr_comm_* (each rank is a plain context and sets its own visibility). */
#define GSR_VIS_MAX_VOLUMES 4
#define GSR_VOL_BOX         1   /* inside iff max(|q.x|, |q.y|, |q.z|) <= 1 */
#define GSR_VOL_ELLIPSOID   2   /* inside iff fmaf(q.x, q.x, fmaf(q.y, q.y, q.z * q.z)) <= 1 */
typedef struct gsr_crop_volume {
    int32_t kind;          /* GSR_VOL_* */
    int32_t invert;        /* 0: the splat passes iff inside; 1: iff NOT inside */
    float   to_unit[12];   /* rows of a 3x4 affine map, to_unit[r*4+c]: upload-space P -> the unit volume */
} gsr_crop_volume;
typedef struct gsr_visibility {
    int32_t n_volumes;     /* 0..GSR_VIS_MAX_VOLUMES; a splat must pass EVERY volume */
    int32_t reserved_;     /* 0 */
    gsr_crop_volume volume[GSR_VIS_MAX_VOLUMES];
    const uint32_t* mask;  /* HOST pointer or NULL: bit (i & 31) of word (i >> 5) set = splat i (UPLOAD order) is hidden */
    int64_t mask_splats;   /* must equal the resident count when mask is given */
} gsr_visibility;
int  gsr_set_visibility(gsr_context* ctx, const gsr_visibility* v);   /* NULL, or no volume and no mask: everything visible again */
int  gsr_get_visibility(gsr_context* ctx, gsr_visibility* out, int64_t* hidden);  /* out->mask is always NULL; either may be NULL */
int  gsr_visibility_eval(const gsr_visibility* v, const float* P, int64_t first, int64_t n, uint8_t* visible_out); /* host, no context, no GPU */

/* ---- removal (resident splats deleted on the GPU, without a re-upload) ---------------------------------------------------------- */
/* A Delete SOP, a trainer's pruning step, "delete what I cropped away": the splats named by a mask leave the resident cloud and the
 * survivors close ranks.  Nothing but the mask (n / 8 bytes; nothing at all for a device mask or GSR_REMOVE_HIDDEN alone) crosses the
 * link: the survivors are compacted on the GPU, go through the ordering of an upload, and their planes are carried into the new
 * storage order as gsr_move carries them.
 * THE MASK: bit (i & 31) of word (i >> 5) set = splat i (UPLOAD order, as gsr_update counts) goes -- the sense and layout of
 * gsr_visibility.mask -- in ceil(n / 32) words for the n resident splats; bits at and behind n in the last word are ignored.  A HOST
 * pointer, or with mask_is_device != 0 device memory of the context's device or pinned host memory, checked like the sources of the
 * device verbs above (4-byte aligned, the memory type, every byte inside its allocation) before anything is launched; the verb then
 * waits for the work queued on the context's public stream, as they do.  NULL only with GSR_REMOVE_HIDDEN.
 * flags: GSR_REMOVE_HIDDEN = also remove every splat the visibility in force hides: splat i goes iff its bit of `mask` is set or the
 * rule of gsr_set_visibility (volumes and visibility mask in force, on the raw P bits) calls it hidden.  Without a visibility in force
 * the flag removes nothing extra.
 * THE SURVIVORS keep their relative upload order: survivor i becomes upload index i' = the number of survivors before it, and every
 * later gsr_update / gsr_move / gsr_set_visibility counts in that index space.  gsr_remove_map is the rule on the host (no context, no
 * GPU): new_index[i] = i', or -1 for a removed splat, for i < n; *n_left = the survivors (either out pointer may be NULL).
 * CONTRACT: after GSR_OK the resident geometry -- geoA, geoB, every colour chunk, the colour rows, the cluster bounds and the storage
 * order -- is bit for bit what a fresh context holds after gsr_upload of the survivors' arrays in that order (same
 * GSR_OPT_STORAGE_ORDER, SH presence and origin), and so is every later frame, in every option mode, target format, frame verb and
 * band.  Whatever a frame of the cloud before left is dropped as an upload drops it.  *n_left (may be NULL) = the splats left.
 * With a visibility in force the volumes stay in force, the survivors' true alphas and their bits of a visibility mask in force are
 * carried into the new upload order (a hidden survivor stays hidden), and the contract is gsr_set_visibility's over the survivors.
 * After GSR_REMOVE_HIDDEN gsr_get_visibility reports 0 hidden.
 * Nothing removed: GSR_OK, *n_left = n, no resident bit changes and nothing is invalidated.  Everything removed: the context holds the
 * empty cloud, as after gsr_upload of 0 splats.
 * Synchronous; waits for every frame in flight first.  gsr_stats does not grow and its uploads, moves, upload_ms and move_ms are left
 * alone; gsr_get_removal reports the calls that removed something, the splats the last one removed, and its stage clock ms[4]:
 *   [0] host -> device wall clock of the mask copy (0.0 for a device mask)   [1] marking, scan, compaction, bounding box, Morton
 *   codes and sort (HIP events)   [2] k_repack and the cluster bounds (HIP events)   [3] wall clock of the call.
 * MEMORY: a removal ALWAYS writes the survivors into the spare planes, also under GSR_OPT_STORAGE_ORDER = 0 (the slots change even
 * when the order does not): a context that uses the verb keeps the second copy of the resident planes that gsr_move documents, and
 * with a visibility in force a second array of true alphas (4 bytes per splat of capacity).  The capacity and every buffer sized by
 * it stay: nothing is freed or shrunk.
 * GSR_E_INVALID, with the context untouched: NULL ctx; a NULL mask without GSR_REMOVE_HIDDEN; unknown flag bits; no geometry
 * resident; an upload in progress; a device mask that fails the pointer check.  Everything is allocated before the first write to
 * resident memory or to the visibility's state: GSR_E_OOM leaves the context untouched.  A HIP failure after that leaves NO
 * geometry, as a failed gsr_move does.
 * Out of scope: the GSplatRenderer shim and the HDK glue (their rows are borrowed host arrays, and Houdini hands a changed point
 * count over as new arrays without saying which points went: that is a re-stage); gsr_comm_* (each rank is a plain context and
 * calls gsr_remove itself); giving memory back (shrinking the capacity, freeing the spare planes);
 * an asynchronous form. */
#define GSR_REMOVE_HIDDEN 1     /* flags: also remove every splat the visibility in force hides */
#define GSR_REMOVE_BLOCK  4096  /* upload indices one workgroup of the compaction kernels spans (k_remove.h) */
int  gsr_remove(gsr_context* ctx, const uint32_t* mask, int mask_is_device, int flags, int64_t* n_left);
int  gsr_remove_map(const uint32_t* mask, int64_t n, int32_t* new_index, int64_t* n_left);   /* host, no context, no GPU */
int  gsr_get_removal(gsr_context* ctx, int64_t* removals, int64_t* removed_last, double ms[4]);   /* any pointer may be NULL */

/* ---- adding (splats appended to the resident cloud on the GPU, without a re-upload) ---------------------------------------------- */
/* A trainer's densification step, a merge of two captures, a simulation that emits splats: m new splats join the n resident ones.
 * Only the m new rows cross the link (nothing at all for device sources): every position goes through the ordering of an upload on
 * the GPU, and the planes of the larger cloud are written in the new storage order from the resident planes (old splats) and the
 * staged rows (new ones) by one kernel (k_add.h).
 * gsr_add: host arrays in gsr_upload_append's layout, m rows; all required for m > 0, the three SH arrays exactly when the resident
 * cloud has SH.  gsr_add_device: float32 arrays in device memory under gsr_upload_append_device's rules -- P required, the NULL
 * defaults (Cd 0, alpha 1, scale 1, orient identity), sh given exactly when the cloud has SH with sh_vec3_per_point in 1..16, every
 * pointer checked before anything is launched, the work queued on the context's public stream waited for first, the attributes
 * quantised on the GPU; its NaN exception is gsr_upload_append_device's.
 * INDEX SPACE: the new splats get the upload indices [n, n + m) in the order given; every resident splat keeps its index, and every
 * later gsr_update / gsr_move / gsr_set_visibility / gsr_remove counts in the new space.  *n_total (may be NULL) = n + m.
 * CONTRACT: after GSR_OK the resident geometry -- geoA, geoB, every colour chunk, the colour rows, the cluster bounds and the storage
 * order -- is bit for bit what a fresh context holds after gsr_upload of the concatenation (the resident arrays as edited so far,
 * then the new rows; same GSR_OPT_STORAGE_ORDER, SH presence and the origin in force: there is no origin parameter), and so is every
 * later frame, in every option mode, target format, frame verb and band.  Whatever a frame of the cloud before left is dropped as an
 * upload drops it.
 * With a visibility in force the volumes apply to the new splats at their positions, a mask in force is carried and extended with
 * clear bits, the true alphas of the new rows are put aside behind the old ones, and the contract is gsr_set_visibility's over the
 * concatenation with the mask extended by zeros; gsr_get_visibility reports the new hidden count and mask_splats = n + m.
 * m == 0: GSR_OK, nothing changes and nothing is invalidated.  Adding to the EMPTY cloud (after gsr_upload of 0 splats, or a removal
 * of everything) leaves what gsr_upload of the rows leaves.
 * CAPACITY: the one edit that can need more room than the context has.  gsr_add_capacity(capacity, n_needed) is the policy, a pure
 * host function (no context, no GPU): n_needed <= capacity gives capacity; otherwise min(n_needed + n_needed / 4, 0x7fffffff) -- the
 * 25 % headroom the list buffers take; a negative argument or n_needed > 0x7fffffff gives GSR_E_INVALID.  When n + m exceeds the
 * capacity in force the add GROWS the context to that value: the planes are written at the new capacity and the old set is freed,
 * and every per-splat buffer of the frame slots and of the visibility follows, all of it allocated before the first write.  A later
 * gsr_upload of a smaller cloud keeps the larger capacity.  A run of small adds therefore grows now and then, not every time.
 * MEMORY: an add ALWAYS writes the larger cloud into a second set of planes, also under GSR_OPT_STORAGE_ORDER = 0; without growth
 * that is the spare copy gsr_move documents, which stays.  After a growth there is no spare copy: the next edit that needs one
 * allocates it again, at the new capacity.
 * Synchronous; waits for every frame in flight first.  gsr_stats.uploads, moves, upload_ms and move_ms are left alone; gsr_get_add
 * reports the calls that added something, the rows the last one added, the capacity in force, how often an add grew it, and the
 * last call's stage clock ms[4]:
 *   [0] host -> device wall clock of the new rows (0.0 for device sources)   [1] positions in upload order, bounding box, Morton
 *   codes and sort (HIP events)   [2] k_add_pack and the cluster bounds (HIP events)   [3] wall clock of the call.
 * GSR_E_INVALID, with the context untouched: NULL ctx; m < 0; n + m > 0x7fffffff; a NULL required array with m > 0; SH arrays for a
 * cloud without SH, or a cloud with SH and not all three arrays (device form: sh absent or present against the cloud, or
 * sh_vec3_per_point outside 1..16); no geometry ever uploaded; an upload in progress; a device source that fails the pointer check.
 * Everything is allocated before the first write to resident memory or to the visibility's state: GSR_E_OOM leaves the context
 * untouched.  A HIP failure after that leaves NO geometry, as a failed gsr_move does.
 * Out of scope: the GSplatRenderer shim and the HDK glue (Houdini hands a changed point count over as new arrays: that is a
 * re-stage); gsr_comm_* (each rank is a plain context and calls gsr_add itself); raw float32 HOST sources; inserting at an index
 * other than the end; an in-place tail append under GSR_OPT_STORAGE_ORDER = 0; giving memory back; a gsr_reserve; an asynchronous
 * form. */
int  gsr_add(gsr_context* ctx, int64_t m, const float* P, const uint16_t* Cd, const float* alpha, const uint16_t* scale,
             const uint16_t* orient, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, int64_t* n_total);
int  gsr_add_device(gsr_context* ctx, int64_t m, const gsr_device_attrs* a, int64_t* n_total);
int64_t gsr_add_capacity(int64_t capacity, int64_t n_needed);   /* host, no context, no GPU */
int  gsr_get_add(gsr_context* ctx, int64_t* adds, int64_t* added_last, int64_t* capacity, int64_t* grows, double ms[4]);   /* any pointer may be NULL */

/* ---- reading back (the resident cloud in upload order, from the GPU) -------------------------------------------------------------- */
/* Saving what a densify / prune / crop session left, or handing it to the next tool on the GPU: the attributes of the resident splats
 * [first, first + n) come back in UPLOAD order -- the index space in force now, after every remove and add -- without the caller
 * keeping a shadow copy of every array and replaying every edit.  One streaming kernel (k_read.h: k_pack run backwards) gathers the
 * rows through the inverse of the storage order; the resident layout loses nothing of what was uploaded.
 * gsr_read_info: what a caller needs to size the arrays -- the resident count, whether the cloud has SH, the origin in force; no
 * kernel, no synchronisation; any pointer may be NULL.
 * gsr_read: HOST destinations in gsr_upload_append's layout (P float[3n]; Cd half[3n]; alpha float[n]; scale half[3n]; orient
 * half[4n]; shx / shy / shz half[16n], all three or none and only for a cloud with SH), rows for [first, first + n); NULL = not
 * wanted.  The kernel writes device rows of the context's own (the upload staging arena, sized for the range), then every wanted array
 * is copied device -> host.
 * gsr_read_device: DEVICE destinations, float32, in gsr_device_attrs' layout -- SH coefficient j, channel c of row t at
 * sh[(t * vpp + j) * 3 + c], vpp = sh_vec3_per_point in 1..16; slots j >= vpp are not written out.  The kernel writes the caller's
 * arrays where they are: nothing is staged and nothing crosses the link.
 * CONTRACT: after GSR_OK rows [0, n) of every array given hold, bit for bit, what a fresh gsr_upload would have to be given to leave
 * the context as it is:
 *   P       the raw position bits: NaN payloads, infinities and -0 come back as they went in;
 *   alpha   the splat's TRUE alpha: under a visibility in force a hidden splat reads back its own alpha, not the resident +0.0f (the
 *           hidden set is gsr_visibility_eval on the P read);
 *   halves  the resident bits.  The extent half of geoB is derived and is not returned.  Index 15 of the x / y / z rows (slot 15 of a
 *           16-slot sh row) is not resident -- the renderer never reads it -- and comes back as a zero half (+0.0f);
 *   the device form returns every half as the float32 of exactly that value (denormals included, no rounding anywhere); a NaN half
 *           becomes a NaN float with unspecified sign and payload (the NaN rule of the target formats above).
 * So a fresh context given gsr_upload of a whole-cloud gsr_read -- or gsr_upload_append_device of a whole-cloud gsr_read_device with
 * sh_vec3_per_point = 16 -- with the same GSR_OPT_STORAGE_ORDER, the origin of gsr_read_info and, under a visibility, the same
 * gsr_set_visibility, holds the same geoA, geoB, colour chunks, colour rows, cluster bounds and storage order.
 * A READ CHANGES AND INVALIDATES NOTHING: no resident bit changes; depth horizons, cached depth orders, policies and the visibility
 * stay; gsr_stats.uploads, moves, upload_ms and move_ms stay; the next frame runs the launches it would have run.  It does not wait
 * for the frames in flight: they never write resident planes.  A context that never reads launches nothing new.
 * ORDERING: the device form first waits for the work queued on the context's public stream (gsr_set_stream) -- a consumer still
 * reading the destinations from the previous iteration has finished.  Both forms are synchronous: on return the destinations are
 * complete.  Every non-NULL device destination is checked before anything is launched, exactly as the device sources above are
 * (4-byte aligned; device memory of the context's device or pinned host memory; all n x row bytes inside the allocation).
 * Overlapping destinations are the caller's mistake and are not detected.
 * GSR_E_INVALID, nothing written: NULL ctx or struct; no geometry ever uploaded, or an upload in progress; first < 0, n < 0 or
 * first + n beyond the resident count; one or two of the three SH arrays; SH destinations for a cloud without SH;
 * sh_vec3_per_point outside 1..16 with sh given; reserved_ != 0; a device destination that fails the pointer check.
 * n == 0, or nothing asked for: GSR_OK, nothing happens and nothing is counted.  The empty cloud (after removing everything) reads 0
 * rows.  Everything is allocated before the launch: GSR_E_OOM leaves the context untouched, and so does a HIP failure, since nothing
 * resident is written.
 * gsr_get_read: the calls that read something, the rows of the last one, and its clock ms[4]: [0] the kernel (HIP events)
 * [1] device -> host copies, wall clock (0.0 for the device form)   [2] 0.0 (reserved)   [3] wall clock of the call.
 * gsr_multi_read (below, with the other gsr_multi verbs): rank 0's copy -- the cloud is replicated.
 * Out of scope: the GSplatRenderer shim and the HDK glue (their rows are the caller's own host arrays already); gsr_comm_* (each
 * rank is a plain context and reads for itself); reading by an index list (by a mask: "copying", below); an asynchronous form; half destinations in
 * device memory; a PLY writer (the INRIA activations are not bit-invertible, and a writer with a tolerance is its own piece of
 * work); a hidden-mask output. */
int  gsr_read_info(gsr_context* ctx, int64_t* n_splats, int* has_sh, float origin[3]);   /* any pointer may be NULL */
typedef struct gsr_read_arrays {          /* HOST destinations in gsr_upload_append's layout, rows for [first, first + n); NULL = not wanted */
    float*    P;                          /* float[3n] */
    uint16_t* Cd;                         /* half[3n]  */
    float*    alpha;                      /* float[n]  */
    uint16_t* scale;                      /* half[3n]  */
    uint16_t* orient;                     /* half[4n] (x, y, z, w) */
    uint16_t *shx, *shy, *shz;            /* half[16n] each */
} gsr_read_arrays;
int  gsr_read(gsr_context* ctx, int64_t first, int64_t n, const gsr_read_arrays* out);
typedef struct gsr_device_out {           /* DEVICE destinations, float32, the layout of gsr_device_attrs; NULL = not wanted */
    float *P, *Cd, *alpha, *scale, *orient, *sh;
    int32_t sh_vec3_per_point;            /* 1..16 when sh is given: slots j >= it are not written out */
    int32_t reserved_;                    /* 0 */
} gsr_device_out;
int  gsr_read_device(gsr_context* ctx, int64_t first, int64_t n, const gsr_device_out* out);
int  gsr_get_read(gsr_context* ctx, int64_t* reads, int64_t* rows_last, double ms[4]);   /* any pointer may be NULL */

/* ---- copying (selected resident splats read out, or duplicated, on the GPU) ---------------------------------------------------------- */
/* The two verbs an editor offers next to delete, move and grade, for the mask gsr_select makes: EXTRACT the selection (gsr_read's
 * contract over a mask in the place of a range) and DUPLICATE it (a copy of each selected splat appended to the cloud), without
 * carrying the cloud over the link.  Kernels: k_copy.h -- gsr_remove's compaction with the selected splats in the survivors' place --
 * in front of k_unpack (a read) or the ordering of an upload and k_repack (a duplicate).
 * THE MASK is gsr_select's and gsr_remove's: ceil(n / 32) words, bit i % 32 of word i / 32 = splat i of the upload is selected; bits at
 * indices >= n in the last word are ignored; NULL selects every splat.  mask_is_device = 0: host memory, copied before the call
 * returns; 1: device memory of the context's device or pinned host memory, read where it is, checked like a device source before
 * anything is launched and never written.  gsr_copy_map is the rule on the host (no context, no GPU): rows[r] (NULL: not wanted) =
 * the upload index of the r-th set bit, ascending; *m = their number.
 * gsr_read_masked / gsr_read_masked_device: row r of every wanted array is what gsr_read / gsr_read_device return for the splat
 * rows[r], bit for bit -- the raw P bits, the TRUE alpha of a splat a visibility hides, the resident halves (the device form: each as
 * the float32 of exactly that value), index 15 of the SH rows a zero half.  The destinations hold max_rows rows; the device form checks
 * every one of them for max_rows rows before anything is launched.  *m (may be NULL) = the rows of the selection.  A selection of more
 * than max_rows rows: GSR_E_INVALID, *m is set and no destination byte is written.  With every destination NULL (out may then be NULL
 * too) the call is a count: *m is filled and nothing else happens; max_rows is not looked at.  Like gsr_read the call changes and
 * invalidates nothing, does not wait for the frames in flight, and is counted by gsr_get_read (a count, a refusal and a read of no rows
 * are not).  Of the link, a device mask and device destinations use one word: the count.
 * gsr_duplicate: a copy of each selected splat joins the cloud at the upload indices [n, n + m), in the ascending upload order of the
 * originals; every resident splat keeps its index.  Afterwards geoA, geoB, colour chunks, colour rows, cluster bounds, storage order and
 * every later frame are, bit for bit, those of a fresh gsr_upload of concat(R, R[rows]), R = what gsr_read(0, n) returned before.  No
 * row leaves the resident planes and nothing is quantised again.  Under a visibility in force the result is what gsr_add of those rows
 * leaves: the copies carry their originals' TRUE alphas, the volumes apply to them, a mask is extended by clear bits.  A duplicate that
 * does not fit grows the context by gsr_add_capacity as an add does; gsr_get_add reports the capacity and counts the growth (its adds
 * and added_last stay).  *m, *n_total (may be NULL) = the copies, the splats resident now.  An empty selection changes, invalidates and
 * writes nothing.  gsr_stats.n_splats follows; uploads and moves stay.  Synchronous; waits for every frame in flight and for the public
 * stream first.  A failure before the first write leaves the context as it was; one after it leaves no geometry, as gsr_add's does.
 * gsr_get_duplicate: the calls that copied something, the copies of the last one, its clock ms[4]: [0] host mask over the link
 * [1] mark .. sort (HIP events)   [2] repack (HIP events)   [3] wall clock of the call.
 * GSR_E_INVALID, nothing written: NULL ctx; no geometry, or an upload in progress; a device mask that fails the pointer check; for the
 * reads what gsr_read / gsr_read_device refuse of their structs, max_rows < 0 with a destination given, a device destination that fails
 * the pointer check for max_rows rows; for a duplicate n + m beyond 2^31 - 1.
 * gsr_multi_read_masked: rank 0's copy, from a host mask into host arrays.  gsr_multi_duplicate: every rank, from a host mask, under
 * gsr_multi_add's agreement rule.
 * Out of scope: the GSplatRenderer shim and the HDK glue; gsr_comm_*; a device mask for the multi verbs; reading by an explicit index
 * list; copies with a built-in offset (gsr_transform with the mask of the copies); copying between two contexts; asynchronous forms;
 * half destinations in device memory; giving memory back. */
int  gsr_copy_map(const uint32_t* mask, int64_t n, int32_t* rows, int64_t* m);   /* host, no context, no GPU */
int  gsr_read_masked(gsr_context* ctx, const uint32_t* mask, int mask_is_device, int64_t max_rows, const gsr_read_arrays* out, int64_t* m);
int  gsr_read_masked_device(gsr_context* ctx, const uint32_t* mask, int mask_is_device, int64_t max_rows, const gsr_device_out* out, int64_t* m);
int  gsr_duplicate(gsr_context* ctx, const uint32_t* mask, int mask_is_device, int64_t* m, int64_t* n_total);
int  gsr_get_duplicate(gsr_context* ctx, int64_t* calls, int64_t* copied_last, double ms[4]);   /* any pointer may be NULL */

/* ---- selection (resident splats picked by screen region, on the GPU) --------------------------------------------------------------- */
/* The masks gsr_set_visibility and gsr_remove take, made from what the user sees: drag a box or paint a lasso over the floaters, and
 * the splats whose CENTRE projects into it come back as a bit mask in upload order -- without reading P and alpha back over the
 * link and restating the vertex stage on the host.  One kernel (k_select.h), one thread per upload index.
 * THE RULE (one function, evaluated by the kernel and by gsr_select_eval; x86 and gfx950 agree bit for bit).  For splat i with raw
 * position bits (px, py, pz) and RESIDENT opacity a, the steps are the vertex stage's own, in its order, every multiply-add one fmaf:
 *   1. x = (px - origin.x) + origin.x, likewise y, z                                  (the origin round trip)
 *   2. tv = obj_view rows . (x, y, z, 1);  ftvy = -tv.y
 *   3. cl = proj rows . (tv.x, ftvy, tv.z, 1)
 *   4. selectable: cl.w > 0 && !(cl.z < -cl.w || cl.z > cl.w) && a >= 1/255; GSR_SELECT_ANY_OPACITY drops the last term.  Under a
 *      visibility in force a hidden splat's resident opacity is +0.0f: by default it is never hit, with the flag it can be.
 *   5. cx = fmaf(cl.x / cl.w, 0.5, 0.5) * W;  cy = fmaf((-cl.y) / cl.w, 0.5, 0.5) * H;  zw = fmaf(cl.z / cl.w, 0.5, 0.5)
 *      (W, H = (float)width, (float)height of the camera; IEEE divisions) -- the centre and window depth of the frame's record.
 * A splat is HIT iff it is selectable and passes every clause that is given; a NaN anywhere (centre or window depth) means no hit:
 *   rect   always: x0 <= cx && cx < x1 && y0 <= cy && cy < y1 -- GL window coordinates, row 0 at the bottom, half-open.  Infinities
 *          are allowed: (-inf, -inf, +inf, +inf) is "everywhere".
 *   pixel  only when an image or a depth buffer is given: cx >= 0 && cx < W && cy >= 0 && cy < H, otherwise no hit; then
 *          p = (int)cy * width + (int)cx.  No index is ever formed from a centre outside the image.
 *   image  a lasso, a brush, any painted region, rasterised by the caller: bit p & 31 of word p >> 5 is set.  One bit per pixel,
 *          packed across rows without padding, ceil(width * height / 32) words.
 *   depth  zw <= depth[p] + depth_bias (one float32 add, one compare).  depth: float[height * width] window depths as
 *          gsr_render_depth takes them.  The opaque pass's depth selects only what geometry does not hide; gsr_resolve_depth of the
 *          depth AOV with a small positive bias selects only the surface layer of the splats themselves.
 * THE MASK has the layout and sense of gsr_visibility.mask and of gsr_remove's mask: bit i & 31 of word i >> 5 is upload index i,
 * ceil(n / 32) words (n: the resident count, gsr_read_info), and the result feeds either verb as it is -- a device mask goes
 * straight into gsr_remove(mask, 1, ...) with nothing crossing the link.  With hit = the rule's verdicts, op decides what the mask
 * holds afterwards (GSR_SELECT_*); every op but REPLACE reads the mask first (a host mask is copied in).  After any op the bits at and
 * behind n in the last word are 0, and not one byte behind word ceil(n / 32) - 1 is written.  The result is deterministic: no atomic
 * touches the mask.
 * n_hit: the splats the rule hit, whatever the op; n_set: the bits set afterwards.  Either may be NULL.
 * SOURCES: host images and depth buffers are copied when the call is made; device ones (image_is_device / depth_is_device) are read in
 * place.  Every device pointer -- mask, image, depth -- is checked with its exact byte size before anything is launched, exactly as the
 * device sources above are; a bad pointer gives GSR_E_INVALID, never a fault.
 * gsr_select_eval: the rule on the host, with no context and no GPU, through the function the kernel evaluates.  P: float[3n] raw
 * positions; opacity: float[n] RESIDENT opacities (NULL = 1); image and depth of the region are HOST pointers whatever the _is_device
 * fields say; op is checked and not applied.  hit_out[k] = 0 / 1; centre_out (or NULL): [n][3] = cx, cy, zw of a selectable splat,
 * else three NaNs.
 * A SELECT CHANGES AND INVALIDATES NOTHING -- gsr_read's contract: no resident bit changes; depth horizons, cached depth orders,
 * policies, the visibility and every entry of gsr_stats stay; it does not wait for the frames in flight; the next frame runs the
 * launches it would have run.  A context that never selects launches nothing new.
 * ORDERING: gsr_read's (host mask) and gsr_read_device's (device mask): with any device pointer the call first waits for the work
 * queued on the context's public stream (gsr_set_stream) -- a gsr_resolve_depth_device queued there has finished.  Both forms are
 * synchronous: on return the mask and the counts are complete.
 * GSR_E_INVALID, nothing written: NULL ctx, camera, region or mask; no geometry ever uploaded, or an upload in progress; width or
 * height outside 1..GSR_MAX_DIM; an unknown op, unknown flag bits, or reserved_ != 0; a device pointer that fails the check.  The
 * empty cloud gives GSR_OK, writes nothing, and both counts are 0.
 * gsr_get_select: the calls that selected, the splats hit by the last one, and its clock ms[4]: [0] the kernel (HIP events)
 * [1] the copies, wall clock   [2] 0.0 (reserved)   [3] wall clock of the call.
 * gsr_multi_select (below, with the other gsr_multi verbs): rank 0's context and a host mask -- the cloud is replicated.
 * Out of scope: the GSplatRenderer shim and the HDK glue (renderPick speaks Houdini's pick-buffer protocol); gsr_comm_* (each rank
 * selects for itself); rasterising a lasso polygon into the image; a device mask for gsr_set_visibility; per-pixel id buffers;
 * selecting by a splat's footprint instead of its centre; an asynchronous form. */
#define GSR_SELECT_REPLACE   0   /* mask = hit                */
#define GSR_SELECT_ADD       1   /* mask |= hit               */
#define GSR_SELECT_SUBTRACT  2   /* mask &= ~hit              */
#define GSR_SELECT_INTERSECT 3   /* mask &= hit               */
#define GSR_SELECT_TOGGLE    4   /* mask ^= hit               */
#define GSR_SELECT_ANY_OPACITY 1 /* flags: no opacity test -- splats below 1/255, and the ones a visibility hides, can be hit */
#define GSR_SELECT_BLOCK     256 /* upload indices one workgroup of the selection kernel spans (k_select.h) */
typedef struct gsr_select_region {
    float x0, y0, x1, y1;                 /* the rect, GL window coordinates, half-open */
    const uint32_t* image;                /* NULL: no image clause */
    int32_t image_is_device;
    const float*    depth;                /* NULL: no depth clause */
    int32_t depth_is_device;
    float   depth_bias;
    int32_t op;                           /* GSR_SELECT_REPLACE .. GSR_SELECT_TOGGLE */
    int32_t flags;                        /* GSR_SELECT_ANY_OPACITY or 0 */
    int32_t reserved_;                    /* 0 */
} gsr_select_region;
int  gsr_select(gsr_context* ctx, const gsr_camera* cam, const gsr_select_region* region,
                uint32_t* mask, int mask_is_device, int64_t* n_hit, int64_t* n_set);
int  gsr_select_eval(const gsr_camera* cam, const float origin[3], const gsr_select_region* region /* host pointers */,
                     const float* P, const float* opacity /* resident; NULL = 1 */, int64_t n,
                     uint8_t* hit_out, float* centre_out /* [n][3] = cx, cy, zw of a selectable splat, else NaN; or NULL */);   /* host, no context, no GPU */
int  gsr_get_select(gsr_context* ctx, int64_t* calls, int64_t* hit_last, double ms[4]);   /* any pointer may be NULL */

/* ---- selection by attribute (resident splats picked by what they are, on the GPU) --------------------------------------------------- */
/* The mask gsr_select makes, from what a splat IS instead of where its centre projects: prune everything below an opacity, larger than
 * a size or thinner than a needle; pick what lies in a box or an ellipsoid; key out a base colour -- without reading P, alpha, scale
 * and Cd back over the link.  One streaming kernel (k_select_attrs.h), one thread per upload index, gsr_select's mask epilogue.
 * THE RULE (one function, evaluated by the kernel and by gsr_select_attrs_eval; x86 and gfx950 agree bit for bit).  For splat i,
 * with a = its TRUE alpha (what gsr_read returns: under a visibility in force a hidden splat's own alpha, not the resident +0.0f),
 * s_k = h2f(scale half k), smax / smin = the largest / smallest of |s_0|, |s_1|, |s_2|, and Cd_c = h2f(Cd half c), a splat is HIT
 * iff it passes every clause that is set in `clauses` (none set: every splat):
 *   GSR_ATTR_ALPHA       alpha_lo <= a <= alpha_hi
 *   GSR_ATTR_SCALE_MAX   scale_max_lo <= smax <= scale_max_hi
 *   GSR_ATTR_SCALE_MIN   scale_min_lo <= smin <= scale_min_hi
 *   GSR_ATTR_ANISOTROPY  smax > 0 && smax >= anisotropy * smin      (one float32 multiply: a needle; all three scales 0 never pass)
 *   GSR_ATTR_COLOUR      colour_lo[c] <= Cd_c <= colour_hi[c] for c = r, g, b
 *   GSR_ATTR_VOLUME      every one of volume[0 .. n_volumes) passes: gsr_volume_inside(volume, raw P) != invert -- the function of
 *                        gsr_set_visibility, with its float32 chains; an inverted volume passes what is NOT inside it
 * A NaN anywhere a clause looks means no hit: a NaN alpha, a NaN scale half (for any of the three scale clauses), a NaN Cd half (for
 * the colour clause), a NaN bound, a NaN coordinate of P (for the volume clause).  lo > hi is allowed and hits nothing; infinite bounds
 * are allowed.  Non-finite matrix entries of a volume are the caller's data and follow the visibility's rule.
 * flags: GSR_ATTR_SKIP_HIDDEN -- a splat the visibility in force hides (its volumes and mask, gsr_splat_visible on the raw P) is never
 * hit; with no visibility in force nothing is hidden.
 * THE MASK, op, n_hit and n_set are gsr_select's: ceil(n / 32) words in upload order, host (mask_is_device = 0) or device / pinned memory
 * (1: checked with its exact size before anything is launched); every op but REPLACE reads the mask first; after any op the bits at and
 * behind n are 0 and not one byte behind word ceil(n / 32) - 1 is written; no atomic touches the mask.  n_hit: the splats the rule
 * hit, whatever the op; n_set: the bits set afterwards; either may be NULL.
 * gsr_select_attrs_eval: the rule on the host, no context and no GPU.  Arrays in gsr_read's layout (P float[3n], alpha float[n] TRUE
 * alphas, scale half[3n], Cd half[3n]); an array no set clause looks at may be NULL.  vis (NULL: none in force) is what SKIP_HIDDEN
 * hides by, as gsr_visibility_eval takes it (a mask must cover the n splats).  op is checked and not applied.  hit_out[k] = 0 / 1.
 * A SELECT CHANGES AND INVALIDATES NOTHING -- gsr_read's contract: no resident bit, depth horizon, cached depth order, policy or
 * visibility state changes, no entry of gsr_stats; it does not wait for the frames in flight.  ORDERING: gsr_select's (with a device
 * mask the call first waits for the work queued on the public stream); synchronous.
 * GSR_E_INVALID, nothing written: NULL ctx, rule or mask; no geometry ever uploaded, or an upload in progress; unknown clause or flag
 * bits; reserved_ != 0; n_volumes outside 1..GSR_VIS_MAX_VOLUMES with GSR_ATTR_VOLUME, or not 0 without it; an unknown volume kind;
 * invert neither 0 nor 1; an unknown op; a device mask that fails the pointer check.  The empty cloud gives GSR_OK, writes nothing,
 * and both counts are 0.
 * gsr_get_select_attrs: the calls that selected, the splats hit by the last one, and its clock ms[4], laid out as gsr_get_select's:
 * [0] the kernel (HIP events)   [1] the copies, wall clock   [2] 0.0 (reserved)   [3] wall clock of the call.
 * gsr_multi_select_attrs (below, with the other gsr_multi verbs): rank 0's context and a host mask -- the cloud is replicated.
 * Out of scope: the GSplatRenderer shim and the HDK glue; gsr_comm_* (each rank selects for itself); a device mask for the multi verb;
 * clauses on SH energy or on view-dependent colour; a clause on screen-space size; a device mask for gsr_set_visibility; asynchronous
 * forms. */
#define GSR_ATTR_ALPHA       1   /* alpha_lo <= a <= alpha_hi; a = the TRUE alpha (what gsr_read returns) */
#define GSR_ATTR_SCALE_MAX   2   /* scale_max_lo <= smax <= scale_max_hi */
#define GSR_ATTR_SCALE_MIN   4   /* scale_min_lo <= smin <= scale_min_hi */
#define GSR_ATTR_ANISOTROPY  8   /* smax > 0 && smax >= anisotropy * smin    (one f32 multiply) */
#define GSR_ATTR_COLOUR     16   /* colour_lo[c] <= Cd_c <= colour_hi[c], c = r, g, b; Cd = h2f of the resident Cd halves */
#define GSR_ATTR_VOLUME     32   /* every volume passes: gsr_volume_inside(vol, raw P) != invert, the visibility's own function */
#define GSR_ATTR_SKIP_HIDDEN 1   /* flags: a splat the visibility in force hides is never hit */
typedef struct gsr_attr_rule {
    int32_t clauses;                      /* GSR_ATTR_* (0: every splat) */
    int32_t flags;                        /* GSR_ATTR_SKIP_HIDDEN or 0 */
    int32_t op;                           /* GSR_SELECT_REPLACE .. GSR_SELECT_TOGGLE */
    int32_t n_volumes;                    /* 1..GSR_VIS_MAX_VOLUMES with GSR_ATTR_VOLUME, else 0 */
    float   alpha_lo, alpha_hi;
    float   scale_max_lo, scale_max_hi;
    float   scale_min_lo, scale_min_hi;
    float   anisotropy;
    float   colour_lo[3], colour_hi[3];
    int32_t reserved_;                    /* 0 */
    gsr_crop_volume volume[GSR_VIS_MAX_VOLUMES];
} gsr_attr_rule;
int  gsr_select_attrs(gsr_context* ctx, const gsr_attr_rule* rule, uint32_t* mask, int mask_is_device, int64_t* n_hit, int64_t* n_set);
int  gsr_select_attrs_eval(const gsr_attr_rule* rule, const gsr_visibility* vis /* NULL: none */, int64_t n, const float* P,
                           const float* alpha, const uint16_t* scale, const uint16_t* Cd, uint8_t* hit_out);   /* host, no context, no GPU */
int  gsr_get_select_attrs(gsr_context* ctx, int64_t* calls, int64_t* hit_last, double ms[4]);   /* any pointer may be NULL */

/* ---- selection by density (resident splats picked by how many neighbours they have, on the GPU) -------------------------------------- */
/* The mask gsr_select makes, from how CROWDED a splat's surroundings are: the floaters of a capture (a splat, or a small clump, alone
 * in space), a trainer's density prune -- without reading P back and counting neighbours on the host.  Three kernels (k_density.h)
 * around the stable radix sort that orders an upload; gsr_select's mask epilogue.
 * THE RULE (one set of functions, evaluated by the kernels and by gsr_select_density_eval; x86 and gfx950 agree bit for bit).  The
 * caller gives a uniform grid of 1024^3 cells: `cell`, the float32 edge length, and origin[3], the grid's low corner in upload space
 * (the space of the raw P bits); reach in {0, 1, 2}; an unsigned range count_lo .. count_hi; alpha_min; an op; flags.
 *   1. THE CELL of a splat, per axis c: t = (p_c - origin_c) * inv_cell -- one float32 subtraction and one float32 multiplication,
 *      each rounded once, never fused; inv_cell = 1.0f / cell is one IEEE float32 division made once on the host.  f = floorf(t).
 *      The splat is IN THE GRID iff 0 <= f && f < 1024 on all three axes, compared in float before any conversion: a NaN, an infinity
 *      or a huge t is outside (-0.0f is cell 0).  The cell is (ix, iy, iz) = ((int)f_x, (int)f_y, (int)f_z), its key
 *      ix | iy << 10 | iz << 20.
 *   2. POPULATION: a splat that is in the grid, whose TRUE alpha a (what gsr_read returns: under a visibility in force a hidden
 *      splat's own alpha) satisfies a >= alpha_min (a NaN alpha never does), and that -- under GSR_DENSITY_SKIP_HIDDEN -- the visibility
 *      in force does not hide (gsr_splat_visible on the raw P; with no visibility in force nothing is hidden).  Without the flag a
 *      hidden splat counts with its true alpha.
 *   3. N(i): the number of population splats, i itself included, whose cell differs from i's by at most `reach` on every axis and lies
 *      inside the grid -- a neighbour cell outside 0..1023 on an axis does not exist, so (1023, y, z) and (0, y + 1, z) never count
 *      each other.  N(i) = 0 for a splat that is not population.
 *   4. HIT: a population splat iff count_lo <= N(i) && N(i) <= count_hi, as unsigned integers (count_lo > count_hi is allowed and
 *      hits nothing); an OUTSIDE splat -- one that passes the alpha and visibility tests but is not in the grid -- iff
 *      GSR_DENSITY_HIT_OUTSIDE is set; nothing else.  "Floaters" is count = (1, k - 1).
 *   5. THE MASK, op, n_hit and n_set are gsr_select's: ceil(n / 32) words in upload order, host (mask_is_device = 0) or device / pinned
 *      memory (1: checked with its exact size before anything is launched); every op but REPLACE reads the mask first; after any op the
 *      bits at and behind n are 0 and not one byte behind word ceil(n / 32) - 1 is written; no atomic touches the mask.
 * THE RESULT (NULL: not wanted): n_population; n_outside; n_cells, the occupied cells (n_population / n_cells says whether `cell` was
 * a sensible choice); count_hist[64]: bin b < 63 holds the population splats with N == b + 1, bin 63 those with N >= 64 -- the
 * histogram a threshold k is chosen by.  Integer atomics only: nothing depends on the order the waves run in.
 * counts_out (NULL: skipped): N(i) for every upload index, uint32[n], host (counts_is_device = 0) or device / pinned memory (1:
 * checked for 4 n bytes before anything is launched).
 * gsr_select_density_eval: the rule on the host, no context and no GPU.  P float[3n] and alpha float[n] (NULL: every alpha 1) in
 * gsr_read's layout; vis (NULL: none in force) is what SKIP_HIDDEN hides by, as gsr_visibility_eval takes it (a mask must cover the n
 * splats).  op is checked and not applied.  hit_out[k] = 0 / 1; counts_out and result may be NULL.
 * WHAT THE VERB TOUCHES: nothing the context keeps -- no resident bit, depth horizon, cached depth order, policy, visibility state or
 * entry of gsr_stats -- but a count buffer of its own (4 bytes per splat, kept between calls) and its tally.  It shares the scratch of
 * an upload's sort (which holds nothing live between uploads and edits), so unlike gsr_select it WAITS for the frames in flight and the
 * work queued on the public stream, as gsr_move does.  Synchronous.  A context that never calls it allocates and launches nothing new.
 * GSR_E_INVALID, nothing launched and nothing written: NULL ctx, rule or mask; no geometry ever uploaded, or an upload in progress;
 * cell not finite or <= 0, or 1.0f / cell not finite; a non-finite origin; reach outside 0..2; unknown flag bits; an unknown op;
 * reserved_ != 0; a NaN alpha_min; a device mask or device counts that fail the pointer check.  The empty cloud gives GSR_OK, zeros,
 * and touches no word.
 * gsr_get_select_density: the calls that selected, the splats hit by the last one, and its clock ms[4], laid out as gsr_get_select's:
 * [0] the verb's own kernels (HIP events)   [1] the copies, wall clock   [2] the sort (HIP events)   [3] wall clock of the call.
 * gsr_multi_select_density (below, with the other gsr_multi verbs): rank 0's context, a host mask and host counts.
 * Out of scope: exact k-nearest-neighbour distances or a radius in world units not tied to the grid; more than 1024 cells per axis; a
 * per-splat grid; connected components (gsr_select_connected, below, is that verb); the GSplatRenderer shim and the HDK glue; gsr_comm_*; a device mask for
 * the multi verb; an asynchronous form; results left in device memory. */
#define GSR_DENSITY_SKIP_HIDDEN 1   /* flags: a splat the visibility in force hides is not population */
#define GSR_DENSITY_HIT_OUTSIDE 2   /* flags: a splat outside the grid (that passes the alpha and visibility tests) is hit */
#define GSR_DENSITY_CELLS    1024   /* cells per axis */
#define GSR_DENSITY_MAX_REACH   2
#define GSR_DENSITY_HIST_BINS  64
typedef struct gsr_density_rule {
    float    cell;                        /* the cells' edge length: finite, > 0, 1.0f / cell finite */
    float    origin[3];                   /* the grid's low corner, upload space */
    int32_t  reach;                       /* 0..GSR_DENSITY_MAX_REACH */
    int32_t  flags;                       /* GSR_DENSITY_* or 0 */
    int32_t  op;                          /* GSR_SELECT_REPLACE .. GSR_SELECT_TOGGLE */
    int32_t  reserved_;                   /* 0 */
    uint32_t count_lo, count_hi;          /* hit iff count_lo <= N <= count_hi */
    float    alpha_min;                   /* population iff a >= alpha_min (-INFINITY: every alpha but a NaN) */
} gsr_density_rule;
typedef struct gsr_density_result {
    int64_t n_population, n_outside, n_cells;
    int64_t count_hist[GSR_DENSITY_HIST_BINS];
} gsr_density_result;
int  gsr_select_density(gsr_context* ctx, const gsr_density_rule* rule, uint32_t* mask, int mask_is_device,
                        uint32_t* counts_out /* NULL */, int counts_is_device, gsr_density_result* result /* NULL */,
                        int64_t* n_hit, int64_t* n_set);
int  gsr_select_density_eval(const gsr_density_rule* rule, const gsr_visibility* vis /* NULL: none */, int64_t n, const float* P,
                             const float* alpha /* NULL: all 1 */, uint8_t* hit_out, uint32_t* counts_out /* NULL */,
                             gsr_density_result* result /* NULL */);   /* host, no context, no GPU */
int  gsr_get_select_density(gsr_context* ctx, int64_t* calls, int64_t* hit_last, double ms[4]);   /* any pointer may be NULL */

/* ---- selection by connectivity (resident splats picked by the connected clump of occupied cells they lie in, on the GPU) ------------- */
/* The mask gsr_select makes, from the CLUMP a splat belongs to.  Floaters come in clumps: five of them in adjacent cells give each other
 * N >= 5 and gsr_select_density keeps them; what marks them is that the clump is small.  "Every connected group of fewer than k splats"
 * is size = (1, k - 1); "grow my selection to the object it touches" is a seed mask.  The key kernel and the sort of
 * gsr_select_density, then a table of the occupied cells, a lock-free union-find over it and gsr_select's mask epilogue (k_connect.h).
 * THE RULE (one set of functions, evaluated by the kernels and by gsr_select_connected_eval; x86 and gfx950 agree bit for bit).
 *   1. GRID, POPULATION, OUTSIDE: exactly gsr_select_density's items 1 and 2 -- cell, origin[3], 1024 cells per axis, the key
 *      ix | iy << 10 | iz << 20, alpha_min, GSR_CONNECT_SKIP_HIDDEN and GSR_CONNECT_HIT_OUTSIDE as the density flags.
 *   2. ADJACENCY: two OCCUPIED cells (cells that hold at least one population splat) are adjacent iff their indices differ by at most
 *      `reach` (0..2) on every axis.  The grid does not wrap: (1023, y, z) and (0, y + 1, z), consecutive as keys, are not adjacent.
 *      At reach 0 no two cells are adjacent.
 *   3. COMPONENT: an equivalence class of occupied cells under the transitive closure of adjacency.  Every population splat carries
 *      its component's SIZE, the number of population splats in it (uint32, 1..n), and its LABEL, the smallest upload index among
 *      them -- canonical, independent of the grid's keys: labels[i] == labels[picked] says "same clump as the one I clicked".
 *   4. HIT: a population splat iff every clause that is set passes -- size_lo <= size && size <= size_hi as unsigned integers
 *      (size_lo > size_hi is allowed and hits nothing), and, if a seed mask is given, its component holds at least one POPULATION splat
 *      whose seed bit is set; an OUTSIDE splat iff GSR_CONNECT_HIT_OUTSIDE, whatever the clauses; nothing else.
 *      THE SEED (NULL: no seed clause) has the layout of the mask: ceil(n / 32) words in upload order, host (seed_is_device = 0) or
 *      device / pinned memory (1); bits at or behind n are ignored; a bit on a splat that is not population seeds nothing.  It MAY be
 *      the mask itself: every word of it is consumed before the mask is written, so op = ADD with seed == mask grows a selection in
 *      place.
 *   5. THE MASK, op, n_hit and n_set are gsr_select's (see gsr_select_density, item 5).
 * THE RESULT (NULL: not wanted): n_population, n_outside, n_cells as gsr_density_result's; n_components; n_seeded, the components that
 * hold a seed (0 without a seed clause); largest, the largest size; comp_hist[32]: bin b holds the components with
 * floor(log2(size)) == b; splat_hist[32]: the population splats in those components -- a size_hi is chosen from it.  Integer atomics
 * only: nothing depends on the order the waves run in.
 * labels_out / sizes_out (each NULL: skipped): uint32[n] in upload order, both host (outs_are_device = 0) or both device / pinned
 * memory (1: each checked for 4 n bytes before anything is launched); GSR_CONNECT_NO_LABEL and 0 for a splat that is not population.
 * gsr_select_connected_eval: the rule on the host, no context and no GPU; P, alpha and vis as gsr_select_density_eval takes them;
 * seed_bits: ceil(n / 32) packed words or NULL; op is checked and not applied; hit_out[k] = 0 / 1; labels_out, sizes_out and result may
 * be NULL.  A sequential union-find with the kernels' hook rule (the larger table index under the smaller).
 * WHAT THE VERB TOUCHES: nothing the context keeps -- no resident bit, depth horizon, cached depth order, policy, visibility state or
 * entry of gsr_stats -- but a cell table of its own (28 bytes per splat, kept between calls; the 4 bytes per splat of
 * gsr_select_density's count buffer are shared) and its tally.  Like gsr_select_density it shares the scratch of an upload's sort, so
 * it WAITS for the frames in flight and the work queued on the public stream.  Synchronous.  A context that never calls it allocates
 * and launches nothing new.
 * GSR_E_INVALID, nothing launched and nothing written: NULL ctx, rule or mask; no geometry ever uploaded, or an upload in progress;
 * what gsr_select_density refuses of cell, origin, reach, flags, op, reserved_ and alpha_min; a device seed, mask, labels_out or
 * sizes_out that fails the pointer check.  The empty cloud gives GSR_OK, zeros, and touches no word.
 * gsr_get_select_connected: the calls that selected, the splats hit by the last one, and its clock ms[4]:
 * [0] the verb's own kernels (HIP events)   [1] the copies, wall clock   [2] the sort (HIP events)   [3] wall clock of the call.
 * gsr_debug_select_connected_stages: the last call's kernels stage by stage (HIP events, ms): [0] keys   [1] the sort   [2] the cell
 * table (mark, scan, table, seeds)   [3] link   [4] flatten, tally and stats   [5] scatter and hit.
 * gsr_multi_select_connected (below, with the other gsr_multi verbs): rank 0's context, host memory only.
 * Out of scope: adjacency by a world-space radius or by the splats' footprints; more than 1024 cells per axis; a device mask for the
 * multi verb; the GSplatRenderer shim and the HDK glue; gsr_comm_*; an asynchronous form; results left in device memory; moving
 * gsr_select_density's counts onto the cell table. */
#define GSR_CONNECT_SKIP_HIDDEN 1   /* flags: a splat the visibility in force hides is not population */
#define GSR_CONNECT_HIT_OUTSIDE 2   /* flags: a splat outside the grid (that passes the alpha and visibility tests) is hit */
#define GSR_CONNECT_CELLS    1024   /* cells per axis */
#define GSR_CONNECT_MAX_REACH   2
#define GSR_CONNECT_HIST_BINS  32
#define GSR_CONNECT_NO_LABEL 0xFFFFFFFFu   /* labels_out of a splat that is not population */
typedef struct gsr_connect_rule {
    float    cell;                        /* the cells' edge length: finite, > 0, 1.0f / cell finite */
    float    origin[3];                   /* the grid's low corner, upload space */
    int32_t  reach;                       /* 0..GSR_CONNECT_MAX_REACH */
    int32_t  flags;                       /* GSR_CONNECT_* or 0 */
    int32_t  op;                          /* GSR_SELECT_REPLACE .. GSR_SELECT_TOGGLE */
    int32_t  reserved_;                   /* 0 */
    uint32_t size_lo, size_hi;            /* hit iff size_lo <= size <= size_hi */
    float    alpha_min;                   /* population iff a >= alpha_min (-INFINITY: every alpha but a NaN) */
} gsr_connect_rule;
typedef struct gsr_connect_result {
    int64_t n_population, n_outside, n_cells;
    int64_t n_components, n_seeded, largest;
    int64_t comp_hist[GSR_CONNECT_HIST_BINS];
    int64_t splat_hist[GSR_CONNECT_HIST_BINS];
} gsr_connect_result;
int  gsr_select_connected(gsr_context* ctx, const gsr_connect_rule* rule, const uint32_t* seed /* NULL: no seed clause */, int seed_is_device,
                          uint32_t* mask, int mask_is_device, uint32_t* labels_out /* NULL */, uint32_t* sizes_out /* NULL */,
                          int outs_are_device, gsr_connect_result* result /* NULL */, int64_t* n_hit, int64_t* n_set);
int  gsr_select_connected_eval(const gsr_connect_rule* rule, const gsr_visibility* vis /* NULL: none */, int64_t n, const float* P,
                               const float* alpha /* NULL: all 1 */, const uint32_t* seed_bits /* NULL: no seed clause */, uint8_t* hit_out,
                               uint32_t* labels_out /* NULL */, uint32_t* sizes_out /* NULL */,
                               gsr_connect_result* result /* NULL */);   /* host, no context, no GPU */
int  gsr_get_select_connected(gsr_context* ctx, int64_t* calls, int64_t* hit_last, double ms[4]);   /* any pointer may be NULL */
int  gsr_debug_select_connected_stages(gsr_context* ctx, double ms[6]);

/* ---- measuring a selection (counts, bounds, moments and histograms of resident splats, on the GPU) ----------------------------------- */
/* What a mask of gsr_select SAYS besides its bit count: where the selected splats are (a transform gizmo's pivot, "home on selection", a
 * crop box around them), how they lie (nine second moments for a PCA on the host), and how their opacity, size, position and base
 * colour are distributed (the histograms beside gsr_select_attrs' range sliders; a prune threshold) -- without reading P, alpha, scale
 * and Cd back over the link.  One streaming kernel (k_measure.h) in gsr_select's shape, and at most three small launches that finish
 * the sums; a few hundred bytes come back.
 * THE RULE (one set of functions, evaluated by the kernels and by gsr_measure_eval; x86 and gfx950 agree bit for bit).  A splat is
 * SELECTED iff its mask bit is set (a NULL mask: every splat) and, with GSR_MEASURE_SKIP_HIDDEN, the visibility in force does not hide
 * it (gsr_splat_visible on the raw P; no visibility: nothing is hidden).  Everything is computed from what gsr_read returns: the raw P
 * bits, the TRUE alpha, the resident scale and Cd halves.
 *   n_selected  the selected splats.
 *   n_measured  with any bit of `what` set: the selected splats whose three P components are finite (else 0).
 *   n_extent    with GSR_MEASURE_EXTENT: the measured splats whose three scale halves are finite too (else 0).
 *   GSR_MEASURE_BOUNDS   lo[3], hi[3]: the minimum and maximum of P over the measured splats in the TOTAL ORDER OF THE FLOATS' BITS
 *                        (-0 < +0), so the result never depends on which of two equal-comparing values was met first; none measured
 *                        (or the bit not set): +inf / -inf.
 *   GSR_MEASURE_EXTENT   lo_e[3], hi_e[3]: the same over fmaf(-extent_k, smax, p) and fmaf(extent_k, smax, p) of the n_extent splats,
 *                        smax = the largest |half| of the three scale halves as gsr_select_attrs forms it.
 *   GSR_MEASURE_MOMENTS  sum[9]: per measured splat d = p - ref (one float32 subtraction per axis), and the binary64 terms d_x, d_y,
 *                        d_z, d_x d_x, d_x d_y, d_x d_z, d_y d_y, d_y d_z, d_z d_z (each product of two doubles: exact).  Each sum IS
 *                        THE VALUE OF THE PERFECT BINARY TREE OVER UPLOAD INDICES: leaf i holds splat i's term, +0.0 if i is not measured
 *                        or not below n; every inner node is left + right in binary64; the tree spans the smallest 2^k >= max(n, 64)
 *                        leaves.  No floating-point atomic and no re-associated add is involved anywhere, so the nine doubles do not
 *                        depend on the launch shape or on the order the waves run in.  (A sum that overflows to a NaN is a NaN; its
 *                        sign and payload are not specified.)  The bit not set: nine +0.0.
 * HISTOGRAMS: n_hist (0..4) specs; gsr_hist_prepare fills one from doubles: lo and hi rounded to float32, inv_w = (float)(bins /
 * ((double)hi - (double)lo)).  It refuses (GSR_E_INVALID) an unknown channel or flag, bins outside 1..256, non-finite bounds, hi <= lo
 * (as float32), and a range so narrow that inv_w is not finite; gsr_measure refuses a spec that gsr_hist_prepare could not have made
 * in the same way (it does not recompute inv_w).  The DOMAIN is the selected splats, not only the measured ones.  The channel's value
 * x: X / Y / Z the raw P, ALPHA the true alpha, SCALE_MAX / SCALE_MIN the largest / smallest |half| (a NaN half: NaN), CD_R / G / B
 * h2f of the Cd halves.  With GSR_HIST_LOG2 a NaN x counts as nan, x <= 0 as under, +inf as over, and a finite x > 0 is first replaced by
 * (float)(int32_t)(bits(x) - 0x3f800000) * 0x1p-23f -- piecewise-linear in log2, integer and conversion arithmetic only.  Then: NaN ->
 * nan; !(x >= lo) -> under; !(x < hi) -> over; else bin min((int)((x - lo) * inv_w), bins - 1): one float32 subtraction, one float32
 * multiply, a truncation.  hist_out: bins + 3 uint32 per spec -- the bins, then under, over, nan -- the specs back to back.
 * THE MASK is gsr_transform's: ceil(n / 32) words in upload order, host (mask_is_device = 0) or device / pinned memory (1: checked with
 * its exact size before anything is launched), bits at and behind n ignored, never written; NULL: every resident splat.
 * gsr_measure_eval: the rule on the host, no context and no GPU.  Arrays in gsr_read's layout (P float[3n], alpha float[n] TRUE alphas,
 * scale half[3n], Cd half[3n]); an array the request does not look at may be NULL.  mask: host words or NULL; vis (NULL: none in
 * force) is what SKIP_HIDDEN hides by, as gsr_visibility_eval takes it (a mask must cover the n splats).
 * A MEASURE CHANGES AND INVALIDATES NOTHING -- gsr_select's contract: no resident bit, depth horizon, cached depth order, policy or
 * visibility state changes, no entry of gsr_stats; it does not wait for the frames in flight.  ORDERING: gsr_select's (with a device
 * mask the call first waits for the work queued on the public stream); synchronous.  The results always come back to host memory.
 * GSR_E_INVALID, nothing written: NULL ctx, request or result; hist_out NULL with n_hist > 0, or not NULL with n_hist == 0; no geometry
 * ever uploaded, or an upload in progress; unknown bits in what or flags; reserved_ != 0; a non-finite ref or extent_k; n_hist outside
 * 0..4; a bad spec; a device mask that fails the pointer check.  The empty cloud gives GSR_OK with no launch and the EMPTY RESULT:
 * counts 0, lo = +inf, hi = -inf (also of the extent), nine +0.0, every histogram word 0.
 * gsr_get_measure: the calls that measured, n_measured of the last one, and its clock ms[4]:
 * [0] k_measure (HIP events)   [1] the launches that finish the sums (HIP events)   [2] the copies, wall clock   [3] wall clock of the call.
 * gsr_multi_measure (below, with the other gsr_multi verbs): rank 0's context and a host mask -- the cloud is replicated.
 * Out of scope: the GSplatRenderer shim and the HDK glue; gsr_comm_*; a device mask for the multi verb; weighted moments and colour
 * statistics beyond histograms; an asynchronous form, and results left in device memory. */
#define GSR_MEASURE_BOUNDS   1   /* what: lo, hi */
#define GSR_MEASURE_EXTENT   2   /* what: lo_e, hi_e, n_extent */
#define GSR_MEASURE_MOMENTS  4   /* what: sum[9] */
#define GSR_MEASURE_SKIP_HIDDEN 1 /* flags: a splat the visibility in force hides is not selected */
#define GSR_HIST_X           0   /* gsr_hist_spec.channel */
#define GSR_HIST_Y           1
#define GSR_HIST_Z           2
#define GSR_HIST_ALPHA       3
#define GSR_HIST_SCALE_MAX   4
#define GSR_HIST_SCALE_MIN   5
#define GSR_HIST_CD_R        6
#define GSR_HIST_CD_G        7
#define GSR_HIST_CD_B        8
#define GSR_HIST_LOG2        1   /* gsr_hist_spec.flags: bin the piecewise-linear log2 of x */
#define GSR_HIST_MAX_BINS  256
#define GSR_MEASURE_MAX_HIST 4
typedef struct gsr_hist_spec {
    int32_t channel;                      /* GSR_HIST_X .. GSR_HIST_CD_B */
    int32_t flags;                        /* GSR_HIST_LOG2 or 0 */
    int32_t bins;                         /* 1..GSR_HIST_MAX_BINS */
    float   lo, hi;                       /* [lo, hi), finite, lo < hi */
    float   inv_w;                        /* (float)(bins / (hi - lo)) */
} gsr_hist_spec;
typedef struct gsr_measure_request {
    int32_t what;                         /* GSR_MEASURE_BOUNDS | _EXTENT | _MOMENTS (0: the count and the histograms alone) */
    int32_t flags;                        /* GSR_MEASURE_SKIP_HIDDEN or 0 */
    float   ref[3];                       /* the point the moments are taken about, upload space */
    float   extent_k;                     /* the extent reaches extent_k * smax to either side */
    int32_t n_hist;                       /* 0..GSR_MEASURE_MAX_HIST */
    gsr_hist_spec hist[GSR_MEASURE_MAX_HIST];
    int32_t reserved_;                    /* 0 */
} gsr_measure_request;
typedef struct gsr_measure_result {
    int64_t n_selected, n_measured, n_extent;
    float   lo[3], hi[3];                 /* GSR_MEASURE_BOUNDS */
    float   lo_e[3], hi_e[3];             /* GSR_MEASURE_EXTENT */
    double  sum[9];                       /* GSR_MEASURE_MOMENTS: d_x, d_y, d_z, xx, xy, xz, yy, yz, zz */
} gsr_measure_result;
int  gsr_measure(gsr_context* ctx, const uint32_t* mask, int mask_is_device, const gsr_measure_request* request, gsr_measure_result* out,
                 uint32_t* hist_out /* host; NULL iff request->n_hist == 0 */);
int  gsr_measure_eval(const gsr_measure_request* request, const gsr_visibility* vis /* NULL: none */, int64_t n, const uint32_t* mask /* NULL: all */,
                      const float* P, const float* alpha, const uint16_t* scale, const uint16_t* Cd, gsr_measure_result* out,
                      uint32_t* hist_out);   /* host, no context, no GPU */
int  gsr_hist_prepare(int channel, int flags, double lo, double hi, int bins, gsr_hist_spec* out);   /* host */
int  gsr_get_measure(gsr_context* ctx, int64_t* calls, int64_t* measured_last, double ms[4]);   /* any pointer may be NULL */

/* ---- transform: selected resident splats rotated, scaled, translated on the GPU ---- */
/* What a mask of gsr_select is for besides hiding and removing: the selected splats are moved, turned and resized where they are
 * resident -- p' = s R (p - pivot) + pivot + translate -- with their scale, orient and SH coefficients following, and nothing but
 * the mask crosses the link.  One kernel (k_transform.h) in gsr_update's work shape, then gsr_move's re-order pipeline.
 * THE MASK has the layout and sense of gsr_remove's mask and gsr_select's output: bit i & 31 of word i >> 5 is upload index i,
 * ceil(n / 32) words; bits at and behind n are ignored; NULL selects every resident splat.  It may live in host memory
 * (mask_is_device = 0) or in device / pinned memory (1: checked with its exact size before anything is launched, as the device sources
 * are -- a bad pointer gives GSR_E_INVALID, never a fault).  It is never written.
 * gsr_xform_prepare derives the float32 RULE from x, in double, each entry rounded to float once: the quaternion normalised, R, A = s R,
 * t = pivot + translate - (s R) pivot, and the SH band matrices D_l (l = 1, 2, 3): with Y_l(d) the vector of the 2l + 1 polynomials
 * the shader multiplies band l's coefficients with (constants and signs included) at a unit direction d, D_l is the matrix with
 * Y_l(R d)^T D_l = Y_l(d)^T for every d -- a rotated splat shows, from the rotated direction, the colour it showed before.  The
 * identity is not special-cased (and comes out exact).  GSR_E_INVALID: a NULL argument, a non-finite field, scale <= 0, a zero
 * quaternion, reserved_ != 0.
 * THE ARITHMETIC per selected splat (one set of functions, evaluated by the kernel and by gsr_transform_eval; x86 and gfx950 agree bit
 * for bit; every multiply-add one fmaf; the normative statement of each chain heads csrc/k_transform.h):
 *   P       P'.r = fmaf(A[3r], x, fmaf(A[3r+1], y, fmaf(A[3r+2], z, t[r]))) on the raw position bits
 *   scale   each half: f2h(s * h2f(scale_k))
 *   orient  f2h of the quaternion product q (x) orient, the transform first, the resident quaternion as it is (unnormalised, as the
 *           vertex stage uses it).  For a non-unit orient this is what a Transform SOP does to the attribute, not an exact rotation of
 *           the matrix the vertex stage forms from it.
 *   SH      per channel and band, c'_m = f2h(sum_k D_l[m][k] h2f(c_k)), a chain of fmaf with k ascending; coefficient order sh[0..2],
 *           sh[3..7], sh[8..14]; slot 15 of a row, Cd and alpha stay; a cloud without SH has no SH step.
 * An unselected splat keeps every bit.  NaN and infinite inputs follow the arithmetic; a half that comes out NaN is NaN on both sides,
 * sign and payload unspecified.
 * gsr_transform_eval: the same on the host, in place, with no context and no GPU: n rows in gsr_upload's layout (shx, shy, shz all
 * three or none), mask as above (host).  CONTRACT of gsr_transform: after GSR_OK the resident geometry -- the planes, the colour rows,
 * the cluster bounds, the storage order -- is bit for bit what a fresh context holds after gsr_upload of what gsr_read returned
 * before the call, passed through gsr_transform_eval, with the same options, origin and SH presence; so is every later frame.
 * A transform invalidates what a move does (depth horizons, cached depth orders, policies).  A visibility in force is evaluated at the
 * new positions; the true alphas and its mask are kept.  A mask with no bit set below n changes, invalidates and writes nothing.
 * *n_moved (may be NULL): the bits set below n.  gsr_stats.uploads, moves and move_ms are not touched: gsr_get_transform has the calls
 * (one with an empty selection counts, with 0 moved and the clock left as it was), the last count and the clock ms[4], laid out as gsr_get_removal's: [0] the mask over the link
 * [1] the kernel .. the sort of the storage order   [2] the planes into the new order   [3] wall clock of the call.
 * ORDERING: synchronous; waits for the public stream (gsr_set_stream) and for the frames in flight, as the device-source verbs do.
 * MEMORY: the second copy of the planes, as a move keeps it.  Everything is allocated before the first write: GSR_E_OOM leaves the
 * context untouched; a HIP failure after the first write leaves no geometry, as with gsr_move.
 * GSR_E_INVALID, context untouched: NULL ctx or x; what gsr_xform_prepare refuses; no geometry; an upload in progress; a device mask
 * that fails the check.
 * Out of scope: non-uniform scale, shear and reflection (the covariance no longer factors into scale and orient); a shortcut for
 * pure translations; transforming the crop volumes along; the GSplatRenderer shim and the HDK glue; gsr_comm_*; a device mask for
 * gsr_multi_transform; an asynchronous form; a per-splat transform array. */
typedef struct gsr_xform {
    float rotate[4];     /* quaternion (x, y, z, w), orient's order; need not be normalised */
    float scale;         /* uniform, finite, > 0 */
    float translate[3];
    float pivot[3];      /* upload space */
    int32_t reserved_;   /* 0 */
} gsr_xform;
typedef struct gsr_xform_rule {   /* what gsr_xform_prepare derives; float32; 100 dwords */
    float A[9];          /* fl32(s * R), rows */
    float t[3];          /* fl32(pivot + translate - (s R) pivot), formed in double */
    float s;             /* fl32(scale) */
    float q[4];          /* fl32 of the quaternion normalised in double, (i, j, k, r) */
    float D1[9], D2[25], D3[49];   /* SH band matrices, rows */
} gsr_xform_rule;
int  gsr_xform_prepare(const gsr_xform* x, gsr_xform_rule* rule);             /* host, no context, no GPU */
int  gsr_transform_eval(const gsr_xform* x, int64_t n, const uint32_t* mask /* NULL: all */,
                        float* P, uint16_t* scale, uint16_t* orient,
                        uint16_t* shx, uint16_t* shy, uint16_t* shz);         /* host, in place, no GPU */
int  gsr_transform(gsr_context* ctx, const uint32_t* mask, int mask_is_device, const gsr_xform* x, int64_t* n_moved);
int  gsr_get_transform(gsr_context* ctx, int64_t* calls, int64_t* moved_last, double ms[4]);   /* any pointer may be NULL */

/* ---- grade: the colour and the opacity of selected resident splats changed on the GPU ---- */
/* The look of a selection -- exposure, tint / white balance, saturation, contrast, brightness, transparency -- baked into the
 * resident splats a mask selects, with nothing but the mask crossing the link.  The vertex stage forms max(Cd + sum_k Y_k(d) sh_k, 0)
 * per channel, which is linear in (Cd, sh_1 .. sh_15) in front of the clamp: an affine colour map c' = M c + b is therefore baked
 * EXACTLY, from every view direction, by Cd' = M Cd + b and sh_k' = M sh_k for every coefficient.  One kernel (k_grade.h) in
 * gsr_update's work shape, in place: no position changes, so the storage order and the cluster bounds stay.
 * THE MASK is gsr_transform's: bit i & 31 of word i >> 5 is upload index i, ceil(n / 32) words, bits at and behind n ignored, NULL
 * selects every resident splat; host memory (mask_is_device = 0) or device / pinned memory (1: checked with its exact size before
 * anything is launched -- a bad pointer gives GSR_E_INVALID, never a fault).  It is never written.
 * gsr_grade TAKES THE RULE, not the parameters: a caller with a colour matrix of its own (a colour-space change, a hue rotation, a
 * channel swap) fills M, b and the flags itself.  gsr_grade_prepare composes, in double, each entry rounded to float32 once:
 *   c1 = 2^exposure * gain o c;   c2 = L + saturation (c1 - L), L = w . c1, w = (0.2126, 0.7152, 0.0722);
 *   c3 = contrast (c2 - pivot) + pivot + offset
 * i.e. M[r][k] = contrast (saturation [r == k] + (1 - saturation) w_k) 2^exposure gain_k, b[r] = pivot (1 - contrast) + offset[r],
 * ag = alpha_gain, ab = alpha_offset.  It sets GSR_GRADE_COLOUR unless the rounded M is the identity and b is zero, GSR_GRADE_ALPHA
 * unless (ag, ab) == (1, 0).  GSR_E_INVALID: a NULL argument, a field that is not finite, an entry of the rule that does not round to
 * a finite float32.
 * THE ARITHMETIC per selected splat (one set of functions, evaluated by the kernel and by gsr_grade_eval; x86 and gfx950 agree bit for
 * bit; the normative statement heads csrc/k_grade.h), (R, G, B) the three halves of one coefficient, r the channel that comes out:
 *   Cd      f2h(fmaf(M[3r], R, fmaf(M[3r+1], G, fmaf(M[3r+2], B, b[r]))))
 *   SH      coefficients 1..15: f2h(fmaf(M[3r], R, fmaf(M[3r+1], G, M[3r+2] * B))); slot 15 of a row stays; no SH step without SH
 *   alpha   min(max(fmaf(ag, alpha, ab), 0), 1) on the TRUE alpha; a NaN becomes 0
 * A step whose flag is clear does not run at all, and a rule without flags is a no-op.  The colour step under the identity is NOT one:
 * a -0 half becomes +0 and an infinite half turns its coefficient NaN -- which is why gsr_grade_prepare clears the flag.  An unselected
 * splat keeps every bit.  Non-finite halves follow the arithmetic; a half that comes out NaN is NaN on both sides.
 * gsr_grade_eval: the same on the host, in place, with no context and no GPU: n rows in gsr_upload's layout; has_sh = 0: shx, shy, shz
 * are not looked at.  CONTRACT of gsr_grade: after GSR_OK the resident geometry is bit for bit what a fresh context holds after
 * gsr_upload of what gsr_read returned before the call, passed through gsr_grade_eval, with the same options, origin, SH presence
 * and visibility; so is every later frame.
 * INVALIDATION is gsr_update's: a colour-only grade drops the cached depth orders and keeps horizons, prefixes and policies; one
 * with GSR_GRADE_ALPHA is a change of shape, like new alphas.  A VISIBILITY in force: the true alphas kept aside are graded, and the
 * rule in force is applied again -- a hidden splat stays +0.0f with its graded alpha aside, and gsr_read returns the graded alphas.
 * EMPTY WORK -- no bit set below n, a rule without flags, no splat resident -- changes, invalidates and writes nothing, and counts as
 * a call.  *n_graded (may be NULL): the bits set below n; 0 for a rule without flags.  gsr_get_grade has the calls that passed their
 * refusals, the last count and the clock ms[4] of the last call that wrote: [0] the mask over the link and its count  [1] the kernel
 * (HIP events)  [2] the visibility rule applied again  [3] wall clock of the call.
 * ORDERING: synchronous; waits for the public stream (gsr_set_stream) and for the frames in flight.  MEMORY: the staging arena (the
 * mask's copy); no spare planes.  GSR_E_INVALID, context untouched: NULL ctx or rule; a float of the rule that is not finite; an
 * unknown flag bit; no geometry; an upload in progress; a device mask that fails the check.
 * Out of scope: maps that are not affine in colour (gamma, curves, hue selection by range); per-splat rules; the GSplatRenderer shim
 * and the HDK glue; gsr_comm_*; a device mask for gsr_multi_grade; an asynchronous form; undo (a caller can invert an invertible M
 * itself, but the roundings to halves do not invert). */
#define GSR_GRADE_COLOUR 1u
#define GSR_GRADE_ALPHA  2u
typedef struct gsr_grade_params {      /* what a user turns; every field finite, else GSR_E_INVALID */
    float exposure;                    /* stops: colour x 2^exposure                    (neutral 0) */
    float gain[3];                     /* tint / white balance, per channel             (neutral 1,1,1) */
    float saturation;                  /* 0 = grey, 1 = as is, > 1 more; Rec.709 luma weights (0.2126, 0.7152, 0.0722) */
    float contrast, pivot;             /* c -> contrast (c - pivot) + pivot             (neutral 1, any pivot) */
    float offset[3];                   /* added last: brightness / lift                 (neutral 0,0,0) */
    float alpha_gain, alpha_offset;    /* opacity -> clamp(alpha_gain * alpha + alpha_offset, 0, 1)   (neutral 1, 0) */
} gsr_grade_params;
typedef struct gsr_grade_rule {        /* what the kernel evaluates: 15 dwords */
    float M[9];                        /* rows */
    float b[3];
    float ag, ab;
    uint32_t flags;                    /* GSR_GRADE_COLOUR | GSR_GRADE_ALPHA: which of the two steps run */
} gsr_grade_rule;
int  gsr_grade_prepare(const gsr_grade_params* p, gsr_grade_rule* rule);          /* host, no context, no GPU */
int  gsr_grade_eval(const gsr_grade_rule* rule, int64_t n, const uint32_t* mask /* NULL: all */, int has_sh,
                    uint16_t* Cd, float* alpha, uint16_t* shx, uint16_t* shy, uint16_t* shz);   /* host, in place, no GPU */
int  gsr_grade(gsr_context* ctx, const uint32_t* mask, int mask_is_device, const gsr_grade_rule* rule, int64_t* n_graded);
int  gsr_get_grade(gsr_context* ctx, int64_t* calls, int64_t* graded_last, double ms[4]);      /* any pointer may be NULL */

/* ---- multi-GPU: tile-row shard ------------------------------------------ */
/* This context renders only the tile rows of shard `index` of `count`: rows r with r % count == index (layout 0,
 * interleaved: balances any scene) or the contiguous band [index*rpb, (index+1)*rpb), rpb = ceil(tile rows / count)
 * (layout 1, GSR_OPT_SHARD_LAYOUT: a rank keeps ~1/count of the splats, so its sort/binning/colour work shrinks too).
 * Its output is the compact band image: the owned tile rows stacked bottom-up, gsr_band_rows() pixel rows of `width`
 * pixels of the context's target format.  The stitched frame is bit-identical to the unsharded one in either layout.  The band is padded to the
 * same height on every rank: pixel rows behind the rank's last image row (a last tile row the image does not fill, whole
 * tile rows of a rank that owns fewer than the others, all of it for a rank beyond the image) are NEVER written in a
 * device target -- clear it once if they are to read as zeros -- and read as zeros in a host target. */
int  gsr_set_row_shard(gsr_context* ctx, int index, int count);
int  gsr_band_rows(int height, int index, int count);      /* pixel rows in that band image */
/* An EXPLICIT band: this context renders only the tile rows [first_tile_row, first_tile_row + tile_rows) of the image -- a
 * contiguous band of any extent, wherever it begins (layout 1's bands are the special case first = index * rpb).  Rows beyond
 * the image are owned but empty; tile_rows = 0 is a rank that owns nothing: its frame is GSR_OK, runs nothing and writes
 * nothing.  The band image is tile_rows * GSR_TILE pixel rows of `width` pixels of the target format; row 0 is the bottom
 * pixel row of tile row first_tile_row.  Padding as above: pixel rows beyond the image are never written in a device target
 * and read as zeros in a host target.  Every frame verb works in a band (gsr_render, _depth, _aov, _over: the depth buffer and
 * the background image are the FULL image, the outputs are the band, as for a row-sharded context), in every target format
 * and option mode.  The band may change between frames: it is a new tile geometry, so the tile table is rebuilt (which
 * synchronises) and depth horizons, tile orders and cached depth orders of the old band are dropped.  gsr_set_row_shard cancels
 * an explicit band, gsr_set_row_band cancels a row shard.  gsr_band_rows and gsr_stitch_bands do not know explicit bands: a
 * band is a block of image rows, so placing it is a row copy.
 * GSR_E_INVALID, context untouched: NULL ctx, a negative argument, first_tile_row + tile_rows > GSR_MAX_DIM / GSR_TILE, a
 * context that holds a communicator (gsr_comm_init: out of scope -- one process per GPU would need an all-gather of the row
 * sums per evaluation). */
int  gsr_set_row_band(gsr_context* ctx, int first_tile_row, int tile_rows);
/* GSR_OPT_ROW_WORK: the newest complete set of per-tile-row work sums and the ordinal of the frame it belongs to (1-based, as
 * the context counts the frames it rendered; frame_out may be NULL).  out[r], r < n_rows = ceil(height / GSR_TILE) of that
 * frame, is the saturating sum over the tiles of GLOBAL tile row r of the blend kernel's per-tile work (wave-record
 * evaluations * 32 + records gathered * 8 + list entries scanned / 2; both phases of a front-slab frame; of a repaired or
 * re-queued frame, the attempt that produced the pixels); 0 for rows the context does not own.  Blend work only: a rank's
 * front-end floor is not in it.  Synchronises like gsr_get_stats (the frames themselves never wait for the sums: they arrive
 * in mapped host memory, every word stamped with the frame's ticket).  GSR_E_INVALID: the option is off, no frame has run with
 * it, or n_rows is not that frame's. */
int  gsr_read_row_work(gsr_context* ctx, uint32_t* out, int n_rows, int64_t* frame_out);
/* The balancer behind GSR_OPT_SHARD_LAYOUT = 2, a pure host function (no context, no GPU).  row_work[tiles_y] -> the
 * boundaries out_first[count + 1] (band g = tile rows [out_first[g], out_first[g + 1]); out_first[0] = 0, out_first[count] =
 * tiles_y) of the contiguous partition into `count` bands whose LARGEST band sum (64-bit) is smallest; every band gets at
 * least one row while tiles_y >= count (with count > tiles_y the trailing bands are empty).  Among the optimal partitions the
 * one whose interior boundaries are closest to layout 1's equal split e[g] = min(g * ceil(tiles_y / count), tiles_y) is
 * chosen, boundary by boundary from the first: smallest |out_first[g] - e[g]|, the smaller boundary on a tie.  All-zero work
 * gives e (made feasible: at least one row per band) itself.
 * Hysteresis: with cur_first (a valid partition) the proposal is adopted only if its largest band sum is at most
 * (1000 - min_gain_permille) / 1000 of cur_first's under the same row_work; otherwise out_first = cur_first.
 * Returns 1 = out_first differs from cur_first (always 1 without cur_first), 0 = kept, negative (GSR_E_INVALID) = bad
 * argument: NULL row_work / out_first, tiles_y < 1 or > GSR_MAX_DIM / GSR_TILE, count < 1 or > 64, min_gain_permille outside
 * 0..1000, a cur_first that is not a monotone cover of [0, tiles_y). */
int  gsr_debug_balance_rows(const uint32_t* row_work, int tiles_y, int count, const int32_t* cur_first,
                            int min_gain_permille, int32_t* out_first);
/* Root side: bands[count] gathered back to back (each padded to
 * gsr_band_rows(height, 0, count) rows) -> full image.  Device pointers; pixels of ctx's target format (set the format the
 * ranks render in on the stitching context too): a row copy, never a conversion. */
int  gsr_stitch_bands(gsr_context* ctx, const float* gathered, int count,
                      int width, int height, float* rgba_out);

/* ---- several GPUs, one caller thread -------------------------------------- */
/* The reference draws from Houdini's single draw thread (src/DM_GSplatHook.C:30-39); gsr_multi drives G contexts -- one
 * per GPU, splats replicated, rank g owning a contiguous band of tile rows (GSR_OPT_SHARD_LAYOUT = 1 is gsr_multi's
 * default; 0 = interleaved rows) -- on behalf of that one thread: every rank's frame is queued by a worker thread of its
 * own (GSR_MULTI_THREADS=0 in the environment: by the caller's thread, one rank after the other), then the caller's thread
 * issues the frame's ONE collective: ncclRecv x (G-1) + ncclSend per peer in one group (RCCL over xGMI) on per-rank
 * transfer streams.  With the band layout the peers' bands are received straight into rgba_out (a band is a block of rows
 * of the final image); with interleaved rows they are de-interleaved on the root.  Bands are double-buffered, so the
 * gather of frame f overlaps the kernels of frame f+1.  The result is bit-identical to the 1-GPU frame. */
typedef struct gsr_multi gsr_multi;
#define GSR_TRANSPORT_AUTO   0   /* RCCL when the devices are distinct (and librccl loads), else COPY */
#define GSR_TRANSPORT_RCCL   1   /* single-process communicator (ncclCommInitAll) */
#define GSR_TRANSPORT_COPY   2   /* hipMemcpyPeerAsync / device-to-device copies ordered by events: several contexts on ONE
                                    GPU (how the 1-GPU test box runs the whole path), or a fallback without RCCL */
int  gsr_multi_create(const int* devices, int count, int transport, gsr_multi** out);   /* devices may repeat for COPY */
void gsr_multi_destroy(gsr_multi* m);
int  gsr_multi_count(gsr_multi* m);
int  gsr_multi_transport(gsr_multi* m);                       /* the transport in use (GSR_TRANSPORT_RCCL / _COPY) */
gsr_context* gsr_multi_context(gsr_multi* m, int rank);      /* rank's context (stats, debug access); do not destroy */
int  gsr_multi_set_stream(gsr_multi* m, void* hip_stream);   /* the stream on devices[0] that frames are ORDERED on (the
                                                                 ranks' kernels and the gather run on streams of the library) */
int  gsr_multi_set_option(gsr_multi* m, int option, int value);
int  gsr_multi_set_target_format(gsr_multi* m, int format);   /* every rank and the root (gsr_set_target_format); synchronises */
/* what RCCL itself reports: ranks_out[g] = ncclCommUserRank of rank g's communicator, *nranks_out = ncclCommCount of the
 * root's (-1 / 0 with the COPY transport) */
int  gsr_multi_comm_info(gsr_multi* m, int* ranks_out, int* nranks_out);
/* the gather on the root's transfer stream, from the first receive to "frame complete", measured with HIP events:
 * enable = 1 / 0 switches the measurement (and clears the sums when it changes), -1 leaves it; returns the sums so far.
 * Synchronises. */
int  gsr_multi_gather_stats(gsr_multi* m, int enable, double* ms_total, int64_t* gathers);
int  gsr_multi_upload_begin(gsr_multi* m, int64_t total_splats, int has_sh, const float origin[3]);
int  gsr_multi_upload_append(gsr_multi* m, int64_t n, const float* P, const uint16_t* Cd, const float* alpha,
                             const uint16_t* scale, const uint16_t* orient,
                             const uint16_t* shx, const uint16_t* shy, const uint16_t* shz);
int  gsr_multi_upload_end(gsr_multi* m);
int  gsr_multi_upload_abort(gsr_multi* m);
int  gsr_multi_upload(gsr_multi* m, int64_t n, const float* P, const uint16_t* Cd, const float* alpha,
                      const uint16_t* scale, const uint16_t* orient,
                      const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, const float origin[3]);
/* gsr_update on every rank (the cloud is replicated); synchronises the frames and the gather in flight first */
int  gsr_multi_update(gsr_multi* m, int64_t first, int64_t n, const gsr_attr_update* u);
/* gsr_move on every rank, after the same synchronisation (every rank then keeps its own second copy of the planes) */
int  gsr_multi_move(gsr_multi* m, int64_t first, int64_t n, const float* P, const float origin[3], const gsr_attr_update* u);
/* gsr_set_visibility on every rank, after the same synchronisation (every rank keeps its own copy of the alphas and of a mask) */
int  gsr_multi_set_visibility(gsr_multi* m, const gsr_visibility* v);
/* gsr_remove on every rank, after the same synchronisation, from a HOST mask (NULL with GSR_REMOVE_HIDDEN alone).  The ranks must
 * agree on the splats left: if they do not, or a rank fails after its first write, the verb fails and NO rank keeps geometry.  The
 * boundaries of balanced bands stay as after an upload: the next evaluation reads the survivors' row sums. */
int  gsr_multi_remove(gsr_multi* m, const uint32_t* mask_host, int flags, int64_t* n_left);
/* gsr_add on every rank, after the same synchronisation, from HOST arrays.  The ranks must agree on the total: if they do not, or a
 * rank fails after its first write, the verb fails and NO rank keeps geometry.  The boundaries of balanced bands stay as after an
 * upload. */
int  gsr_multi_add(gsr_multi* m, int64_t n_new, const float* P, const uint16_t* Cd, const float* alpha, const uint16_t* scale,
                   const uint16_t* orient, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, int64_t* n_total);
/* gsr_read of rank 0's copy (the cloud is replicated), after the same synchronisation; no rank's state changes */
int  gsr_multi_read(gsr_multi* m, int64_t first, int64_t n, const gsr_read_arrays* out);
/* gsr_select on rank 0's copy (the cloud is replicated) into a HOST mask, after the same synchronisation; no rank's state changes */
int  gsr_multi_select(gsr_multi* m, const gsr_camera* cam, const gsr_select_region* region, uint32_t* mask_host,
                      int64_t* n_hit, int64_t* n_set);
/* gsr_select_attrs on rank 0's copy (the cloud is replicated) into a HOST mask, after the same synchronisation; no rank's state changes */
int  gsr_multi_select_attrs(gsr_multi* m, const gsr_attr_rule* rule, uint32_t* mask_host, int64_t* n_hit, int64_t* n_set);
/* gsr_select_density on rank 0's copy into a HOST mask and HOST counts (NULL: skipped), after the same synchronisation; no rank's state changes */
int  gsr_multi_select_density(gsr_multi* m, const gsr_density_rule* rule, uint32_t* mask_host, uint32_t* counts_host /* NULL */,
                              gsr_density_result* result /* NULL */, int64_t* n_hit, int64_t* n_set);
/* gsr_select_connected on rank 0's copy, HOST memory only (seed, labels and sizes may be NULL), after the same synchronisation; no rank's state changes */
int  gsr_multi_select_connected(gsr_multi* m, const gsr_connect_rule* rule, const uint32_t* seed_host /* NULL */, uint32_t* mask_host,
                                uint32_t* labels_host /* NULL */, uint32_t* sizes_host /* NULL */, gsr_connect_result* result /* NULL */,
                                int64_t* n_hit, int64_t* n_set);
/* gsr_measure on rank 0's copy (the cloud is replicated) from a HOST mask (NULL: every splat), after the same synchronisation; no rank's state changes */
int  gsr_multi_measure(gsr_multi* m, const uint32_t* mask_host, const gsr_measure_request* request, gsr_measure_result* out, uint32_t* hist_out);
/* gsr_transform on every rank, after the same synchronisation, from a HOST mask (NULL: every splat).  gsr_multi_remove's agreement
 * rule: if the ranks do not agree on the count, or a rank fails after its first write, the verb fails and NO rank keeps geometry. */
int  gsr_multi_transform(gsr_multi* m, const uint32_t* mask_host, const gsr_xform* x, int64_t* n_moved);
/* gsr_grade on every rank's replica, after the same synchronisation, from a HOST mask (NULL: every splat), under the same agreement
 * rule: ranks that do not agree on the count, or a rank that fails after its first write, and NO rank keeps geometry. */
int  gsr_multi_grade(gsr_multi* m, const uint32_t* mask_host, const gsr_grade_rule* rule, int64_t* n_graded);
/* gsr_read_masked of rank 0's copy (the cloud is replicated), from a HOST mask (NULL: every splat) into host arrays, after the same
 * synchronisation; no rank's state changes */
int  gsr_multi_read_masked(gsr_multi* m, const uint32_t* mask_host, int64_t max_rows, const gsr_read_arrays* out, int64_t* n_rows);
/* gsr_duplicate on every rank's replica, after the same synchronisation, from a HOST mask (NULL: every splat), under gsr_multi_add's
 * agreement rule: ranks that do not agree on the total, or a rank that fails after its first write, and NO rank keeps geometry. */
int  gsr_multi_duplicate(gsr_multi* m, const uint32_t* mask_host, int64_t* n_copied, int64_t* n_total);
/* The agreement rule of those five verbs, a pure host function (no context, no GPU).  rc: what the ranks returned together (the
 * first failure, GSR_OK if none); counts[ranks * per_rank]: rank g's per_rank counts at [g * per_rank ..], -1 where the rank did
 * not return GSR_OK (a rank writes them only then).  *verdict =
 *   GSR_REPLICA_KEEP_REFUSAL  rc is a refusal (not GSR_E_HIP) and no rank has a count: every rank refused before its first write,
 *                             the replicas are what they were, and the verb returns rc;
 *   GSR_REPLICA_AGREED        rc == GSR_OK and every rank's counts equal rank 0's: the verb returns rank 0's counts;
 *   GSR_REPLICA_DROP_ALL      anything else (GSR_E_HIP may have come behind a rank's first write): every rank drops its geometry.
 * Returns GSR_E_INVALID for NULL counts / verdict, ranks < 1 or per_rank < 1. */
#define GSR_REPLICA_KEEP_REFUSAL 0
#define GSR_REPLICA_AGREED       1
#define GSR_REPLICA_DROP_ALL     2
int  gsr_debug_replica_verdict(int rc, int ranks, int per_rank, const int64_t* counts, int* verdict);
/* full frame on devices[0] (device pointer there, asynchronous, ordered on the stream of gsr_multi_set_stream) or in host
 * memory (synchronous): height*width pixels of the target format */
int  gsr_multi_render(gsr_multi* m, const gsr_camera* cam, float* rgba_out, int out_is_device);
int  gsr_multi_render_depth(gsr_multi* m, const gsr_camera* cam, const float* depth, int depth_is_device,
                            float* rgba_out, int out_is_device);
int  gsr_multi_synchronize(gsr_multi* m);
int  gsr_multi_get_stats(gsr_multi* m, int rank, gsr_stats* out);
/* BALANCED BANDS, gsr_multi_set_option(m, GSR_OPT_SHARD_LAYOUT, 2): contiguous bands like layout 1, but their boundaries follow
 * the blend work.  Every rank runs with GSR_OPT_ROW_WORK; the frames start from the equal split; every GSR_MULTI_BALANCE_PERIOD
 * frames the ranks' newest row sums are merged (each rank contributes the rows it owns; nothing waits: a rank whose set has not
 * arrived leaves the evaluation to the next period), gsr_debug_balance_rows proposes a partition, and if it cuts the heaviest
 * band by at least GSR_MULTI_BALANCE_GAIN permille every rank gets its new band with gsr_set_row_band.  A rebalance costs a
 * synchronisation, a tile-table rebuild and every rank's depth horizons -- hence the period and the gain.  The gather follows the
 * bands of the frame it gathers (per-rank rows and counts).  Pixels are the 1-GPU frame's, bit for bit.
 * gsr_multi_get_bands: first[count + 1] = the boundaries of the last frame in tile rows (layout 1: the equal split; layout 0:
 * GSR_E_INVALID), *rebalances = how often they have changed (either may be NULL).
 * Out of scope: gsr_comm_* (one process per GPU); balancing by anything but blend work (the per-rank front-end floor is not in the
 * tile weights); the GSplatRenderer shim and the HDK glue keep gsr_multi's default layout 1; there is no stitch kernel for
 * unequal bands (none is needed: a band is a block of rows). */
#define GSR_MULTI_BALANCE_PERIOD 24     /* frames between two evaluations (LAB_NOTES.md, "Balanced bands": a rebalance costs 1.3 frame
                                           times once the buffers exist, 5 the first time, and wins ~5 % of T1's heaviest band) */
#define GSR_MULTI_BALANCE_GAIN   150    /* permille by which a proposal must cut the heaviest band's work sum (T1 at 4 ranks: 250) */
int  gsr_multi_get_bands(gsr_multi* m, int32_t* first, int64_t* rebalances);

/* ---- one process per GPU (torchrun-style launches): the same gather ----------- */
/* The launcher hands every rank the 128-byte id rank 0 obtained (any side channel); after gsr_comm_init a frame is one
 * call per rank: the rank's band is rendered (in the context's target format: set the same one on every rank), sent (ncclSend) or received (root: straight into rgba_out_device with the
 * band layout, stitched there with interleaved rows).  With world > 1 the context's kernels move to a stream of the
 * library and the collective to a second one (the gather of frame f overlaps frame f+1); the frame is ORDERED on the
 * context's public stream (gsr_set_stream, before or after gsr_comm_init).  rgba_out_device is the FULL frame on the root
 * and ignored elsewhere. */
#define GSR_COMM_ID_BYTES 128
int  gsr_comm_available(void);                       /* 1 if librccl could be loaded in this process (no GPU work) */
int  gsr_comm_get_unique_id(void* id);
int  gsr_comm_init(gsr_context* ctx, const void* id, int rank, int world);   /* collective; sets the row shard (rank, world) */
int  gsr_comm_info(gsr_context* ctx, int* rank, int* nranks);               /* ncclCommUserRank / ncclCommCount */
int  gsr_comm_destroy(gsr_context* ctx);
int  gsr_comm_render(gsr_context* ctx, const gsr_camera* cam, const float* depth, int depth_is_device,
                     float* rgba_out_device);

/* ---- per frame ---------------------------------------------------------- */
/* Renders the uploaded splats.  rgba_out: rows*width pixels of the context's target format
 * (float[rows*width*4] by default), premultiplied RGBA, row 0 = BOTTOM row (GL window coordinates), cleared to 0 -- what the
 * reference's blend leaves in an initially transparent float target.  rows =
 * height, or gsr_band_rows() when sharded.  out_is_device: 0 = host pointer
 * (synchronous), 1 = device pointer: asynchronous, ordered on the context's public stream
 * (gsr_set_stream); the call itself only waits for the frame's 4-byte pair count, which the GPU
 * delivers mid-frame while it keeps working (GSR_OPT_DEFERRED_CHECK removes that wait too). */
int  gsr_render(gsr_context* ctx, const gsr_camera* cam, float* rgba_out, int out_is_device);

/* Same frame, depth-tested against what is already in the viewport: the reference draws
 * after Houdini's opaque pass with the depth test on and depth writes off (src/GSplatRenderer.C:595-610).
 * depth: float[height*width] window-space depth (0..1, row 0 = bottom) of the FULL image (also when
 * sharded), host or device pointer; NULL = no test.  A fragment survives iff the splat's window depth
 * (one value per quad, ndc.z*0.5+0.5) <= depth[pixel]. */
int  gsr_render_depth(gsr_context* ctx, const gsr_camera* cam, const float* depth, int depth_is_device,
                      float* rgba_out, int out_is_device);

/* ---- depth AOV ----------------------------------------------------------
 * gsr_render_depth plus one plane beside the image.  GSR_AOV_DEPTH: per pixel two float32 {zsum, cov}, 8 bytes, ALWAYS float32
 * whatever the context's target format; rows*width pixels, row 0 = bottom, like the image (a row-sharded context writes its band
 * plane, gsr_band_rows() rows, padded like the band image).
 *   zsum = sum of w_i * zwin_i over exactly the fragments the image composites, nearest first, with the same weights w = T*alpha
 *          (same discard, same per-pixel early-out, same depth test), accumulated as Z = fma(w, zwin, Z);
 *          zwin = the quad's window depth (ndc.z*0.5+0.5), the value the depth test compares;
 *   cov  = 1 - T: the bits of the RGBA32F image's alpha.
 * A pixel nothing covers holds {0, 0}.  The image is bit-identical to gsr_render_depth's.  aov_out lives where rgba_out lives
 * (out_is_device); a device pointer must be 8-byte aligned.  aov = 0 or aov_out = NULL: gsr_render_depth itself; an unknown aov:
 * GSR_E_INVALID.
 * Not covered: gsr_multi_* and gsr_comm_* have no AOV verb (nothing is gathered); gsr_stitch_bands does not know the plane (a band
 * plane stitches like a band image, by copying each rank's rows of tiles to where they belong); the wire overlay writes none. */
#define GSR_AOV_DEPTH 1
int  gsr_render_aov(gsr_context* ctx, const gsr_camera* cam, const float* depth, int depth_is_device,
                    float* rgba_out, int out_is_device, int aov, float* aov_out);
/* The plane -> a window-depth buffer gsr_render_depth (or GL) accepts: per pixel
 *   cov >= cov_min ? min(zsum / cov, 1) : 1      (IEEE division; 1 = the far plane, what a cleared depth buffer holds)
 * Host form: no context, no GPU.  Device form: one small kernel on the context's public stream, the same function. */
int  gsr_resolve_depth(const float* aov, int64_t n_pixels, float cov_min, float* depth_out);
int  gsr_resolve_depth_device(gsr_context* ctx, const float* aov, int64_t n_pixels, float cov_min, float* depth_out);

/* ---- background ----------------------------------------------------------
 * gsr_render_depth composited over a premultiplied background -- a colour, or an image of the frame's size -- inside the blend
 * kernel: the target holds the rounded FINAL picture (one rounding in a packed format, no full-frame pass behind the frame).
 * With S = the f32 pixel of gsr_render_depth (S_a = 1 - T) and B = the background pixel decoded to f32:
 *   k = 1.0f - B_a;   out_c = fmaf(k, S_c, B_c)   for c = r, g, b, a;   then the target format's store rule.
 * That is the reference's blend function (ONE_MINUS_DST_ALPHA, ONE; src/GSplatRenderer.C:613-621) applied once to the finished
 * pixel; the reference applies it per fragment into a target that is not empty -- algebraically the same, rounded differently.
 * A pixel no splat covers, and a pixel under B_a == 1, get B exactly.  The background is the caller's data and is not sanitised
 * (the 8-bit store maps NaN to 0).  Image pixels decode as: RGBA32F as is; RGBA16F binary16 -> f32 (exact); RGBA8 (float)byte / 255.0f
 * (an IEEE division).  The image's format is independent of the context's target format.
 * NaN: where the rule yields NaN (a NaN operand, 0 * inf under an infinite B_a, inf - inf) the target's channel is NaN exactly where
 * gsr_composite_over's is, with sign and payload unspecified; every other channel is bit-exact, and RGBA8 is bit-exact throughout.
 * The image lives on either side whatever the target: a host image is copied when the call is made; a DEVICE image is read in
 * place, must be aligned to its pixel size and must stay valid and unchanged until the frame completes on the public stream.
 * There is NO in-place form (a device image whose bytes overlap a device rgba_out: GSR_E_INVALID): a frame can be composited more
 * than once before it is final -- a repair after a broken horizon, a re-queue after the pair count outgrew the lists, a re-sort,
 * a guard miss -- and every attempt must read the original background.
 * bg = NULL or kind = 0: gsr_render_depth itself, bit for bit, the same launches.  GSR_E_INVALID: an unknown kind or image format,
 * a NULL image, a misaligned or overlapping device image.
 * Not covered: there is no AOV + background verb; gsr_multi_*, gsr_comm_* and the wire overlay take no background.  A row-sharded
 * context composites its band over its own rows of the FULL image (padding rows as ever: never written in a device target, zero
 * in a host target), so stitched bands are the unsharded over-frame. */
#define GSR_BG_COLOUR 1
#define GSR_BG_IMAGE  2
typedef struct gsr_background {
    int32_t kind;             /* 0 = none: the verb is gsr_render_depth itself */
    int32_t format;           /* GSR_BG_IMAGE: GSR_TARGET_* of the image's pixels (independent of the context's target format) */
    float   rgba[4];          /* GSR_BG_COLOUR: premultiplied */
    const void* image;        /* GSR_BG_IMAGE: height*width pixels of the FULL image (also when row-sharded, like `depth`), row 0 = bottom */
    int32_t image_is_device;
    int32_t reserved_;
} gsr_background;
int  gsr_render_over(gsr_context* ctx, const gsr_camera* cam, const float* depth, int depth_is_device,
                     const gsr_background* bg, float* rgba_out, int out_is_device);
/* The rule on the host (no context, no GPU), through the very functions the kernel composites and stores with: n_pixels RGBA-f32
 * pixels over bg (a HOST image of n_pixels pixels, or a colour) -> out_format.  What the tests hold the GPU path to. */
int  gsr_composite_over(const float* rgba32f, int64_t n_pixels, const gsr_background* bg,
                        int out_format, void* out);

/* Wireframe overlay (the reference's wire program, shaders/GSplatShaderSource.h:22-110 drawn in
 * src/GR_GSplat.C:477-483): the outline of every splat's +-2 quad in colour Cd, alpha 1, nearest line wins,
 * background 0, in the context's target format (Cd is stored as halves: RGBA16F gets those bits).  Whole image (ignores the row shard), synchronous.  Like the reference's wire program it uses
 * P without the GSplatOrigin round trip and no object matrix in the covariance. */
int  gsr_render_wire(gsr_context* ctx, const gsr_camera* cam, float* rgba_out, int out_is_device);
/* Wire-OVER display: the reference draws the outlines and still includes the primitive in the splat pass
 * (src/GR_GSplat.C:471-486), so shaded + wire shows both.  The outlines are written on top of the frame that is
 * already in rgba_inout (a finished gsr_render / gsr_render_depth target of the same size and format); pixels no outline
 * covers keep their value. */
int  gsr_render_wire_over(gsr_context* ctx, const gsr_camera* cam, float* rgba_inout, int is_device);

/* ---- selection overlay (k_marks.h) ------------------------
 * SHOW a selection: the splats a mask selects (gsr_select's and gsr_select_attrs' output; NULL: every splat) are drawn into the
 * finished frame in rgba_inout -- the camera's size, the context's target format -- as centre dots or as the outlines of their +-2
 * quads, nearest first, in a fixed colour or their own Cd.  On the GPU throughout: with a device mask and a device target nothing
 * crosses the link.  Whole image (ignores the row shard), synchronous, a device target aligned to its pixel: gsr_render_wire_over's
 * rules.
 * THE RULE.  A DOT is drawn for upload index i iff its mask bit is set, gsr_select_hit says hit for the rect (-inf, -inf, +inf, +inf)
 * with no image and no depth -- the vertex stage's centre (cx, cy, zw), the clip test and the opacity test on the RESIDENT opacity
 * (GSR_MARK_ANY_OPACITY = GSR_SELECT_ANY_OPACITY drops it), NaN meaning no hit -- and 0 <= cx < W && 0 <= cy < H.  Its fragments are
 * the pixels [qx - r, qx + r] x [qy - r, qy + r] clipped to the image, qx = (int)cx, qy = (int)cy, r = radius.  An OUTLINE is drawn
 * iff its mask bit is set and (GSR_MARK_ANY_OPACITY is given or the resident a >= 1.0f / 255.0f); its fragments are exactly the wire
 * overlay's for that splat (its clip test, its covariance axes, its four edges).  Every fragment carries the key
 * (bits(zw) << 32) | i; per pixel the smallest key wins: nearest first, the lower upload index on equal depth.  A pixel with a
 * winner (zw, i) is left untouched under a depth buffer unless zw <= depth[p] + depth_bias (one f32 add, one compare; the winner has
 * the pixel's smallest zw, so this is the per-fragment test).  Otherwise c = style.rgba, or (Cd_i.rgb, 1) as the wire overlay colours
 * a line; D = the target pixel decoded by the background's rule (RGBA32F as is, binary16 exact, RGBA8 (float)byte / 255.0f); each
 * channel is out = fmaf(1 - c.a, D, c), through the function gsr_composite_over composites with, stored by the target format's
 * store.  Every other pixel keeps its bytes; *n_pixels (may be NULL) = the pixels written.
 * CONSEQUENCES.  Radius-0 dots write exactly the centre pixels of the splats gsr_select hits with the same mask as prior, the same
 * depth clause and GSR_SELECT_INTERSECT.  A NULL mask with OUTLINE and COLOUR_CD is the wire-over display that honours the visibility
 * in force (with GSR_MARK_ANY_OPACITY, over a finite frame: gsr_render_wire_over's bytes).  The verb changes and invalidates nothing the context keeps --
 * gsr_select's contract, gsr_stats included -- and a context that never calls it launches nothing new.
 * mask: ceil(n / 32) words, host or device / pinned memory.  style.depth: float[height * width] window depths as gsr_render_depth
 * takes them, a host buffer copied when the call is made, a device buffer read in place.  ORDERING: like gsr_render_wire_over the
 * call first waits for the frames in flight and for the work queued on the public stream, so a device mask, depth buffer or frame
 * produced there is complete.  Every device pointer is checked (gsr_upload_append_device's test) before anything is launched.
 * GSR_E_INVALID, nothing written: a NULL ctx, camera, style or target; no geometry, or an upload in progress; a bad frame size, shape,
 * radius or colour mode; unknown flag bits; a non-finite rgba or an alpha outside [0, 1] (FIXED); reserved_ != 0; a misaligned
 * device target; a device pointer that fails the check.  The empty cloud and an all-clear mask: GSR_OK, 0 pixels, the target
 * byte-identical.
 * gsr_get_marks: the calls that drew, the pixels the last one wrote, and its clock ms[4]: [0] the z-buffer clear and k_mark,
 * [1] k_mark_resolve (HIP events both), [2] the copies over the link (a host mask, depth buffer or frame), [3] wall clock.
 * NOT COVERED: gsr_multi_* and gsr_comm_*, the GSplatRenderer shim and the HDK glue; a filled or tinted footprint in the beauty pass;
 * an asynchronous form; an AOV. */
#define GSR_MARK_DOT      1   /* a (2r+1)^2 square of pixels around the centre's pixel */
#define GSR_MARK_OUTLINE  2   /* the wire overlay's outline of the splat's +-2 quad */
#define GSR_MARK_COLOUR_FIXED 0
#define GSR_MARK_COLOUR_CD    1   /* (Cd.rgb, 1), as the wire overlay colours a line */
#define GSR_MARK_ANY_OPACITY  1   /* flags: also splats below 1/255 and the ones a visibility hides */
#define GSR_MARK_MAX_RADIUS   8
typedef struct gsr_mark_style {
    int32_t shape;            /* GSR_MARK_DOT / GSR_MARK_OUTLINE */
    int32_t radius;           /* DOT: 0..8 pixels; OUTLINE: 0 */
    int32_t colour_mode;
    int32_t flags;
    float   rgba[4];          /* FIXED: premultiplied, finite, 0 <= a <= 1 */
    const float* depth;       /* NULL: no test; float[height*width] window depths as gsr_render_depth takes them */
    int32_t depth_is_device;
    float   depth_bias;
    int32_t reserved_;        /* 0 */
} gsr_mark_style;
int  gsr_render_marks(gsr_context* ctx, const gsr_camera* cam, const uint32_t* mask, int mask_is_device,
                      const gsr_mark_style* style, void* rgba_inout, int is_device, int64_t* n_pixels);
int  gsr_get_marks(gsr_context* ctx, int64_t* calls, int64_t* pixels_last, double ms[4]);   /* any pointer may be NULL */

int  gsr_synchronize(gsr_context* ctx);
int  gsr_get_stats(gsr_context* ctx, gsr_stats* out);     /* synchronizes the stream */
int  gsr_stats_reset(gsr_context* ctx);

/* ---- knobs (performance only; never change pixels) ---------------------- */
#define GSR_OPT_XCD_SWIZZLE     1   /* tile -> workgroup mapping of the blend kernel: 0 = raster order, 1 = every XCD gets whole
                                       super-tiles, 2 (default) = 1 + heaviest tiles first (from the previous frame's per-tile work) whenever the
                                       kernels find the tiles unequal enough for it to pay, 3 = heaviest first always */
#define GSR_OPT_STAGE_TIMING    2   /* HIP events on the frame's stream: 0 = none, 1 = around the blend kernel only
                                       (default; feeds gsr_stats.blend_ms_total), 2 = around every stage (ms_* fields) */
#define GSR_OPT_SORT_CACHE      3   /* 0/1 (default 1): skip the depth sort when the frame description (camera, shard, geometry) is
                                       unchanged -- argsortByDistance's caching (src/GSplatRenderer.C:179-186) for the case
                                       that matters, a static viewport redraw; the sorted list holds only the splats visible
                                       to the camera that sorted, so a pure rotation re-sorts.
                                       2: the reference's rule in full (src/GSplatRenderer.C:165-186) -- the order depends on the camera
                                       POSITION only: the second frame in a row from one position sorts ALL splats for it once, and until
                                       the position moves every frame walks the splats in that order and skips its sort (pixels identical;
                                       single context, not deferred).  Off by default: on MI355X re-sorting the few hundred thousand splats
                                       a frame keeps is cheaper than walking six million in depth order */
#define GSR_OPT_SUPER_TILE      4   /* super-tile edge in tiles: 0 = auto (smallest power of two giving
                                       <= 256 super-tiles), or a lower bound 1,2,4,8,16 (raised as needed
                                       to stay within 256 super-tiles) */
#define GSR_OPT_FRAMES_IN_FLIGHT 6  /* 1 (default) or 2: with 2, frame f+1's front end (preprocess, sorts, binning) overlaps frame f's
                                       blend kernel on the GPU.  Per-frame results and their order on the context stream are
                                       unchanged.  Measured on MI355X: +3..6 % on frames that are not occlusion-culled, -4..10 % on
                                       culled ones (a slot's depth horizons are then two frames old, and the hand-over costs events) */
#define GSR_OPT_DEBUG_FLAGS     5   /* A/B switches for profiling: 1 = no alpha-support shrink of the bboxes,
                                       2 = bbox-only quadrant masks (no separating-axis test), 4 = sort all 32 key bits,
                                       8 = lazy colour without the ahead-of-time pass (every tile takes the fallback), 16 = cluster culling in the
                                       several-rounds-per-workgroup form of clouds beyond 33 M splats */
#define GSR_OPT_DEFERRED_CHECK   7   /* 0 (default) / 1: with a DEVICE target, gsr_render returns as soon as the frame is queued --
                                       no host wait at all -- and the frame's pair count is looked at by the next call that
                                       touches the context.  The back end always runs against the list buffer sized from
                                       earlier frames (+25 % headroom); a frame whose pair count outgrows it is composited
                                       from clamped lists and counted in gsr_stats.frames_truncated (the buffer is regrown
                                       for the next frame).  The first frame after a buffer-less start is never deferred. */
#define GSR_OPT_ROW_WORK        17   /* 0 (default) / 1: every frame ends with one more launch (k_row_work) that reduces the blend kernel's
                                       per-tile work to one sum per GLOBAL tile row, in mapped host memory: gsr_read_row_work.  Off: the
                                       frame's launches are exactly what they were */
#define GSR_OPT_SHARD_LAYOUT     9   /* (2 = gsr_multi's balanced bands, see gsr_multi_get_bands; a plain context takes 2 as 1)
                                       0 (default) = interleaved tile rows, 1 = contiguous bands; set on every rank AND on the
                                       context that stitches */
#define GSR_OPT_TIMING_EVERY    11   /* timing level 1 brackets the blend kernel of every N-th frame only (default 1): a pair of events in
                                       the stream costs the GPU ~12 us of idle queue, and an average wants a sample, not a census */
#define GSR_OPT_OCCLUSION_CULL  10   /* 0 / 1 (default: when the kernels find horizons for most lists, and not for a while after a
                                       horizon broke) / 2 (whenever possible): splats behind the depth at which every tile of the super-tiles they reach went
                                       opaque in the previous frame are dropped before projection, sorting and binning.  Exact: the lists
                                       are cut at those horizons, a tile that runs off a cut list without going opaque reports the
                                       frame, and gsr_render renders it again (as a front-slab frame where that pays: GSR_OPT_FRONT_SLAB) before it
                                       returns (gsr_stats.frames_repaired).  3 = never against a previous frame: every frame is a front-slab frame
                                       (occlusion culling inside the frame only: no prediction, no repairs, a frame time that does not depend on
                                       how the camera moved).
                                       Off for GSR_OPT_DEFERRED_CHECK frames.  Every rank of gsr_multi / gsr_comm culls and checks its own band. */
#define GSR_OPT_LAZY_COLOUR      8   /* SH colours only for the splats a frame can composite (the front of every super-tile list, as
                                       deep as the previous frame scanned, with an on-demand fallback) instead of for every visible
                                       splat: 0 = never, 2 = always, 1 (default) = when it pays -- the kernels compare, every frame,
                                       what the colour pass would evaluate with what eager evaluation does (large dense clouds: yes;
                                       small or sparse ones: no).  Same pixels, bit for bit, in every mode. */
#define GSR_OPT_CLUSTER_CULL    12   /* 1 (default) / 0: every frame starts by testing CLUSTERS of 64 spatially adjacent splats (their box + largest
                                       extent) against the clip planes, the screen, this rank's band of tile rows and the depth
                                       horizons; the per-splat stage runs over the surviving clusters only.  Conservative: same pixels. */
#define GSR_OPT_STORAGE_ORDER   13   /* 1 (default) = the splats are stored in Morton order of their positions (takes effect at the next
                                       upload), 0 = in upload order.  The storage order is what breaks ties in the depth sort (the
                                       reference's own tie order is unspecified: unstable tbb::parallel_sort, src/GSplatRenderer.C:206-207);
                                       gsr_debug_read_storage_order returns it. */
#define GSR_OPT_CULL_DILATE     14   /* occlusion culling: tiles by which a splat's (or cluster's) tile rect is widened before it is compared with the
                                       depth horizons of the previous frame (default 2; 0..64).  The view moves between frames: a wider
                                       neighbourhood culls less but breaks less often.  The library doubles it whenever a frame had to be
                                       repaired and lets it shrink back to this value while frames hold. */
#define GSR_OPT_LOCAL_SORT      15   /* depth sort of frames that keep few splats: 1 (default) = when the slot's previous frame kept <= 0.5 M, one global
                                       scatter into 1024 buckets over the key range that frame kept + one kernel that sorts every bucket locally
                                       (2 launches instead of 9); 0 = always three global LSD passes; 2 = the local form whenever a previous
                                       frame's key range is known.  Same order either way. */
#define GSR_OPT_FRONT_SLAB      16   /* occlusion culling WITHOUT a previous frame.  A frame that cannot use the previous frame's depth horizons (the
                                       first frames of a cloud, a camera jump, the re-render of a frame that broke a horizon) is rendered in two
                                       phases: the nearest splats first (a slab holding ~a tenth of the surviving clusters, picked from a histogram of
                                       their distances), then -- the tiles that are opaque by then need nothing more, exactly, with no prediction and
                                       no check -- the rest only where a tile is still open, continuing from the stored colour and transmittance.
                                       Bit-identical to the one-pass frame.  1 (default) = where occlusion culling pays; 0 = off; 2 = every frame
                                       that is not culled against a previous frame. */
int  gsr_set_option(gsr_context* ctx, int option, int value);

/* ---- debug / test access (device -> host copies of intermediates) -------- */
/* One projected record as tests read it back (not the packed device layout). */
typedef struct gsr_debug_record {
    float cx, cy, a1x, a1y, b1x, b1y, hx, hy, r, g, b, la;   /* a1 = kappa e/s1, b1 = kappa e_perp/s2, kappa = sqrt(log2 e); la = log2(opacity) (contract v3) */
    float key;
    int32_t visible;   /* 0 = culled */
} gsr_debug_record;
int  gsr_debug_read_records(gsr_context* ctx, gsr_debug_record* out, int64_t n);
/* what the two cull stages of the last frame left.  rect[i], i < n: the packed tile rect K1 gave the splat of upload index i
 * (x0 | y0 << 8 | x1 << 16 | y1 << 24, in units of 1, 2 or 4 tiles: frames of up to 4096, 8192, 16384 pixels a side), 0xffffffff = the
 * splat left no sort entry.  clusters: the ordered list of the clusters k_cluster_cull kept (cluster k = storage slots [64 k, 64 k + 64):
 * gsr_debug_read_storage_order); writes min(cap, count) of them and the count.  After a front-slab frame: its second phase's.
 * GSR_E_INVALID after a frame that walked the splats in a cached order (no clusters). */
int  gsr_debug_read_cull(gsr_context* ctx, uint32_t* rect, int64_t n, uint32_t* clusters, int64_t cap, int64_t* n_clusters);
/* depth order (nearest first) of the splats that survived culling in the last frame; writes min(cap, count)
 * indices and the count */
int  gsr_debug_read_depth_order(gsr_context* ctx, int32_t* perm, int64_t cap, int64_t* n_sorted);
/* the storage order of the uploaded splats: perm[j] = upload index of the splat in storage slot j (n = uploaded count).
 * Equal sort keys leave the depth sort in this order. */
int  gsr_debug_read_storage_order(gsr_context* ctx, int32_t* perm, int64_t n);
/* the resident geometry as stored, bytes as they sit in HBM: which = 0 geoA (n x 16: P.xyz, opacity), 1 geoB (n x 16: scale, orient, extent
 * half), 2 col (the colour chunks, 16 bytes per splat each: 6 with SH, 1 without, chunk k starting k * CAPACITY splats in -- the capacity is
 * the largest count the context has been uploaded with since its chunk count last changed, so the plane is size / (16 * chunks) splats
 * per chunk, of which the first n are live), 3 colrow (n x 128; GSR_E_INVALID for a cloud without SH), 4 clusA, 5 clusB (clusters x 16).
 * out = NULL: returns the plane's size in bytes; otherwise copies it (bytes = room in out) and returns the size.  Storage order. */
int  gsr_debug_read_resident(gsr_context* ctx, int which, void* out, int64_t bytes);
/* per-SUPER-tile [start,end) into the sorted pair list + the list itself (splat indices);
 * n_lists = stiles_x*stiles_y, n_pairs = pairs_total of the last frame */
int  gsr_debug_read_tile_lists(gsr_context* ctx, int32_t* list_start, int32_t* list_end, int64_t n_lists,
                               int32_t* pair_splat, int64_t n_pairs);

/* per tile of the last frame, four uint32: {list entries scanned, records gathered, wave-record evaluations, bit 0: the tile
 * stopped because every pixel was opaque} as the blend kernel counted them */
int  gsr_debug_read_tile_work(gsr_context* ctx, uint32_t* work4, int64_t n_tiles);
/* per tile of the WHOLE image (tiles_x * tiles_y of the frame, not the shard), four planes of n_tiles floats: the depth horizons the slot's
 * next frame would be culled against (distance^2, dilated; +inf = none), the raw horizons (sign bit = the tile's status), the dilated
 * status, and the covered depths of the last depth-tested frame as K1 saw them */
int  gsr_debug_read_horizons(gsr_context* ctx, float* out4, int64_t n_tiles);
/* ALL levels of the max pyramid the slot's next frame would be culled against (six: level l holds ((tiles_x - 1) >> l) + 1 by
 * ((tiles_y - 1) >> l) + 1 cells, row by row, from float meta24[2 + l] on; level 0 is the first plane of gsr_debug_read_horizons), and
 * what a look-up in it needs, as 24 int32: [0] tiles_x [1] tiles_y (whole image) [2..7] the levels' first cells [8] rect_shift
 * [9] super_shift [10] key_min [11] key_max of the last frame (uint32 bits) [12] the dilation radius built into the pyramid
 * [13] horizons valid (1) [14] stiles_x [15] the entries the list buffer holds; of the attempt queued last: [16] it applied the tiles'
 * status [17] it dropped splats behind the depth buffer where no horizon applied [18] it was culled; [19] shard index [20] count
 * [21] rows per band (0 = interleaved) [22] the band's first tile row [23] tile rows of this shard.  n_floats = the cells of all levels;
 * out = NULL with n_floats = 0 fills the words alone (the sizes a caller needs for the call proper).
 * GSR_E_INVALID before the first frame, after a frame that left no horizons, and for another count.  Changes nothing. */
int  gsr_debug_read_horizon_pyramid(gsr_context* ctx, float* out, int64_t n_floats, int32_t* meta24);

/* Stand-alone device radix sort of (key,value) u32 pairs on bits [0, key_bits):
 * the sort the pipeline uses, exposed for parity tests (host pointers). */
int  gsr_debug_sort_pairs(gsr_context* ctx, uint32_t* keys, uint32_t* vals, int64_t n, int key_bits);
/* ... the form small frames use: one scatter into 1024 buckets of width 2^bucket_shift starting at bucket_lo (keys outside
 * land in the first / last bucket), then every bucket sorted by one workgroup (k_radix_local).  Any lo / shift gives the same order;
 * GSR_E_INVALID if a bucket outgrows its region of 8192 keys (the pipeline then falls back to the global sort). */
int  gsr_debug_sort_pairs_local(gsr_context* ctx, uint32_t* keys, uint32_t* vals, int64_t n, int key_bits,
                                uint32_t bucket_lo, int bucket_shift);
/* The depth sort of a FRAME on given data, through the frame's own host functions and kernel instantiations (uint2 payloads, the
 * compacting first pass, a live `failed` word).  The input is K1's block-compacted layout: blk_cnt[b] (<= 256) items at the head of
 * slots [256 b, 256 b + 256) of keys[n_slots] / vals2[n_slots][2]; what the other slots hold is never read as an item.  n_slots is
 * the host's bound (a multiple of 256, > 0); n_slots_dev (a multiple of 256, <= n_slots) is the slot count the kernels read from
 * device memory: only blocks below it count.  mode:
 *   GSR_SORT_GLOBAL        the LSD passes on bits [0, key_bits), 3072 slots per workgroup; allow9 = 9-bit digits where they save a pass
 *   GSR_SORT_GLOBAL_MID    ... in the mid-size form, 1024 slots per workgroup
 *   GSR_SORT_LOCAL_GATHER  1024 buckets of width 2^shift from lo filled by the gathering scatter, then every bucket on its own
 *   GSR_SORT_LOCAL_K1      ... filled by one wave per block: k1_grid workgroups of four blocks (a smaller grid loops); range_dev != 0
 *                          hands lo and shift over in device memory, as a front-slab phase does
 *   GSR_SORT_LOCAL_DIRECT  ... filled with one atomic per key
 *   GSR_SORT_ORDERED       the position-keyed order: the blocks' heads one behind the other, as they are
 * Equal keys leave the global passes in slot order and the local kernel in the order of vals2[.][0].  On return keys / vals2 hold the
 * *n_kept items the device counted, sorted, and *failed what the local sort's "gave up" word held (a bucket beyond 8192 keys, a run of
 * more than 64 equal keys: the order means nothing then).  GSR_E_INVALID for sizes that are no multiples of 256, n_slots == 0 and
 * counts above 256.  All memory of the call goes with it. */
enum { GSR_SORT_GLOBAL = 0, GSR_SORT_GLOBAL_MID = 1, GSR_SORT_LOCAL_GATHER = 2, GSR_SORT_LOCAL_K1 = 3, GSR_SORT_LOCAL_DIRECT = 4, GSR_SORT_ORDERED = 5 };
int  gsr_debug_sort_frame(gsr_context* ctx, int mode, uint32_t* keys, uint32_t* vals2, const uint32_t* blk_cnt, int64_t n_slots,
                          int64_t n_slots_dev, int key_bits, int allow9, uint32_t lo, int shift, int range_dev, int k1_grid,
                          int64_t* n_kept, uint32_t* failed);
/* The plan of the attempt queued last (csrc/gsr_frame_plan.h: GSR_PLAN_OUT_FIELDS in their order, one int32 each; out32 holds 32):
 * which sort the frame really took. */
int  gsr_debug_last_plan(gsr_context* ctx, int32_t* out32);
/* The host-side policies (csrc/gsr_policy.h; DESIGN.md section 4: state table) as a pure function: state16 holds
 * [0] cull.pays [1] cull.weak [2] cull.vis_unculled [3] cull.holdoff [4] cull.backoff [5] cull.streak [6] cull.dilate [7] cull.opt_dilate
 * [8] slab.holdoff [9] local.fails [10] local.holdoff [11] (out) the event's answer; event = GsrPolicyEvent (0 upload, 1 cull allows?(a = opt),
 * 2 cull tick, 3 kernel verdict(a), 4 kept(a = splats, b = culled | opt << 1), 5 frame held, 6 horizon broke, 7 slab allows?(a = forced),
 * 8 slab tick, 9 slab done(a = kept), 10 local-sort begin(a = opt, b = static redraw), 11 local-sort result(a = failed), 12 set dilate(a)).
 * No context, no GPU: what tests/test_policy.py drives.  gsr_debug_policy_state reads a live context's state in the same layout. */
int  gsr_debug_policy(int32_t* state16, int event, long long a, long long b);
int  gsr_debug_policy_state(gsr_context* ctx, int32_t* state16);
/* What the library's host code holds at this moment, in the whole process: out4 = {device buffers, pinned host buffers, events,
 * streams} (the owning handles of csrc/gsr_host_buffers.h; the multi-GPU layer's own buffers are not counted).  Every count goes back
 * to what it was when a context is destroyed.  No context, no GPU: four zeros in a process that never created one. */
int  gsr_debug_live_handles(int64_t out4[4]);
/* The bytes the context's staging arena answers for right now (uploads, the host forms of the edits and reads and the copy verbs
 * stage there; it only grows): tests read it to know that a call had to replace the arena.  -1: ctx is NULL. */
int64_t gsr_debug_stage_bytes(gsr_context* ctx);
/* The frame driver's decisions (csrc/gsr_frame_plan.h, which documents the flat int32 layouts) as pure functions: which = 0 plans a
 * frame (in: the plan inputs, the slot's hints, classic_once; policy16: gsr_debug_policy's state, updated by the frame's policy events),
 * which = 1 reads an attempt's outcome from its mailbox (policy16 unused).  No context, no GPU: what tests/test_frame_plan.py drives. */
int  gsr_debug_frame_plan(int which, const int32_t* in, int32_t* policy16, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif
