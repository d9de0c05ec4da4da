// gsr_debug_read.h -- the debug / test doors of gsr_api.hip: a frame's intermediates read back (gsr_debug_read_*, gsr_debug_last_plan) and the
// pipeline's sorts on a test's arrays (gsr_debug_sort_*).  Host code of that translation unit, included by gsr_api.hip alone and IN FRONT of
// gsr_resident_edit.h: k_bucket_scatter<uint32_t, false> and k_radix_local<uint32_t> are first used here, and a kernel template's place in
// the code object is that of its first use.  Every door checks its own arguments and then goes through debug_enter; read-backs speak UPLOAD
// indices (host_perm, to_upload_index); what a call allocates is a std::vector or a DevMem of the call.
#pragma once

// number of entries of the depth-sorted list of the last frame (= visible splats of that frame)
static uint32_t sorted_count(FrameSlot* sl)
{
    (void)hipMemcpy(sl->h_counters, sl->d_frame, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    return (uint32_t)(sl->h_counters[6] & 0xffffffffull);
}

// storage slot -> upload index, on the host; empty = identity (fetched once per storage order, by each door where it always fetched it)
static int host_perm(gsr_context* c)
{
    if (!c->perm || c->h_perm.size() == c->n) return GSR_OK;
    c->h_perm.resize(c->n);
    if (c->n) HIP_TRY(hipMemcpy(c->h_perm.data(), c->perm, (size_t)c->n * 4, hipMemcpyDeviceToHost));
    return GSR_OK;
}
static inline uint32_t to_upload_index(const gsr_context* c, uint32_t slot) { return c->perm && slot < c->h_perm.size() ? (uint32_t)c->h_perm[slot] : slot; }

// behind a door's argument check: the context's device, everything in flight finished (a deferred frame that is rendered again included),
// *sl = the slot of the newest frame (need_frame: refused in the door's name where there is none), perm: the host copy of the storage order
static int debug_enter(gsr_context* c, const char* who, FrameSlot** sl = nullptr, bool need_frame = false, bool perm = false)
{
    HIP_TRY(hipSetDevice(c->device));
    const int rc = sync_all(c);
    if (rc) return rc;
    if (sl) *sl = latest_slot(c);
    if (need_frame && !*sl) return set_err(GSR_E_INVALID, "%s: no frame rendered yet", who);
    return perm ? host_perm(c) : GSR_OK;
}

extern "C" int gsr_debug_read_storage_order(gsr_context* c, int32_t* perm, int64_t n)
{
    if (!c || !perm || n < 0 || (uint64_t)n != c->n) return set_err(GSR_E_INVALID, "gsr_debug_read_storage_order: bad argument");
    if (const int rc = debug_enter(c, "gsr_debug_read_storage_order", nullptr, false, true)) return rc;
    for (int64_t j = 0; j < n; ++j) perm[j] = (int32_t)to_upload_index(c, (uint32_t)j);
    return GSR_OK;
}

extern "C" int gsr_debug_read_records(gsr_context* c, gsr_debug_record* out, int64_t n)
{
    if (!c || !out || n < 0 || (uint64_t)n > c->n) return set_err(GSR_E_INVALID, "gsr_debug_read_records: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_records", &sl, true)) return rc;
    if (sl->last_lazy && sl->last_supers > 0 && c->n > 0) {
        // lazy colour leaves most records pending: evaluate every list completely before reading them back
        hipLaunchKernelGGL(k_colour_prefix, dim3((unsigned)(sl->last_supers * CL_BLOCKS_PER_LIST)), dim3(CL_THREADS), 0, sl->stream,
                           sl->job.f, sl->pvA, sl->tiles.sstart, sl->tiles.send, c->prefix_all, (int)list_cap(*sl), c->colrow, sl->rec, sl->colour_evals);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(sl->stream));
    }
    if (const int rc = host_perm(c)) return rc;
    const uint32_t ns = sorted_count(sl);
    const int64_t n_out = n;
    n = (int64_t)c->n;   // (records live at storage slots: read them all, hand back the caller's first n_out upload indices)
    std::vector<GsrRecord> hr;
    std::vector<uint32_t> hk;
    std::vector<uint2> hv;
    try { hr.resize((size_t)n); hk.resize(ns); hv.resize(ns); }
    catch (const std::bad_alloc&) { return set_err(GSR_E_OOM, "gsr_debug_read_records: host allocation failed"); }
    if (n) {
        hipError_t e = hipMemcpy(hr.data(), sl->rec, (size_t)n * sizeof(GsrRecord), hipMemcpyDeviceToHost);
        // keys and rects live in depth order and only for the visible splats: un-permute through the payload
        if (e == hipSuccess && ns) e = hipMemcpy(hk.data(), sl->keyA, (size_t)ns * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && ns) e = hipMemcpy(hv.data(), sl->valA, (size_t)ns * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_debug_read_records: %s", hipGetErrorString(e));
    }
    for (int64_t i = 0; i < n_out; ++i) std::memset(&out[i], 0, sizeof(out[i]));
    for (uint32_t r = 0; r < ns; ++r) {
        const uint32_t slot = hv[r].x;
        if ((int64_t)slot >= n) continue;
        const uint32_t i = to_upload_index(c, slot);
        if ((int64_t)i >= n_out) continue;
        gsr_debug_record& o = out[i];
        const GsrRecord& q = hr[slot];
        o.visible = 1;
        o.cx = q.cx; o.cy = q.cy; o.a1x = q.a1x; o.a1y = q.a1y; o.b1x = q.b1x; o.b1y = q.b1y;
        o.hx = q.hx; o.hy = q.hy; o.r = q.r; o.g = q.g; o.b = q.b; o.la = q.la;
        const uint32_t kb = hk[r] + sl->key_min;   // keys are stored relative to the frame's key_min
        std::memcpy(&o.key, &kb, 4);
    }
    return GSR_OK;
}

extern "C" int gsr_debug_read_cull(gsr_context* c, uint32_t* rect, int64_t n, uint32_t* clusters, int64_t cap, int64_t* n_clusters)
{
    if (!c || !rect || n < 0 || (uint64_t)n > c->n || cap < 0 || (cap > 0 && !clusters) || !n_clusters) return set_err(GSR_E_INVALID, "gsr_debug_read_cull: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_cull", &sl, true)) return rc;
    if (!sl->last_cc_groups) return set_err(GSR_E_INVALID, "gsr_debug_read_cull: the last frame ran no cluster pass over clusters");
    if (const int rc = host_perm(c)) return rc;
    // rects live in depth order beside the storage slots of the splats that stayed (gsr_debug_read_records)
    const uint32_t ns = sorted_count(sl);
    std::vector<uint2> hv(ns ? ns : 1);
    if (ns) HIP_TRY(hipMemcpy(hv.data(), sl->valA, (size_t)ns * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) rect[i] = 0xffffffffu;
    for (uint32_t r = 0; r < ns; ++r) {
        const uint32_t slot = hv[r].x;
        if ((uint64_t)slot >= c->n) continue;
        const uint32_t i = to_upload_index(c, slot);
        if ((int64_t)i < n) rect[i] = hv[r].y;
    }
    // the survivors: workgroup g left cnt[g] of them, in cluster order, at seg[g * per ...]
    const uint32_t ng = sl->last_cc_groups, per = sl->last_cc_per;
    std::vector<uint32_t> cnt(ng), seg((size_t)ng * per);
    HIP_TRY(hipMemcpy(cnt.data(), sl->ccnt, (size_t)ng * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(seg.data(), sl->cseg, (size_t)ng * per * 4, hipMemcpyDeviceToHost));
    int64_t m = 0;
    for (uint32_t g = 0; g < ng; ++g)
        for (uint32_t k = 0; k < cnt[g] && k < per; ++k, ++m)
            if (m < cap) clusters[m] = seg[(size_t)g * per + k];
    *n_clusters = m;
    return GSR_OK;
}

extern "C" int gsr_debug_read_depth_order(gsr_context* c, int32_t* perm, int64_t cap, int64_t* n_sorted)
{
    if (!c || !perm || !n_sorted || cap < 0) return set_err(GSR_E_INVALID, "gsr_debug_read_depth_order: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_depth_order", &sl, true)) return rc;
    const uint32_t ns = sorted_count(sl);
    *n_sorted = ns;
    const int64_t m = (int64_t)ns < cap ? (int64_t)ns : cap;
    if (m) HIP_TRY(hipMemcpy2D(perm, 4, sl->valA, 8, 4, (size_t)m, hipMemcpyDeviceToHost));
    if (const int rc = host_perm(c)) return rc;
    for (int64_t r = 0; r < m; ++r) perm[r] = (int32_t)to_upload_index(c, (uint32_t)perm[r]);
    return GSR_OK;
}

extern "C" int gsr_debug_read_tile_lists(gsr_context* c, int32_t* list_start, int32_t* list_end, int64_t n_lists,
                                         int32_t* pair_splat, int64_t n_pairs)
{
    if (!c || !list_start || !list_end) return set_err(GSR_E_INVALID, "gsr_debug_read_tile_lists: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_tile_lists", &sl, true)) return rc;
    if (n_lists != (int64_t)sl->last_supers || n_pairs != (int64_t)sl->last_pairs || (n_pairs > 0 && !pair_splat))
        return set_err(GSR_E_INVALID, "gsr_debug_read_tile_lists: expected %d lists / %u pairs", sl->last_supers, sl->last_pairs);
    if (n_lists) {
        HIP_TRY(hipMemcpy(list_start, sl->tiles.sstart, (size_t)n_lists * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(list_end, sl->tiles.send, (size_t)n_lists * 4, hipMemcpyDeviceToHost));
    }
    if (n_pairs) HIP_TRY(hipMemcpy2D(pair_splat, 4, sl->pvA, 8, 4, (size_t)n_pairs, hipMemcpyDeviceToHost));
    if (const int rc = host_perm(c)) return rc;
    for (int64_t r = 0; r < n_pairs; ++r) pair_splat[r] = (int32_t)to_upload_index(c, (uint32_t)pair_splat[r] & sl->job.f.idx_mask);   // (depth bits off: gsr_device.h)
    return GSR_OK;
}

extern "C" int gsr_debug_read_tile_work(gsr_context* c, uint32_t* work4, int64_t n_tiles)
{
    if (!c || !work4) return set_err(GSR_E_INVALID, "gsr_debug_read_tile_work: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_tile_work", &sl)) return rc;
    if (!sl || n_tiles != (int64_t)sl->last_tiles_x * sl->last_local_ty)
        return set_err(GSR_E_INVALID, "gsr_debug_read_tile_work: expected %d tiles", sl ? sl->last_tiles_x * sl->last_local_ty : 0);
    if (n_tiles) HIP_TRY(hipMemcpy(work4, sl->tiles.tile_work, (size_t)n_tiles * 16, hipMemcpyDeviceToHost));
    return GSR_OK;
}

// what the slot's NEXT frame would be culled against, per tile of the whole image: [0] the (dilated) depth horizons (distance^2, +inf = none),
// [1] the raw horizons before dilation with the tile's status in the sign (k_blend.h: GsrHorizonArgs.stat), [2] the dilated status, [3] the
// covered depths of the last depth-tested frame as K1 saw them (level 0 of pyrc, k_cluster.h)
extern "C" int gsr_debug_read_horizons(gsr_context* c, float* out4, int64_t n_tiles)
{
    if (!c || !out4) return set_err(GSR_E_INVALID, "gsr_debug_read_horizons: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_horizons", &sl)) return rc;
    if (!sl || n_tiles <= 0) return set_err(GSR_E_INVALID, "gsr_debug_read_horizons: no frame");
    std::vector<float> zero((size_t)n_tiles, 0.0f);
    HIP_TRY(hipMemcpy(out4, sl->hpyr, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));                     // (level 0 starts at offset 0)
    HIP_TRY(hipMemcpy(out4 + n_tiles, sl->hraw, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out4 + 2 * n_tiles, sl->hstat, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    if (sl->dpyr && sl->dpyr.cap() >= (size_t)n_tiles) HIP_TRY(hipMemcpy(out4 + 3 * n_tiles, sl->dpyr + (size_t)(2 * sl->dpar + 1) * sl->dpyr.cap(), (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    else std::memcpy(out4 + 3 * n_tiles, zero.data(), (size_t)n_tiles * 4);
    return GSR_OK;
}

// every level of the pyramid the slot's NEXT frame would be culled against (sl->hpyr behind queue_frame_end's swap: levels 1..3 from the
// dilation's wave shuffles, 4..5 from its atomics), level l at meta[2 + l], and in `meta` what gsr_pyr_max, gsr_k1_back's look-up and
// k_tile_pass's rules took from the last frame (gsplat_hip.h lists the words).  Reads only: no resident bit, horizon, cached order,
// hint or policy changes.
extern "C" int gsr_debug_read_horizon_pyramid(gsr_context* c, float* out, int64_t n_floats, int32_t* meta24)
{
    const bool query = !out && n_floats == 0;      // (the words alone: how large is the pyramid?)
    if (!c || !meta24 || (!query && (!out || n_floats <= 0))) return set_err(GSR_E_INVALID, "gsr_debug_read_horizon_pyramid: bad argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_read_horizon_pyramid", &sl, true)) return rc;
    if (!sl->horizon_valid) return set_err(GSR_E_INVALID, "gsr_debug_read_horizon_pyramid: the last frame left no horizons");
    const FrameJob& j = sl->job;
    const GsrFrame& f = j.f;
    const int top = GSR_PYR_LEVELS - 1;
    const int64_t cells = (int64_t)f.pyr_off[top] + (int64_t)gsr_pyr_dim(f.tiles_x, top) * gsr_pyr_dim(f.tiles_y, top);
    if ((!query && n_floats != cells) || cells > (int64_t)GSR_PYR_FLOATS)
        return set_err(GSR_E_INVALID, "gsr_debug_read_horizon_pyramid: expected %lld floats", (long long)cells);
    if (!query) HIP_TRY(hipMemcpy(out, sl->hpyr, (size_t)cells * 4, hipMemcpyDeviceToHost));
    int o = 0;
    meta24[o++] = f.tiles_x; meta24[o++] = f.tiles_y;
    for (int l = 0; l < GSR_PYR_LEVELS; ++l) meta24[o++] = f.pyr_off[l];
    meta24[o++] = f.rect_shift; meta24[o++] = f.super_shift;
    meta24[o++] = (int32_t)f.key_min; meta24[o++] = (int32_t)f.key_max;
    meta24[o++] = sl->hpyr_re; meta24[o++] = sl->horizon_valid ? 1 : 0;
    meta24[o++] = f.stiles_x; meta24[o++] = list_cap(*sl);
    // (k_tile_pass's switches of the attempt queued last: queue_frame_end)
    meta24[o++] = (j.cull && j.dcull && j.dstat) ? 1 : 0; meta24[o++] = (j.dcull && !j.dblind) ? 1 : 0; meta24[o++] = j.cull ? 1 : 0;
    meta24[o++] = f.shard_index; meta24[o++] = f.shard_count; meta24[o++] = f.shard_rpb; meta24[o++] = f.shard_first;
    meta24[o++] = f.local_tiles_y;
    static_assert(2 + GSR_PYR_LEVELS + 16 == 24, "gsr_debug_read_horizon_pyramid writes 24 words");
    return GSR_OK;
}

// the pipeline's stable sort of (key, value) pairs on host arrays; local: the small-frame form, one scatter into BK_BUCKETS buckets of
// width 2^shift from lo, then every bucket on its own (k_radix_local)
static int debug_sort_pairs(gsr_context* c, uint32_t* keys, uint32_t* vals, int64_t n64, int key_bits, bool local, uint32_t lo, int shift)
{
    if (!c || n64 < 0 || n64 > 0x7fffffffll || key_bits < 1 || key_bits > 32 || (n64 > 0 && (!keys || !vals)))
        return set_err(GSR_E_INVALID, "gsr_debug_sort_pairs: bad argument");
    if (n64 == 0) return GSR_OK;
    int rc = debug_enter(c, "gsr_debug_sort_pairs");
    if (rc) return rc;
    FrameSlot& sl = c->slot[0];
    const uint32_t n = (uint32_t)n64;
    DevMem<uint32_t> scratch[4];           // the pairs (kA, vA) and (kB, vB) of the sort, gone with the call
    for (DevMem<uint32_t>& m : scratch)
        if ((rc = m.alloc(n))) return rc;
    uint32_t *kA = scratch[0], *vA = scratch[1], *kB = scratch[2], *vB = scratch[3];
    hipError_t e = hipMemcpyAsync(kA, keys, (size_t)n * 4, hipMemcpyHostToDevice, sl.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(vA, vals, (size_t)n * 4, hipMemcpyHostToDevice, sl.stream);
    if (e == hipSuccess) {
        if (local) {
            // (uint32 payloads in the slot's bucket regions: the payload region is large enough for either type)
            const uint32_t nblk = div_up(n, RS_TILE);
            hipError_t e2 = hipMemsetAsync(sl.bkt_cnt, 0, (size_t)BK_BUCKETS * BK_STRIDE * sizeof(uint32_t), sl.stream);
            if (e2 == hipSuccess) e2 = hipMemsetAsync(sl.d_counts + 2, 0, 4, sl.stream);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bucket_scatter<uint32_t, false>), dim3(nblk), dim3(RS_THREADS), 0, sl.stream, kA, vA, n, (const uint32_t*)nullptr,
                               shift, lo, (const uint32_t*)nullptr, sl.bkt_cnt, sl.bkt_key, reinterpret_cast<uint32_t*>(sl.bkt_val.get()), (uint32_t*)nullptr, sl.d_counts + 2);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_radix_local<uint32_t>), dim3(BK_BUCKETS), dim3(RL_THREADS), 0, sl.stream, sl.bkt_cnt, shift, key_bits, lo,
                               sl.bkt_key, reinterpret_cast<uint32_t*>(sl.bkt_val.get()), kA, vA, (uint32_t*)nullptr, (uint32_t*)nullptr);
            uint32_t over = 0;
            if (e2 == hipSuccess) e2 = hipMemcpyAsync(&over, sl.d_counts + 2, 4, hipMemcpyDeviceToHost, sl.stream);
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(sl.stream);
            if (e2 != hipSuccess) rc = set_err(GSR_E_HIP, "gsr_debug_sort_pairs_local: %s", hipGetErrorString(e2));
            else if (over) rc = set_err(GSR_E_INVALID, "gsr_debug_sort_pairs_local: a bucket overflowed its region of %d keys (the pipeline would fall back to the global sort)", BK_CAP);
        } else {
            rc = radix_sort(sl, kA, vA, kB, vB, n, key_bits, true, (uint32_t*)nullptr, RS_XCD_DEPTH != 0);
        }
        if (!rc) {
            e = hipMemcpyAsync(keys, kA, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(vals, vA, (size_t)n * 4, hipMemcpyDeviceToHost, sl.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
        }
    }
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_debug_sort_pairs: %s", hipGetErrorString(e));
    return rc;
}
extern "C" int gsr_debug_sort_pairs(gsr_context* c, uint32_t* keys, uint32_t* vals, int64_t n64, int key_bits)
{
    return debug_sort_pairs(c, keys, vals, n64, key_bits, false, 0u, 0);
}
extern "C" int gsr_debug_sort_pairs_local(gsr_context* c, uint32_t* keys, uint32_t* vals, int64_t n64, int key_bits, uint32_t bucket_lo, int bucket_shift)
{
    if (bucket_shift < 0 || bucket_shift > 31) return set_err(GSR_E_INVALID, "gsr_debug_sort_pairs_local: bad bucket shift");
    return debug_sort_pairs(c, keys, vals, n64, key_bits, true, bucket_lo, bucket_shift);
}

// The depth sort of a FRAME on a test's arrays: K1's block-compacted layout in, what the frame's own drivers (radix_sort<uint2> with a
// compacting first pass, launch_local_sort, launch_ordered_compact) make of it out.  Every array is a DevMem of this call; the bucket
// regions are the slot's (as in gsr_debug_sort_pairs_local), and the slot's histogram is set aside for the call and put back.
extern "C" int gsr_debug_sort_frame(gsr_context* c, int mode, uint32_t* keys, uint32_t* vals2, const uint32_t* blk_cnt, int64_t n_slots64,
                                    int64_t n_slots_dev64, int key_bits, int allow9, uint32_t lo, int shift, int range_dev, int k1_grid,
                                    int64_t* n_kept, uint32_t* failed)
{
    const bool local = mode == GSR_SORT_LOCAL_GATHER || mode == GSR_SORT_LOCAL_K1 || mode == GSR_SORT_LOCAL_DIRECT;
    if (!c || !keys || !vals2 || !blk_cnt || !n_kept || !failed || mode < GSR_SORT_GLOBAL || mode > GSR_SORT_ORDERED)
        return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: bad argument");
    if (n_slots64 <= 0 || n_slots64 > 0x7fffff00ll || n_slots64 % RS_SRC_BLOCK || n_slots_dev64 < 0 || n_slots_dev64 > n_slots64 || n_slots_dev64 % RS_SRC_BLOCK)
        return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: slot counts are multiples of %d, 0 < n_slots, 0 <= n_slots_dev <= n_slots", RS_SRC_BLOCK);
    if (key_bits < 1 || key_bits > 32 || shift < 0 || shift > 31) return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: bad key bits or bucket shift");
    if (range_dev && mode != GSR_SORT_LOCAL_K1) return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: only LOCAL_K1 reads its range from the device");
    if (mode == GSR_SORT_LOCAL_K1 && k1_grid < 1) return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: LOCAL_K1 needs a grid of at least one workgroup");
    const uint32_t n_slots = (uint32_t)n_slots64, n_blocks = n_slots / RS_SRC_BLOCK;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (blk_cnt[b] > (uint32_t)RS_SRC_BLOCK) return set_err(GSR_E_INVALID, "gsr_debug_sort_frame: block %u counts %u items of %d slots", b, blk_cnt[b], RS_SRC_BLOCK);
    int rc = debug_enter(c, "gsr_debug_sort_frame");
    if (rc) return rc;
    FrameSlot& sl = c->slot[0];
    hipStream_t s = sl.stream;
    DevMem<uint32_t> kbuf[2], cnt, ctl, pre;   // ctl: [0] slots filled, [1] items kept, [2] the sort gave up, [4..5] { lo, shift }
    DevMem<uint2> vbuf[2];
    if ((rc = kbuf[0].alloc(n_slots)) || (rc = kbuf[1].alloc(n_slots)) || (rc = vbuf[0].alloc(n_slots)) || (rc = vbuf[1].alloc(n_slots)) ||
        (rc = cnt.alloc(n_blocks)) || (rc = ctl.alloc(8)) || (rc = pre.alloc((size_t)n_blocks + 8)))
        return rc;
    const uint32_t h_ctl[8] = {(uint32_t)n_slots_dev64, 0u, 0u, 0u, lo, (uint32_t)shift, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(kbuf[0], keys, (size_t)n_slots * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(vbuf[0], vals2, (size_t)n_slots * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(cnt, blk_cnt, (size_t)n_blocks * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ctl, h_ctl, sizeof h_ctl, hipMemcpyHostToDevice, s));
    uint32_t *kA = kbuf[0], *kB = kbuf[1];
    uint2 *vA = vbuf[0], *vB = vbuf[1];
    if (local) {
        HIP_TRY(hipMemsetAsync(sl.bkt_cnt, 0, (size_t)BK_BUCKETS * BK_STRIDE * sizeof(uint32_t), s));
        LocalSortOps o{};
        o.keys = kA; o.vals = vA; o.cnt = cnt; o.slots_dev = ctl; o.n_slots = n_slots;
        o.scatter = mode == GSR_SORT_LOCAL_DIRECT ? LS_DIRECT : (mode == GSR_SORT_LOCAL_K1 ? LS_PER_WAVE : LS_GATHER);
        o.wave_grid = std::min(div_up(n_blocks, 4u), (uint32_t)std::max(k1_grid, 1));
        o.range = range_dev ? ctl + 4 : (const uint32_t*)nullptr;
        o.lo = range_dev ? 0u : lo;       // (as a front-slab phase passes them: the kernels must take the device's)
        o.shift = range_dev ? 0 : shift;
        o.key_bits = key_bits;
        o.bkt_cnt = sl.bkt_cnt; o.bkt_key = sl.bkt_key; o.bkt_val = sl.bkt_val;
        o.failed = ctl + 2; o.n_out = ctl + 1;
        rc = launch_local_sort(s, o);
    } else if (mode == GSR_SORT_ORDERED) {
        rc = launch_ordered_compact(s, kA, vA, cnt, ctl, n_blocks, pre, kB, vB, ctl + 1);
        std::swap(kA, kB); std::swap(vA, vB);
    } else {
        DevVec<uint32_t> hist;             // (the slot's own histogram, with its capacity, comes back as it was)
        sl.hist.swap(hist);
        rc = radix_sort(sl, kA, vA, kB, vB, n_slots, key_bits, allow9 != 0, ctl + 1, RS_XCD_DEPTH != 0, cnt, ctl, mode == GSR_SORT_GLOBAL_MID);
        const hipError_t e = hipStreamSynchronize(s);   // (before the call's histogram goes)
        sl.hist.swap(hist);
        if (!rc && e != hipSuccess) rc = set_err(GSR_E_HIP, "gsr_debug_sort_frame: %s", hipGetErrorString(e));
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    uint32_t out_ctl[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(out_ctl, ctl, sizeof out_ctl, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_ctl[1] > n_slots) return set_err(GSR_E_HIP, "gsr_debug_sort_frame: the device counted %u items in %u slots", out_ctl[1], n_slots);
    *n_kept = out_ctl[1];
    *failed = out_ctl[2];
    if (out_ctl[1]) {
        HIP_TRY(hipMemcpy(keys, kA, (size_t)out_ctl[1] * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(vals2, vA, (size_t)out_ctl[1] * 8, hipMemcpyDeviceToHost));
    }
    return GSR_OK;
}

// the plan of the attempt queued last (GSR_PLAN_OUT_FIELDS of csrc/gsr_frame_plan.h, in their order, one int32 each)
extern "C" int gsr_debug_last_plan(gsr_context* c, int32_t* out32)
{
    if (!c || !out32) return set_err(GSR_E_INVALID, "gsr_debug_last_plan: NULL argument");
    FrameSlot* sl = nullptr;
    if (const int rc = debug_enter(c, "gsr_debug_last_plan", &sl, true)) return rc;
    const GsrFramePlan& r = sl->last_plan;
    int o = 0;
#define GSR_PUT(t, name) out32[o++] = (int32_t)r.name;
    GSR_PLAN_OUT_FIELDS(GSR_PUT)
#undef GSR_PUT
#define GSR_COUNT(t, name) + 1
    static_assert(0 GSR_PLAN_OUT_FIELDS(GSR_COUNT) <= 32, "gsr_debug_last_plan writes at most 32 words");
#undef GSR_COUNT
    return GSR_OK;
}
