// gsr_resident_select.h -- the verbs that select resident splats by screen region: gsr_select, gsr_select_eval,
// gsr_get_select.  Host code only; included once, behind gsr_resident_read.h, whose contract it keeps and whose refusals
// (refuse_edit) and pointer check (check_device_source) it shares.  The rule and the kernel are k_select.h's.
//
// A select writes NOTHING the context keeps: no resident bit, no horizon, no cached order, no policy, no visibility state, no entry of
// gsr_stats.  It therefore does not wait for the frames in flight, and the next frame runs the launches it would have run.  What it
// uses of the context: slot 0's own stream, the first two events of the upload clock, the inverse of the storage order (built on first
// use per geometry), the staging arena -- idle, because an upload in progress is refused -- for what comes from host memory, and
// counter slots of its own.
#pragma once

static_assert(GSR_SELECT_REPLACE == GSR_SELOP_REPLACE && GSR_SELECT_ADD == GSR_SELOP_ADD && GSR_SELECT_SUBTRACT == GSR_SELOP_SUBTRACT &&
              GSR_SELECT_INTERSECT == GSR_SELOP_INTERSECT && GSR_SELECT_TOGGLE == GSR_SELOP_TOGGLE && GSR_SELECT_ANY_OPACITY == GSR_SELF_ANY_OPACITY && GSR_SELECT_BLOCK == GSR_SELECT_THREADS,
              "the header's ops and flags are the kernel's");

// what is wrong with the caller's camera or region (NULL: nothing)
static const char* select_error(const gsr_camera* cam, const gsr_select_region* r)
{
    if (cam->width < 1 || cam->height < 1 || cam->width > GSR_MAX_DIM || cam->height > GSR_MAX_DIM) return "width or height is not within 1..GSR_MAX_DIM";
    if (r->op < GSR_SELECT_REPLACE || r->op > GSR_SELECT_TOGGLE) return "unknown op";
    if (r->flags & ~GSR_SELECT_ANY_OPACITY) return "unknown flag bits";
    if (r->reserved_ != 0) return "reserved_ is not 0";
    return nullptr;
}
// the rule of (cam, origin, region) as the kernel takes it: the matrices by the accessors build_frame uses
static GsrSelectRule select_rule(const gsr_camera* cam, const float origin[3], const gsr_select_region* r)
{
    GsrSelectRule s{};
    for (int row = 0; row < 3; ++row)
        for (int k = 0; k < 4; ++k) s.ov[row * 4 + k] = M4h(cam->obj_view, row, k);
    for (int row = 0; row < 4; ++row)
        for (int k = 0; k < 4; ++k) s.pr[row * 4 + k] = M4h(cam->proj, row, k);
    for (int k = 0; k < 3; ++k) s.origin[k] = origin[k];
    s.W = (float)cam->width; s.H = (float)cam->height;
    s.x0 = r->x0; s.y0 = r->y0; s.x1 = r->x1; s.y1 = r->y1;
    s.depth_bias = r->depth_bias;
    s.flags = r->flags;
    s.width = cam->width; s.height = cam->height;
    return s;
}

extern "C" int gsr_select_eval(const gsr_camera* cam, const float origin[3], const gsr_select_region* r, const float* P, const float* opacity,
                               int64_t n, uint8_t* hit_out, float* centre_out)
{
    if (!cam || !origin || !r) return set_err(GSR_E_INVALID, "gsr_select_eval: NULL argument");
    const char* bad = select_error(cam, r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_eval: %s", bad);
    if (n < 0 || (n > 0 && (!P || !hit_out))) return set_err(GSR_E_INVALID, "gsr_select_eval: bad argument");
    const GsrSelectRule rule = select_rule(cam, origin, r);
    for (int64_t k = 0; k < n; ++k)
        hit_out[k] = gsr_select_hit(rule, P[3 * k], P[3 * k + 1], P[3 * k + 2], opacity ? opacity[k] : 1.0f, r->image, r->depth,
                                    centre_out ? centre_out + 3 * k : nullptr) ? 1 : 0;
    return GSR_OK;
}

extern "C" int gsr_get_select(gsr_context* c, int64_t* calls, int64_t* hit_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_select: ctx is NULL");
    return c->sel.report(calls, hit_last, ms);
}

extern "C" int gsr_select(gsr_context* c, const gsr_camera* cam, const gsr_select_region* r, uint32_t* mask, int mask_is_device,
                          int64_t* n_hit, int64_t* n_set)
{
    const char* const who = "gsr_select";
    if (!c || !cam || !r || !mask) return set_err(GSR_E_INVALID, "gsr_select: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const char* bad = select_error(cam, r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select: %s", bad);
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask exists
        if (n_hit) *n_hit = 0;
        if (n_set) *n_set = 0;
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const size_t words = ((size_t)n + 31) / 32, pixels = (size_t)cam->width * (size_t)cam->height, image_words = (pixels + 31) / 32;
    // every device pointer, with its exact size, before anything is launched: a wrong pointer must never be found out by a kernel
    if (mask_is_device && (rc = check_device_source(c, mask, words * 4, who, "mask"))) return rc;
    if (r->image && r->image_is_device && (rc = check_device_source(c, r->image, image_words * 4, who, "image"))) return rc;
    if (r->depth && r->depth_is_device && (rc = check_device_source(c, r->depth, pixels * 4, who, "depth"))) return rc;
    // whoever produced a device source on the public stream (gsr_resolve_depth_device, say) or still reads the mask there has finished
    if ((mask_is_device || (r->image && r->image_is_device) || (r->depth && r->depth_is_device)) && c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
    // ---- everything the call needs, before the launch: what comes from or goes to host memory is staged in the arena
    const bool reads_mask = r->op != GSR_SELECT_REPLACE;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oMask = place(mask_is_device ? 0 : words * 4), oImage = place(r->image && !r->image_is_device ? image_words * 4 : 0),
                 oDepth = place(r->depth && !r->depth_is_device ? pixels * 4 : 0);
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    if ((rc = ensure_stage(c, off)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    if (!c->sel_counters && (rc = c->sel_counters.alloc(cwords))) return rc;
    if (!c->sel_h_counters && c->sel_h_counters.alloc(cwords, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "gsr_select: no pinned host memory for the counters");
    }
    uint32_t* const dmask = mask_is_device ? mask : reinterpret_cast<uint32_t*>(c->stage + oMask);
    const uint32_t* dimage = r->image;
    const float* ddepth = r->depth;
    hipStream_t us = c->slot[0].own;
    double copy_ms = 0.0;
    {
        const double t0 = up_now_ms();
        hipError_t e = hipSuccess;
        bool copied = false;
        auto h2d = [&](void* d, const void* h, size_t bytes) { if (e == hipSuccess) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, us); copied = true; };
        if (!mask_is_device && reads_mask) h2d(dmask, mask, words * 4);
        if (r->image && !r->image_is_device) { uint32_t* d = reinterpret_cast<uint32_t*>(c->stage + oImage); h2d(d, r->image, image_words * 4); dimage = d; }
        if (r->depth && !r->depth_is_device) { float* d = reinterpret_cast<float*>(c->stage + oDepth); h2d(d, r->depth, pixels * 4); ddepth = d; }
        if (copied && e == hipSuccess) e = hipStreamSynchronize(us);           // the caller's arrays may be freed on return
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select: %s", hipGetErrorString(e));
        if (copied) copy_ms = up_now_ms() - t0;
    }
    const GsrSelectRule rule = select_rule(cam, c->origin, r);
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    hipError_t e = hipMemsetAsync(c->sel_counters, 0, cwords * 8, us);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_select, dim3(div_up(n, GSR_SELECT_THREADS)), dim3(GSR_SELECT_THREADS), 0, us, n, inv, c->geoA, rule, dimage, ddepth, (int)r->op,
                           dmask, c->sel_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->sel_h_counters, c->sel_counters, cwords * 8, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess && !mask_is_device) e = hipMemcpyAsync(mask, dmask, words * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    const unsigned long long* const h = c->sel_h_counters;
    unsigned long long hits = 0, set = 0;              // (a slot's words cannot carry: each counts at most n <= 2^31 splats)
    for (size_t k = 0; k < cwords; k += GSR_SEL_COUNTER_STRIDE) { hits += h[k] & 0xffffffffull; set += h[k] >> 32; }
    if (n_hit) *n_hit = (int64_t)hits;
    if (n_set) *n_set = (int64_t)set;
    float ms = 0.0f;
    c->sel.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->sel.ms[1] = copy_ms;
    c->sel.ms[2] = 0.0;
    c->sel.ms[3] = up_now_ms() - t_begin;
    c->sel.calls += 1;
    c->sel.last = (int64_t)hits;
    return GSR_OK;
}
