// gsr_resident_select.h -- the verbs that select resident splats by screen region: gsr_select, gsr_select_eval,
// gsr_get_select; and by attribute: gsr_select_attrs, gsr_select_attrs_eval, gsr_get_select_attrs.  Host code only;
// included once, behind gsr_resident_read.h, whose contract it keeps and whose refusals (refuse_edit), pointer check
// (check_device_source), mask intake (MaskArg) and visibility rule (visibility_error, visibility_rule) it shares.  The rules and the
// kernels are k_select.h's and k_select_attrs.h's.
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

// the counter slots both selection kernels count into, and the pinned words they are read back into
static int ensure_sel_counters(gsr_context* c, const char* who)
{
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    int rc = GSR_OK;
    if (!c->sel_counters && (rc = c->sel_counters.alloc(cwords))) return rc;
    if (!c->sel_h_counters && c->sel_h_counters.alloc(cwords, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "%s: no pinned host memory for the counters", who);
    }
    return GSR_OK;
}
// the two counts of the slots read back: splats hit, bits set (a slot's words cannot carry: each counts at most n <= 2^31 splats)
static void sum_sel_counters(const gsr_context* c, unsigned long long* hits, unsigned long long* set)
{
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    const unsigned long long* const h = c->sel_h_counters;
    *hits = *set = 0;
    for (size_t k = 0; k < cwords; k += GSR_SEL_COUNTER_STRIDE) { *hits += h[k] & 0xffffffffull; *set += h[k] >> 32; }
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
    if ((rc = ensure_stage(c, off)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true)) || (rc = ensure_sel_counters(c, who)))
        return rc;
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
    unsigned long long hits = 0, set = 0;
    sum_sel_counters(c, &hits, &set);
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

// ---------------------------------------------------------------------------
// Selection by attribute (k_select_attrs.h).  gsr_select's contract and epilogue; the rule looks at the resident
// planes instead of the screen.
static_assert(GSR_ATTR_ALPHA == GSR_ATTRC_ALPHA && GSR_ATTR_SCALE_MAX == GSR_ATTRC_SCALE_MAX && GSR_ATTR_SCALE_MIN == GSR_ATTRC_SCALE_MIN &&
              GSR_ATTR_ANISOTROPY == GSR_ATTRC_ANISOTROPY && GSR_ATTR_COLOUR == GSR_ATTRC_COLOUR && GSR_ATTR_VOLUME == GSR_ATTRC_VOLUME &&
              GSR_ATTR_SKIP_HIDDEN == GSR_ATTRF_SKIP_HIDDEN, "the header's clauses and flags are the kernel's");
static_assert(sizeof(gsr_attr_rule) == sizeof(GsrAttrRule) && offsetof(gsr_attr_rule, alpha_lo) == offsetof(GsrAttrRule, alpha_lo) &&
              offsetof(gsr_attr_rule, anisotropy) == offsetof(GsrAttrRule, anisotropy) && offsetof(gsr_attr_rule, colour_lo) == offsetof(GsrAttrRule, colour_lo) &&
              offsetof(gsr_attr_rule, colour_hi) == offsetof(GsrAttrRule, colour_hi) && offsetof(gsr_attr_rule, reserved_) == offsetof(GsrAttrRule, reserved_) &&
              offsetof(gsr_attr_rule, volume) == offsetof(GsrAttrRule, vol), "gsr_attr_rule is the kernel's rule");

// what is wrong with the caller's rule (NULL: nothing)
static const char* attr_rule_error(const gsr_attr_rule* r)
{
    if (r->clauses & ~GSR_ATTRC_ALL) return "unknown clause bits";
    if (r->flags & ~GSR_ATTR_SKIP_HIDDEN) return "unknown flag bits";
    if (r->reserved_ != 0) return "reserved_ is not 0";
    if (r->op < GSR_SELECT_REPLACE || r->op > GSR_SELECT_TOGGLE) return "unknown op";
    if (r->clauses & GSR_ATTR_VOLUME) {
        if (r->n_volumes < 1 || r->n_volumes > GSR_VIS_MAX_VOLUMES) return "n_volumes is not within 1..GSR_VIS_MAX_VOLUMES with GSR_ATTR_VOLUME";
    } else if (r->n_volumes != 0) {
        return "n_volumes is not 0 without GSR_ATTR_VOLUME";
    }
    for (int k = 0; k < r->n_volumes; ++k) {
        if (r->volume[k].kind != GSR_VOL_BOX && r->volume[k].kind != GSR_VOL_ELLIPSOID) return "unknown volume kind";
        if (r->volume[k].invert != 0 && r->volume[k].invert != 1) return "invert is neither 0 nor 1";
    }
    return nullptr;
}
// the rule as the kernel takes it (volumes beyond n_volumes zeroed)
static GsrAttrRule attr_rule(const gsr_attr_rule* r)
{
    GsrAttrRule a{};
    std::memcpy(&a, r, offsetof(GsrAttrRule, vol));
    std::memcpy(a.vol, r->volume, sizeof(GsrVisVolume) * (size_t)r->n_volumes);
    return a;
}

extern "C" int gsr_select_attrs_eval(const gsr_attr_rule* r, const gsr_visibility* vis, int64_t n, const float* P, const float* alpha,
                                     const uint16_t* scale, const uint16_t* Cd, uint8_t* hit_out)
{
    if (!r) return set_err(GSR_E_INVALID, "gsr_select_attrs_eval: rule is NULL");
    const char* bad = attr_rule_error(r);
    if (!bad) bad = visibility_error(vis);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_attrs_eval: %s", bad);
    if (n < 0 || n > 0x7fffffffll || (n > 0 && !hit_out)) return set_err(GSR_E_INVALID, "gsr_select_attrs_eval: bad argument");
    const int cl = r->clauses;
    const gsr_visibility* const hide = (r->flags & GSR_ATTR_SKIP_HIDDEN) ? vis : nullptr;   // (no visibility: nothing is hidden)
    const uint32_t* const vmask = hide ? hide->mask : nullptr;
    if (vmask && hide->mask_splats < n)
        return set_err(GSR_E_INVALID, "gsr_select_attrs_eval: the visibility's mask covers %lld of the %lld splats", (long long)hide->mask_splats, (long long)n);
    const bool need_P = (cl & GSR_ATTR_VOLUME) || (hide && hide->n_volumes > 0);
    if (n > 0 && ((need_P && !P) || ((cl & GSR_ATTR_ALPHA) && !alpha) || ((cl & GSR_ATTRC_SCALES) && !scale) || ((cl & GSR_ATTR_COLOUR) && !Cd)))
        return set_err(GSR_E_INVALID, "gsr_select_attrs_eval: an array a set clause needs is NULL");
    const GsrAttrRule rule = attr_rule(r);
    const GsrVisRule vr = visibility_rule(hide);
    for (int64_t k = 0; k < n; ++k) {
        const float px = P ? P[3 * k] : 0.0f, py = P ? P[3 * k + 1] : 0.0f, pz = P ? P[3 * k + 2] : 0.0f;
        const bool hidden = hide && !gsr_splat_visible(vr, px, py, pz, vmask ? vmask[k >> 5] : 0u, (uint32_t)(k & 31));
        const uint16_t* const s = scale ? scale + 3 * k : nullptr;
        const uint16_t* const d = Cd ? Cd + 3 * k : nullptr;
        hit_out[k] = gsr_attr_hit(rule, px, py, pz, alpha ? alpha[k] : 0.0f, s ? s[0] : 0u, s ? s[1] : 0u, s ? s[2] : 0u, d ? d[0] : 0u,
                                  d ? d[1] : 0u, d ? d[2] : 0u, hidden) ? 1 : 0;
    }
    return GSR_OK;
}

extern "C" int gsr_get_select_attrs(gsr_context* c, int64_t* calls, int64_t* hit_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_select_attrs: ctx is NULL");
    return c->sela.report(calls, hit_last, ms);
}

extern "C" int gsr_select_attrs(gsr_context* c, const gsr_attr_rule* r, uint32_t* mask, int mask_is_device, int64_t* n_hit, int64_t* n_set)
{
    const char* const who = "gsr_select_attrs";
    if (!c || !r || !mask) return set_err(GSR_E_INVALID, "gsr_select_attrs: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const char* bad = attr_rule_error(r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_attrs: %s", bad);
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask exists
        if (n_hit) *n_hit = 0;
        if (n_set) *n_set = 0;
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const MaskArg mk{mask, mask_is_device != 0, n};
    if ((rc = mk.check(c, who))) return rc;            // before anything is launched: a wrong pointer must never be found out by a kernel
    if (mk.is_device && c->stream) HIP_TRY(hipStreamSynchronize(c->stream));   // a producer of the mask on the public stream has finished
    // ---- everything the call needs, before the launch: a host mask is staged in the arena
    if ((rc = ensure_stage(c, mk.stage_bytes())) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true)) ||
        (rc = ensure_sel_counters(c, who)))
        return rc;
    uint32_t* const dmask = mk.is_device ? mask : reinterpret_cast<uint32_t*>(c->stage + 0);
    hipStream_t us = c->slot[0].own;
    double copy_ms = 0.0;
    if (!mk.is_device && r->op != GSR_SELECT_REPLACE) {               // every op but REPLACE reads the mask first
        const uint32_t* staged = nullptr;
        const hipError_t e = mk.to_device(c, us, 0, &copy_ms, &staged);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_attrs: %s", hipGetErrorString(e));
    }
    // what a lane loads (k_select_attrs.h): only what the set clauses and the visibility in force need
    const int cl = r->clauses;
    const bool vis = c->vis_on, hide = vis && (r->flags & GSR_ATTR_SKIP_HIDDEN);
    int loads = 0;
    if (cl & GSR_ATTR_ALPHA) loads |= vis ? GSR_ATTRL_ALPHA0 : GSR_ATTRL_GEOA;
    if (cl & GSR_ATTR_VOLUME) loads |= GSR_ATTRL_GEOA;
    if (cl & GSR_ATTRC_SCALES) loads |= GSR_ATTRL_GEOB;
    if (cl & GSR_ATTR_COLOUR) loads |= GSR_ATTRL_COL;
    if (hide) loads |= GSR_ATTRL_HIDDEN | (c->vis.n_volumes > 0 ? GSR_ATTRL_GEOA : 0);
    const GsrAttrRule rule = attr_rule(r);
    const GsrVisRule vrule = hide ? c->vis : GsrVisRule{};
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    const float* const alpha0 = vis ? (const float*)c->alpha0 : nullptr;
    const uint32_t* const vis_mask = hide ? (const uint32_t*)c->vis_mask : nullptr;
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    hipError_t e = hipMemsetAsync(c->sel_counters, 0, cwords * 8, us);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_select_attrs, dim3(div_up(n, GSR_SELECT_THREADS)), dim3(GSR_SELECT_THREADS), 0, us, n, loads, inv, c->geoA, c->geoB, c->col,
                           alpha0, vis_mask, rule, vrule, dmask, c->sel_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->sel_h_counters, c->sel_counters, cwords * 8, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess && !mk.is_device) e = hipMemcpyAsync(mask, dmask, mk.words() * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_attrs: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    unsigned long long hits = 0, set = 0;
    sum_sel_counters(c, &hits, &set);
    if (n_hit) *n_hit = (int64_t)hits;
    if (n_set) *n_set = (int64_t)set;
    float ms = 0.0f;
    c->sela.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->sela.ms[1] = copy_ms;
    c->sela.ms[2] = 0.0;
    c->sela.ms[3] = up_now_ms() - t_begin;
    c->sela.calls += 1;
    c->sela.last = (int64_t)hits;
    return GSR_OK;
}
