// gsr_resident_select.h -- the verbs that select resident splats by screen region: gsr_select, gsr_select_eval,
// gsr_get_select; and by attribute: gsr_select_attrs, gsr_select_attrs_eval, gsr_get_select_attrs.  Host code only;
// included once, behind gsr_resident_read.h, whose contract it keeps and whose refusals (refuse_edit), pointer check
// (check_device_source), mask intake (MaskArg) and visibility rule (visibility_error, visibility_rule) it shares.  The rules and the
// kernels are k_select.h's and k_select_attrs.h's.  At the end, by density (k_density.h): gsr_select_density,
// gsr_select_density_eval, gsr_get_select_density -- the same mask contract, but it borrows the scratch of an upload's sort and
// therefore DOES wait for the frames in flight; what it says there holds for it alone.
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

// ---------------------------------------------------------------------------
// Selection by density (k_density.h).  gsr_select's mask contract and epilogue; the rule counts the population of the
// cells around a splat.  Unlike its two siblings the verb borrows the scratch of an upload's sort (c->up_sort, slot 0's histogram and
// digit totals: nothing live between uploads and edits -- morton_order copies the permutation out), so it waits for the frames in
// flight first, as gsr_move does, and queues everything on the stream that sort runs on.
static_assert(GSR_DENSITY_SKIP_HIDDEN == GSR_DENF_SKIP_HIDDEN && GSR_DENSITY_HIT_OUTSIDE == GSR_DENF_HIT_OUTSIDE && GSR_DENSITY_CELLS == GSR_DEN_CELLS &&
              GSR_DENSITY_HIST_BINS == GSR_DEN_BINS, "the header's flags and limits are the kernels'");
static_assert(sizeof(gsr_density_rule) == 44 && offsetof(gsr_density_rule, reach) == 16 && offsetof(gsr_density_rule, count_lo) == 32 &&
              offsetof(gsr_density_rule, alpha_min) == 40 && sizeof(gsr_density_result) == 8 * (3 + GSR_DENSITY_HIST_BINS), "the rule is 11 dwords, the result 67 counts");

// what is wrong with the caller's rule (NULL: nothing)
static const char* density_rule_error(const gsr_density_rule* r)
{
    if (!std::isfinite(r->cell) || !(r->cell > 0.0f)) return "cell is not a finite positive number";
    if (!std::isfinite(1.0f / r->cell)) return "1 / cell is not finite";
    if (!std::isfinite(r->origin[0]) || !std::isfinite(r->origin[1]) || !std::isfinite(r->origin[2])) return "origin is not finite";
    if (r->reach < 0 || r->reach > GSR_DENSITY_MAX_REACH) return "reach is not within 0..GSR_DENSITY_MAX_REACH";
    if (r->flags & ~(GSR_DENSITY_SKIP_HIDDEN | GSR_DENSITY_HIT_OUTSIDE)) return "unknown flag bits";
    if (r->op < GSR_SELECT_REPLACE || r->op > GSR_SELECT_TOGGLE) return "unknown op";
    if (r->reserved_ != 0) return "reserved_ is not 0";
    if (r->alpha_min != r->alpha_min) return "alpha_min is a NaN";
    return nullptr;
}
// the rule as the kernels take it: inv_cell by ONE IEEE float32 division, here and nowhere else
static GsrDensityRule density_rule(const gsr_density_rule* r)
{
    GsrDensityRule d{};
    d.inv_cell = 1.0f / r->cell;
    for (int k = 0; k < 3; ++k) d.origin[k] = r->origin[k];
    d.reach = r->reach; d.flags = r->flags; d.op = r->op;
    d.count_lo = r->count_lo; d.count_hi = r->count_hi;
    d.alpha_min = r->alpha_min;
    return d;
}

// The rule on the host.  The classes come from gsr_density_class; the counts from a table of the OCCUPIED cells (the sorted unique keys
// and the running population in front of each): N is formed once per cell, as the difference of two running populations per row of
// gsr_density_row, and handed to every splat of the cell.
extern "C" int gsr_select_density_eval(const gsr_density_rule* r, const gsr_visibility* vis, int64_t n, const float* P, const float* alpha,
                                       uint8_t* hit_out, uint32_t* counts_out, gsr_density_result* result)
{
    if (!r) return set_err(GSR_E_INVALID, "gsr_select_density_eval: rule is NULL");
    const char* bad = density_rule_error(r);
    if (!bad) bad = visibility_error(vis);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_density_eval: %s", bad);
    if (n < 0 || n > 0x7fffffffll || (n > 0 && (!P || !hit_out))) return set_err(GSR_E_INVALID, "gsr_select_density_eval: bad argument");
    const gsr_visibility* const hide = (r->flags & GSR_DENSITY_SKIP_HIDDEN) ? vis : nullptr;   // (no visibility: nothing is hidden)
    const uint32_t* const vmask = hide ? hide->mask : nullptr;
    if (vmask && hide->mask_splats < n)
        return set_err(GSR_E_INVALID, "gsr_select_density_eval: the visibility's mask covers %lld of the %lld splats", (long long)hide->mask_splats, (long long)n);
    const GsrDensityRule rule = density_rule(r);
    const GsrVisRule vr = visibility_rule(hide);
    gsr_density_result res;
    std::memset(&res, 0, sizeof res);
    std::vector<uint32_t> cls((size_t)n), cells;
    for (int64_t k = 0; k < n; ++k) {
        const float px = P[3 * k], py = P[3 * k + 1], pz = P[3 * k + 2];
        const bool hidden = hide && !gsr_splat_visible(vr, px, py, pz, vmask ? vmask[k >> 5] : 0u, (uint32_t)(k & 31));
        const uint32_t c = gsr_density_class(rule, px, py, pz, alpha ? alpha[k] : 1.0f, hidden);
        cls[(size_t)k] = c;
        if (c < GSR_DEN_NOKEY) cells.push_back(c);
        else if (c == GSR_DEN_OUTSIDE) res.n_outside += 1;
    }
    res.n_population = (int64_t)cells.size();
    // the occupied cells: ukey[u] rising, before[u] = the population of the cells in front of u (before[U] = all of it)
    std::sort(cells.begin(), cells.end());
    std::vector<uint32_t> ukey, before;
    for (size_t k = 0; k < cells.size(); ++k)
        if (k == 0 || cells[k] != cells[k - 1]) { ukey.push_back(cells[k]); before.push_back((uint32_t)k); }
    before.push_back((uint32_t)cells.size());
    res.n_cells = (int64_t)ukey.size();
    std::vector<uint32_t> cell_n(ukey.size(), 0u);
    for (size_t u = 0; u < ukey.size(); ++u) {
        uint32_t N = 0u;
        for (int dz = -rule.reach; dz <= rule.reach; ++dz)
            for (int dy = -rule.reach; dy <= rule.reach; ++dy) {
                uint32_t klo = 0u, khi = 0u;
                if (!gsr_density_row(ukey[u], rule.reach, dy, dz, &klo, &khi)) continue;
                const size_t a = (size_t)(std::lower_bound(ukey.begin(), ukey.end(), klo) - ukey.begin());
                const size_t b = (size_t)(std::upper_bound(ukey.begin(), ukey.end(), khi) - ukey.begin());
                N += before[b] - before[a];
            }
        cell_n[u] = N;
        res.count_hist[gsr_density_bin(N)] += (int64_t)(before[u + 1] - before[u]);
    }
    for (int64_t k = 0; k < n; ++k) {
        const uint32_t c = cls[(size_t)k];
        const uint32_t N = c < GSR_DEN_NOKEY ? cell_n[(size_t)(std::lower_bound(ukey.begin(), ukey.end(), c) - ukey.begin())] : 0u;
        hit_out[k] = gsr_density_hit(rule, c == GSR_DEN_OUTSIDE ? GSR_DEN_CNT_OUTSIDE : N) ? 1 : 0;
        if (counts_out) counts_out[k] = N;
    }
    if (result) *result = res;
    return GSR_OK;
}

extern "C" int gsr_get_select_density(gsr_context* c, int64_t* calls, int64_t* hit_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_select_density: ctx is NULL");
    return c->seld.report(calls, hit_last, ms);
}

extern "C" int gsr_select_density(gsr_context* c, const gsr_density_rule* r, uint32_t* mask, int mask_is_device, uint32_t* counts_out,
                                  int counts_is_device, gsr_density_result* result, int64_t* n_hit, int64_t* n_set)
{
    const char* const who = "gsr_select_density";
    if (!c || !r || !mask) return set_err(GSR_E_INVALID, "gsr_select_density: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const char* bad = density_rule_error(r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_density: %s", bad);
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask or the counts exists
        if (n_hit) *n_hit = 0;
        if (n_set) *n_set = 0;
        if (result) std::memset(result, 0, sizeof *result);
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const MaskArg mk{mask, mask_is_device != 0, n};
    if ((rc = mk.check(c, who))) return rc;            // before anything is launched: a wrong pointer must never be found out by a kernel
    const bool counts_dev = counts_out && counts_is_device;
    if (counts_dev && (rc = check_device_source(c, counts_out, (size_t)n * 4, who, "counts_out"))) return rc;
    // the sort's scratch is shared with the frames' sorts and an upload's: nothing may be in flight (this also waits for whoever
    // produced a device mask on the public stream)
    if ((rc = sync_all(c))) return rc;
    // ---- everything the call needs, before the launch: a host mask, host counts and the result block are placed in the arena
    FrameSlot& sl = c->slot[0];
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oMask = place(mk.stage_bytes()), oRes = place((size_t)GSR_DEN_R_WORDS * 4), oCounts = place(counts_out && !counts_dev ? (size_t)n * 4 : 0);
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    if ((rc = ensure_stage(c, off)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 4, who, true)) || (rc = ensure_sel_counters(c, who)))
        return rc;
    if (!c->den_h && c->den_h.alloc((size_t)GSR_DEN_R_WORDS, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "gsr_select_density: no pinned host memory for the result");
    }
    if (c->up_sort.hold(n)) return set_err(GSR_E_OOM, "gsr_select_density: no room for the sort of the cell keys");
    if ((rc = ensure_counts(sl.hist, (size_t)512 * div_up(n, (uint32_t)RS_THREADS * (uint32_t)RS_ITEMS) + 8))) return rc;
    if ((rc = c->den_cnt.ensure((size_t)n, (size_t)n + n / 8 + 1024))) return rc;
    HIP_TRY(hipStreamSynchronize(sl.own));             // the inverse of the storage order is built there
    hipStream_t us = sl.stream;                        // where radix_sort queues its passes
    uint32_t* const dmask = mk.is_device ? mask : reinterpret_cast<uint32_t*>(c->stage + oMask);
    uint32_t* const dres = reinterpret_cast<uint32_t*>(c->stage + oRes);
    uint32_t* const dcounts = !counts_out ? nullptr : counts_dev ? counts_out : reinterpret_cast<uint32_t*>(c->stage + oCounts);
    double copy_ms = 0.0;
    if (!mk.is_device && r->op != GSR_SELECT_REPLACE) {               // every op but REPLACE reads the mask first
        const uint32_t* staged = nullptr;
        const hipError_t e = mk.to_device(c, us, oMask, &copy_ms, &staged);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_density: %s", hipGetErrorString(e));
    }
    const bool vis = c->vis_on, hide = vis && (r->flags & GSR_DENSITY_SKIP_HIDDEN);
    const GsrDensityRule rule = density_rule(r);
    const GsrVisRule vrule = hide ? c->vis : GsrVisRule{};
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    const float* const alpha0 = vis ? (const float*)c->alpha0 : nullptr;
    const uint32_t* const vis_mask = hide ? (const uint32_t*)c->vis_mask : nullptr;
    uint32_t *kA = c->up_sort.kA, *kB = c->up_sort.kB, *vA = c->up_sort.vA, *vB = c->up_sort.vB;
    const uint32_t nchunks = div_up(n, GSR_DENSITY_THREADS);
    const dim3 grid(nchunks), capped(std::min(nchunks, (uint32_t)GSR_DENSITY_BLOCKS)), block(GSR_DENSITY_THREADS);
    hipError_t e = hipMemsetAsync(c->sel_counters, 0, cwords * 8, us);
    if (e == hipSuccess) e = hipMemsetAsync(dres, 0, (size_t)GSR_DEN_R_WORDS * 4, us);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_density_keys, capped, block, 0, us, n, nchunks, inv, c->geoA, alpha0, vis_mask, hide ? 1 : 0, rule, vrule, kA, vA, c->den_cnt.get(), dres);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_density: %s", hipGetErrorString(e));
    // the 31-bit keys with their upload indices, in the instantiation morton_order launches (four 8-bit passes): the sentinels sort last
    if ((rc = radix_sort(sl, kA, vA, kB, vB, n, 31, true, (uint32_t*)nullptr, RS_XCD_DEPTH != 0))) return rc;   // (leaves the result in what kA / vA name now)
    e = hipEventRecord(c->up_ev[2], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_density_count, capped, block, 0, us, n, nchunks, (int)r->reach, kA, vA, c->den_cnt.get(), dres);
        hipLaunchKernelGGL(k_density_hit, grid, block, 0, us, n, rule, c->den_cnt.get(), dcounts, dmask, c->sel_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[3], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->sel_h_counters, c->sel_counters, cwords * 8, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipMemcpyAsync(c->den_h, dres, (size_t)GSR_DEN_R_WORDS * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_density: %s", hipGetErrorString(e));
    // the counts the kernels left must add up before a word of the caller's is written
    const uint32_t* const h = c->den_h;
    gsr_density_result res;
    std::memset(&res, 0, sizeof res);
    res.n_population = (int64_t)h[GSR_DEN_R_POP];
    res.n_outside = (int64_t)h[GSR_DEN_R_OUTSIDE];
    res.n_cells = (int64_t)h[GSR_DEN_R_CELLS];
    int64_t binned = 0;
    for (int b = 0; b < GSR_DEN_BINS; ++b) binned += (res.count_hist[b] = (int64_t)h[GSR_DEN_R_HIST + b]);
    if (res.n_population + res.n_outside > (int64_t)n || res.n_cells > res.n_population || binned != res.n_population)
        return set_err(GSR_E_HIP, "gsr_select_density: the kernels counted %lld population, %lld outside, %lld cells, %lld binned among %u splats",
                       (long long)res.n_population, (long long)res.n_outside, (long long)res.n_cells, (long long)binned, n);
    if (!mk.is_device) e = hipMemcpyAsync(mask, dmask, mk.words() * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess && counts_out && !counts_dev) e = hipMemcpyAsync(counts_out, dcounts, (size_t)n * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_density: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    unsigned long long hits = 0, set = 0;
    sum_sel_counters(c, &hits, &set);
    if (n_hit) *n_hit = (int64_t)hits;
    if (n_set) *n_set = (int64_t)set;
    if (result) *result = res;
    float ms = 0.0f, ms2 = 0.0f;
    c->seld.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess && hipEventElapsedTime(&ms2, c->up_ev[2], c->up_ev[3]) == hipSuccess ? (double)ms + (double)ms2 : 0.0;
    c->seld.ms[1] = copy_ms;
    c->seld.ms[2] = hipEventElapsedTime(&ms, c->up_ev[1], c->up_ev[2]) == hipSuccess ? (double)ms : 0.0;
    c->seld.ms[3] = up_now_ms() - t_begin;
    c->seld.calls += 1;
    c->seld.last = (int64_t)hits;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Selection by connectivity (k_connect.h).  gsr_select_density's grid, population, key kernel, sort and waits; behind
// the sort a table of the occupied cells, a union-find over it and gsr_select's epilogue.  The per-splat size words are the density
// verb's count buffer (c->den_cnt: k_density_keys writes every word of it), the per-cell arrays the context's own (c->con_tab), the
// per-splat labels and the cell of each sorted entry live in the sort's B buffers, which hold nothing once the sort has ended.
static_assert(GSR_CONNECT_SKIP_HIDDEN == GSR_DENF_SKIP_HIDDEN && GSR_CONNECT_HIT_OUTSIDE == GSR_DENF_HIT_OUTSIDE && GSR_CONNECT_CELLS == GSR_DEN_CELLS &&
              GSR_CONNECT_MAX_REACH == GSR_DENSITY_MAX_REACH && GSR_CONNECT_HIST_BINS == GSR_CON_BINS && GSR_CONNECT_NO_LABEL == GSR_CON_NOLABEL,
              "the header's flags and limits are the kernels'");
static_assert(sizeof(gsr_connect_rule) == 44 && offsetof(gsr_connect_rule, origin) == 4 && offsetof(gsr_connect_rule, reach) == 16 &&
              offsetof(gsr_connect_rule, flags) == 20 && offsetof(gsr_connect_rule, op) == 24 && offsetof(gsr_connect_rule, reserved_) == 28 &&
              offsetof(gsr_connect_rule, size_lo) == 32 && offsetof(gsr_connect_rule, size_hi) == 36 && offsetof(gsr_connect_rule, alpha_min) == 40,
              "the rule is the density rule's 11 dwords, the size range in the place of the count range");
static_assert(sizeof(gsr_connect_result) == 8 * (6 + 2 * GSR_CONNECT_HIST_BINS) && offsetof(gsr_connect_result, n_components) == 24 &&
              offsetof(gsr_connect_result, comp_hist) == 48 && offsetof(gsr_connect_result, splat_hist) == 48 + 8 * GSR_CONNECT_HIST_BINS,
              "the result is 70 counts");
#define GSR_CON_TAB_ARRAYS 7           // ckey, cstart, parent, croot, csize, clabel, cseed: n + 1 words each

// the density rule that has the connect rule's grid, population and flags: what is wrong with one is what is wrong with the other
static gsr_density_rule connect_as_density(const gsr_connect_rule* r)
{
    gsr_density_rule d{};
    d.cell = r->cell;
    for (int k = 0; k < 3; ++k) d.origin[k] = r->origin[k];
    d.reach = r->reach; d.flags = r->flags; d.op = r->op; d.reserved_ = r->reserved_;
    d.count_lo = 0u; d.count_hi = 0u;
    d.alpha_min = r->alpha_min;
    return d;
}
static GsrConnectRule connect_rule(const gsr_connect_rule* r, bool has_seed)
{
    const gsr_density_rule d = connect_as_density(r);
    GsrConnectRule k{};
    k.den = density_rule(&d);
    k.size_lo = r->size_lo; k.size_hi = r->size_hi;
    k.has_seed = has_seed ? 1 : 0;
    return k;
}

// The rule on the host.  The classes come from gsr_density_class; the table is the sorted unique keys, as gsr_select_density_eval
// builds it, with each cell's population, smallest upload index and seed mark; the components come from a SEQUENTIAL union-find over
// the rows of gsr_connect_row with the kernels' hook rule (gsr_connect_hook), the verdict from gsr_connect_hit.
extern "C" int gsr_select_connected_eval(const gsr_connect_rule* r, const gsr_visibility* vis, int64_t n, const float* P, const float* alpha,
                                         const uint32_t* seed_bits, uint8_t* hit_out, uint32_t* labels_out, uint32_t* sizes_out, gsr_connect_result* result)
{
    if (!r) return set_err(GSR_E_INVALID, "gsr_select_connected_eval: rule is NULL");
    const gsr_density_rule as_density = connect_as_density(r);
    const char* bad = density_rule_error(&as_density);
    if (!bad) bad = visibility_error(vis);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_connected_eval: %s", bad);
    if (n < 0 || n > 0x7fffffffll || (n > 0 && (!P || !hit_out))) return set_err(GSR_E_INVALID, "gsr_select_connected_eval: bad argument");
    const gsr_visibility* const hide = (r->flags & GSR_CONNECT_SKIP_HIDDEN) ? vis : nullptr;   // (no visibility: nothing is hidden)
    const uint32_t* const vmask = hide ? hide->mask : nullptr;
    if (vmask && hide->mask_splats < n)
        return set_err(GSR_E_INVALID, "gsr_select_connected_eval: the visibility's mask covers %lld of the %lld splats", (long long)hide->mask_splats, (long long)n);
    const GsrConnectRule rule = connect_rule(r, seed_bits != nullptr);
    const GsrVisRule vr = visibility_rule(hide);
    gsr_connect_result res;
    std::memset(&res, 0, sizeof res);
    std::vector<uint32_t> cls((size_t)n);
    std::vector<std::pair<uint32_t, uint32_t>> pairs;  // (key, upload index) of the population: sorted, the index breaks ties as the stable sort does
    for (int64_t k = 0; k < n; ++k) {
        const float px = P[3 * k], py = P[3 * k + 1], pz = P[3 * k + 2];
        const bool hidden = hide && !gsr_splat_visible(vr, px, py, pz, vmask ? vmask[k >> 5] : 0u, (uint32_t)(k & 31));
        const uint32_t c = gsr_density_class(rule.den, px, py, pz, alpha ? alpha[k] : 1.0f, hidden);
        cls[(size_t)k] = c;
        if (c < GSR_DEN_NOKEY) pairs.emplace_back(c, (uint32_t)k);
        else if (c == GSR_DEN_OUTSIDE) res.n_outside += 1;
    }
    res.n_population = (int64_t)pairs.size();
    std::sort(pairs.begin(), pairs.end());
    // the cell table: ukey rising; per cell its population, its smallest upload index and whether it holds a seed
    std::vector<uint32_t> ukey, cpop, cmin, cseed;
    for (size_t k = 0; k < pairs.size(); ++k) {
        if (k == 0 || pairs[k].first != pairs[k - 1].first) { ukey.push_back(pairs[k].first); cpop.push_back(0u); cmin.push_back(pairs[k].second); cseed.push_back(0u); }
        cpop.back() += 1u;
        const uint32_t i = pairs[k].second;
        if (seed_bits && ((seed_bits[i >> 5] >> (i & 31u)) & 1u)) cseed.back() = 1u;
    }
    const size_t U = ukey.size();
    res.n_cells = (int64_t)U;
    std::vector<uint32_t> parent(U);
    for (size_t u = 0; u < U; ++u) parent[u] = (uint32_t)u;
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t u = 0; u < U; ++u)
        for (int dz = 0; dz <= rule.den.reach; ++dz)
            for (int dy = -rule.den.reach; dy <= rule.den.reach; ++dy) {
                uint32_t klo = 0u, khi = 0u;
                if (!gsr_connect_row(ukey[u], rule.den.reach, dy, dz, &klo, &khi)) continue;
                for (size_t p = (size_t)(std::lower_bound(ukey.begin(), ukey.end(), klo) - ukey.begin()); p < U && ukey[p] <= khi; ++p) {
                    const uint32_t a = find((uint32_t)u), b = find((uint32_t)p);
                    if (a == b) continue;
                    uint32_t under = 0u, over = 0u;
                    gsr_connect_hook(a, b, &under, &over);
                    parent[under] = over;
                }
            }
    // the tally per root: population, smallest upload index, seed
    std::vector<uint32_t> root(U), size(U, 0u), label(U, GSR_CON_NOLABEL), seeded(U, 0u);
    for (size_t u = 0; u < U; ++u) {
        const uint32_t t = root[u] = find((uint32_t)u);
        size[t] += cpop[u];
        label[t] = std::min(label[t], cmin[u]);
        seeded[t] |= cseed[u];
    }
    for (size_t u = 0; u < U; ++u) {
        if (root[u] != (uint32_t)u) continue;
        res.n_components += 1;
        res.n_seeded += seeded[u] ? 1 : 0;
        res.largest = std::max(res.largest, (int64_t)size[u]);
        res.comp_hist[gsr_connect_bin(size[u])] += 1;
        res.splat_hist[gsr_connect_bin(size[u])] += (int64_t)size[u];
    }
    for (int64_t k = 0; k < n; ++k) {
        const uint32_t c = cls[(size_t)k];
        uint32_t word = c == GSR_DEN_OUTSIDE ? GSR_DEN_CNT_OUTSIDE : 0u, lab = GSR_CON_NOLABEL;
        bool sd = false;
        if (c < GSR_DEN_NOKEY) {
            const uint32_t t = root[(size_t)(std::lower_bound(ukey.begin(), ukey.end(), c) - ukey.begin())];
            word = size[t]; lab = label[t]; sd = seeded[t] != 0u;
        }
        hit_out[k] = gsr_connect_hit(rule, word, sd) ? 1 : 0;
        if (labels_out) labels_out[k] = lab;
        if (sizes_out) sizes_out[k] = word & ~GSR_DEN_CNT_OUTSIDE;
    }
    if (result) *result = res;
    return GSR_OK;
}

extern "C" int gsr_get_select_connected(gsr_context* c, int64_t* calls, int64_t* hit_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_select_connected: ctx is NULL");
    return c->selc.report(calls, hit_last, ms);
}

extern "C" int gsr_debug_select_connected_stages(gsr_context* c, double ms[6])
{
    if (!c || !ms) return set_err(GSR_E_INVALID, "gsr_debug_select_connected_stages: NULL argument");
    for (int k = 0; k < 6; ++k) ms[k] = c->con_stage_ms[k];
    return GSR_OK;
}

extern "C" int gsr_select_connected(gsr_context* c, const gsr_connect_rule* r, const uint32_t* seed, int seed_is_device, uint32_t* mask, int mask_is_device,
                                    uint32_t* labels_out, uint32_t* sizes_out, int outs_are_device, gsr_connect_result* result, int64_t* n_hit, int64_t* n_set)
{
    const char* const who = "gsr_select_connected";
    if (!c || !r || !mask) return set_err(GSR_E_INVALID, "gsr_select_connected: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const gsr_density_rule as_density = connect_as_density(r);
    const char* bad = density_rule_error(&as_density);
    if (bad) return set_err(GSR_E_INVALID, "gsr_select_connected: %s", bad);
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask or the outputs exists
        if (n_hit) *n_hit = 0;
        if (n_set) *n_set = 0;
        if (result) std::memset(result, 0, sizeof *result);
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    // before anything is launched: a wrong pointer must never be found out by a kernel
    const MaskArg mk{mask, mask_is_device != 0, n};
    const MaskArg sk{seed, seed_is_device != 0, n};
    if ((rc = mk.check(c, who))) return rc;
    if (seed && sk.is_device && (rc = check_device_source(c, seed, sk.words() * 4, who, "seed"))) return rc;
    const bool outs_dev = outs_are_device != 0;
    if (labels_out && outs_dev && (rc = check_device_source(c, labels_out, (size_t)n * 4, who, "labels_out"))) return rc;
    if (sizes_out && outs_dev && (rc = check_device_source(c, sizes_out, (size_t)n * 4, who, "sizes_out"))) return rc;
    // the sort's scratch is shared with the frames' sorts and an upload's: nothing may be in flight (this also waits for whoever
    // produced a device mask or seed on the public stream)
    if ((rc = sync_all(c))) return rc;
    // ---- everything the call needs, before the launch: host masks, host outputs, the result block and the block counts in the arena
    FrameSlot& sl = c->slot[0];
    const uint32_t nblocks = div_up(n, (uint32_t)GSR_CONNECT_BLOCK);
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oMask = place(mk.stage_bytes()), oSeed = place(sk.stage_bytes()), oRes = place((size_t)GSR_CON_R_WORDS * 4);
    const size_t oCounts = place((size_t)nblocks * 4), oOffsets = place(((size_t)nblocks + 1) * 4);
    const size_t oLabels = place(labels_out && !outs_dev ? (size_t)n * 4 : 0), oSizes = place(sizes_out && !outs_dev ? (size_t)n * 4 : 0);
    const size_t cwords = (size_t)GSR_SEL_COUNTER_SLOTS * GSR_SEL_COUNTER_STRIDE;
    if ((rc = ensure_stage(c, off)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_sel_counters(c, who))) return rc;
    for (Event& ev : c->con_ev) {
        if (ev) continue;
        const hipError_t ee = ev.create(hipEventDefault);
        if (ee != hipSuccess) return set_err(ee == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "gsr_select_connected: no event: %s", hipGetErrorString(ee));
    }
    if (!c->con_h && c->con_h.alloc((size_t)GSR_CON_R_WORDS, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "gsr_select_connected: no pinned host memory for the result");
    }
    if (c->up_sort.hold(n)) return set_err(GSR_E_OOM, "gsr_select_connected: no room for the sort of the cell keys");
    if ((rc = ensure_counts(sl.hist, (size_t)512 * div_up(n, (uint32_t)RS_THREADS * (uint32_t)RS_ITEMS) + 8))) return rc;
    if ((rc = c->den_cnt.ensure((size_t)n, (size_t)n + n / 8 + 1024))) return rc;
    const size_t tab = (size_t)n + 1;                  // words per array of the table (cstart holds a sentinel behind the last cell)
    if ((rc = c->con_tab.ensure(tab * GSR_CON_TAB_ARRAYS, (tab + tab / 8 + 1024) * GSR_CON_TAB_ARRAYS))) return rc;
    HIP_TRY(hipStreamSynchronize(sl.own));             // the inverse of the storage order is built there
    hipStream_t us = sl.stream;                        // where radix_sort queues its passes
    uint32_t* const dmask = mk.is_device ? mask : reinterpret_cast<uint32_t*>(c->stage + oMask);
    uint32_t* const dres = reinterpret_cast<uint32_t*>(c->stage + oRes);
    uint32_t* const dcounts = reinterpret_cast<uint32_t*>(c->stage + oCounts);
    uint32_t* const doffsets = reinterpret_cast<uint32_t*>(c->stage + oOffsets);
    uint32_t* const dlabels = !labels_out ? nullptr : outs_dev ? labels_out : reinterpret_cast<uint32_t*>(c->stage + oLabels);
    uint32_t* const dsizes = !sizes_out ? nullptr : outs_dev ? sizes_out : reinterpret_cast<uint32_t*>(c->stage + oSizes);
    uint32_t* const t0 = c->con_tab.get();
    uint32_t *const ckey = t0, *const cstart = t0 + tab, *const parent = t0 + 2 * tab, *const croot = t0 + 3 * tab, *const csize = t0 + 4 * tab,
             *const clabel = t0 + 5 * tab, *const cseed = t0 + 6 * tab;
    double copy_ms = 0.0;
    const uint32_t* dseed = nullptr;
    if (seed) {                                        // a host seed goes to its own place in the arena: it may be the host mask itself
        const hipError_t e = sk.to_device(c, us, oSeed, &copy_ms, &dseed);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_connected: %s", hipGetErrorString(e));
    }
    if (!mk.is_device && r->op != GSR_SELECT_REPLACE) {               // every op but REPLACE reads the mask first
        const uint32_t* staged = nullptr;
        const hipError_t e = mk.to_device(c, us, oMask, &copy_ms, &staged);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_connected: %s", hipGetErrorString(e));
    }
    const bool vis = c->vis_on, hide = vis && (r->flags & GSR_CONNECT_SKIP_HIDDEN);
    const GsrConnectRule rule = connect_rule(r, seed != nullptr);
    const GsrVisRule vrule = hide ? c->vis : GsrVisRule{};
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    const float* const alpha0 = vis ? (const float*)c->alpha0 : nullptr;
    const uint32_t* const vis_mask = hide ? (const uint32_t*)c->vis_mask : nullptr;
    uint32_t *kA = c->up_sort.kA, *kB = c->up_sort.kB, *vA = c->up_sort.vA, *vB = c->up_sort.vB;
    const uint32_t nchunks = div_up(n, GSR_CONNECT_THREADS);
    const dim3 grid(nchunks), capped(std::min(nchunks, (uint32_t)GSR_DENSITY_BLOCKS)), block(GSR_CONNECT_THREADS);
    Event* const ev = c->con_ev;
    hipError_t e = hipMemsetAsync(c->sel_counters, 0, cwords * 8, us);
    if (e == hipSuccess) e = hipMemsetAsync(dres, 0, (size_t)GSR_CON_R_WORDS * 4, us);
    if (e == hipSuccess) e = hipEventRecord(ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_density_keys, capped, block, 0, us, n, nchunks, inv, c->geoA, alpha0, vis_mask, hide ? 1 : 0, rule.den, vrule, kA, vA, c->den_cnt.get(), dres);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_connected: %s", hipGetErrorString(e));
    // the 31-bit keys with their upload indices, in the instantiation morton_order launches (four 8-bit passes): the sentinels sort last
    if ((rc = radix_sort(sl, kA, vA, kB, vB, n, 31, true, (uint32_t*)nullptr, RS_XCD_DEPTH != 0))) return rc;   // (leaves the result in what kA / vA name now)
    uint32_t *const ulabel = kB, *const cidx = vB;     // the other two buffers are free from here on
    e = hipEventRecord(ev[2], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_connect_mark, dim3(nblocks), block, 0, us, n, kA, dres, dcounts);
        hipLaunchKernelGGL(k_remove_scan, dim3(1), dim3(GSR_REMOVE_SCAN_THREADS), 0, us, nblocks, dcounts, doffsets);
        hipLaunchKernelGGL(k_connect_table, dim3(nblocks), block, 0, us, n, kA, dres, doffsets, ckey, cstart, parent, csize, clabel, cseed, cidx);
        if (dseed) hipLaunchKernelGGL(k_connect_seed, capped, block, 0, us, n, nchunks, vA, dres, dseed, cidx, cseed);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[3], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_connect_link, capped, block, 0, us, n, nchunks, (int)r->reach, dres, ckey, parent);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[4], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_connect_flatten, capped, block, 0, us, n, nchunks, dres, vA, cstart, parent, cseed, croot, csize, clabel);
        hipLaunchKernelGGL(k_connect_stats, capped, block, 0, us, n, nchunks, croot, csize, dres);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[5], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_connect_scatter, capped, block, 0, us, n, nchunks, dres, vA, cidx, croot, csize, clabel, c->den_cnt.get(), ulabel);
        hipLaunchKernelGGL(k_connect_hit, grid, block, 0, us, n, rule, c->den_cnt.get(), ulabel, dlabels, dsizes, dmask, c->sel_counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[6], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->sel_h_counters, c->sel_counters, cwords * 8, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipMemcpyAsync(c->con_h, dres, (size_t)GSR_CON_R_WORDS * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_connected: %s", hipGetErrorString(e));
    // the counts the kernels left must add up before a word of the caller's is written
    const uint32_t* const h = c->con_h;
    gsr_connect_result res;
    std::memset(&res, 0, sizeof res);
    res.n_population = (int64_t)h[GSR_CON_R_POP];
    res.n_outside = (int64_t)h[GSR_CON_R_OUTSIDE];
    res.n_cells = (int64_t)h[GSR_CON_R_CELLS];
    res.n_components = (int64_t)h[GSR_CON_R_COMPS];
    res.n_seeded = (int64_t)h[GSR_CON_R_SEEDED];
    res.largest = (int64_t)h[GSR_CON_R_LARGEST];
    int64_t comps = 0, binned = 0;
    for (int b = 0; b < GSR_CON_BINS; ++b) {
        comps += (res.comp_hist[b] = (int64_t)h[GSR_CON_R_CHIST + b]);
        binned += (res.splat_hist[b] = (int64_t)h[GSR_CON_R_SHIST + b]);
    }
    if (res.n_population + res.n_outside > (int64_t)n || res.n_cells > res.n_population || res.n_components > res.n_cells || comps != res.n_components ||
        binned != res.n_population || res.n_seeded > res.n_components || res.largest > res.n_population)
        return set_err(GSR_E_HIP, "gsr_select_connected: the kernels counted %lld population, %lld outside, %lld cells, %lld components (%lld binned, %lld splats "
                       "binned, largest %lld) among %u splats", (long long)res.n_population, (long long)res.n_outside, (long long)res.n_cells,
                       (long long)res.n_components, (long long)comps, (long long)binned, (long long)res.largest, n);
    if (!mk.is_device) e = hipMemcpyAsync(mask, dmask, mk.words() * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess && labels_out && !outs_dev) e = hipMemcpyAsync(labels_out, dlabels, (size_t)n * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess && sizes_out && !outs_dev) e = hipMemcpyAsync(sizes_out, dsizes, (size_t)n * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_select_connected: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    unsigned long long hits = 0, set = 0;
    sum_sel_counters(c, &hits, &set);
    if (n_hit) *n_hit = (int64_t)hits;
    if (n_set) *n_set = (int64_t)set;
    if (result) *result = res;
    double total = 0.0;
    for (int k = 0; k < 6; ++k) {
        float ms = 0.0f;
        c->con_stage_ms[k] = hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess ? (double)ms : 0.0;
        if (k != 1) total += c->con_stage_ms[k];
    }
    c->selc.ms[0] = total;
    c->selc.ms[1] = copy_ms;
    c->selc.ms[2] = c->con_stage_ms[1];
    c->selc.ms[3] = up_now_ms() - t_begin;
    c->selc.calls += 1;
    c->selc.last = (int64_t)hits;
    return GSR_OK;
}
