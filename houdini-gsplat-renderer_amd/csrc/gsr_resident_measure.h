// gsr_resident_measure.h -- the verbs that measure a selection of resident splats: gsr_measure, gsr_measure_eval,
// gsr_hist_prepare, gsr_get_measure.  Host code only; included once, behind gsr_resident_select.h, whose contract it keeps and whose
// refusals (refuse_edit), pointer check (check_device_source), mask intake (MaskArg) and visibility rule (visibility_error,
// visibility_rule) it shares.  The rule and the kernels are k_measure.h's.
//
// A measure writes NOTHING the context keeps but its own tally: no resident bit, no horizon, no cached order, no policy, no
// visibility state, no entry of gsr_stats.  It therefore does not wait for the frames in flight, and the next frame runs the launches
// it would have run.  What it uses of the context: slot 0's own stream, the first three events of the upload clock, the inverse of the
// storage order (built on first use per geometry), the staging arena -- idle, because an upload in progress is refused -- for a host
// mask, the result block and the tree's partial sums, and pinned words of its own for the result.
#pragma once

static_assert(GSR_MEASURE_BOUNDS == GSR_MEASW_BOUNDS && GSR_MEASURE_EXTENT == GSR_MEASW_EXTENT && GSR_MEASURE_MOMENTS == GSR_MEASW_MOMENTS &&
              GSR_MEASURE_SKIP_HIDDEN == GSR_MEASF_SKIP_HIDDEN && GSR_HIST_X == GSR_HISTC_X && GSR_HIST_Y == GSR_HISTC_Y && GSR_HIST_Z == GSR_HISTC_Z &&
              GSR_HIST_ALPHA == GSR_HISTC_ALPHA && GSR_HIST_SCALE_MAX == GSR_HISTC_SCALE_MAX && GSR_HIST_SCALE_MIN == GSR_HISTC_SCALE_MIN &&
              GSR_HIST_CD_R == GSR_HISTC_CD_R && GSR_HIST_CD_G == GSR_HISTC_CD_G && GSR_HIST_CD_B == GSR_HISTC_CD_B && GSR_HIST_LOG2 == GSR_HISTF_LOG2 &&
              GSR_HIST_MAX_BINS == GSR_MEAS_BINS && GSR_MEASURE_MAX_HIST == GSR_MEAS_HISTS, "the header's bits, channels and limits are the kernel's");
static_assert(sizeof(gsr_hist_spec) == sizeof(GsrHistSpec) && offsetof(gsr_hist_spec, bins) == offsetof(GsrHistSpec, bins) &&
              offsetof(gsr_hist_spec, inv_w) == offsetof(GsrHistSpec, inv_w) && sizeof(gsr_measure_request) == sizeof(GsrMeasureRule) &&
              offsetof(gsr_measure_request, ref) == offsetof(GsrMeasureRule, ref) && offsetof(gsr_measure_request, extent_k) == offsetof(GsrMeasureRule, extent_k) &&
              offsetof(gsr_measure_request, n_hist) == offsetof(GsrMeasureRule, n_hist) && offsetof(gsr_measure_request, hist) == offsetof(GsrMeasureRule, hist) &&
              offsetof(gsr_measure_request, reserved_) == offsetof(GsrMeasureRule, reserved_), "gsr_measure_request is the kernel's rule");
static_assert(sizeof(gsr_measure_result) == 144 && offsetof(gsr_measure_result, lo) == 24 && offsetof(gsr_measure_result, sum) == 72, "the result is 3 counts, 12 floats, 9 doubles");

// what is wrong with a spec (NULL: nothing): what gsr_hist_prepare could not have made
static const char* hist_spec_error(const gsr_hist_spec* s)
{
    if (s->channel < 0 || s->channel >= GSR_HISTC_COUNT) return "unknown histogram channel";
    if (s->flags & ~GSR_HIST_LOG2) return "unknown histogram flag bits";
    if (s->bins < 1 || s->bins > GSR_HIST_MAX_BINS) return "bins is not within 1..GSR_HIST_MAX_BINS";
    if (!std::isfinite(s->lo) || !std::isfinite(s->hi)) return "a histogram's bounds are not finite";
    if (!(s->lo < s->hi)) return "a histogram's hi is not above its lo";
    if (!std::isfinite(s->inv_w) || !(s->inv_w > 0.0f)) return "a histogram's inv_w is not a finite positive number";
    return nullptr;
}
// what is wrong with the caller's request (NULL: nothing)
static const char* measure_request_error(const gsr_measure_request* r)
{
    if (r->what & ~GSR_MEASW_ALL) return "unknown bits in what";
    if (r->flags & ~GSR_MEASURE_SKIP_HIDDEN) return "unknown flag bits";
    if (r->reserved_ != 0) return "reserved_ is not 0";
    if (!std::isfinite(r->ref[0]) || !std::isfinite(r->ref[1]) || !std::isfinite(r->ref[2])) return "ref is not finite";
    if (!std::isfinite(r->extent_k)) return "extent_k is not finite";
    if (r->n_hist < 0 || r->n_hist > GSR_MEASURE_MAX_HIST) return "n_hist is not within 0..GSR_MEASURE_MAX_HIST";
    for (int h = 0; h < r->n_hist; ++h) {
        const char* bad = hist_spec_error(&r->hist[h]);
        if (bad) return bad;
    }
    return nullptr;
}
// the request as the kernel takes it (specs beyond n_hist zeroed)
static GsrMeasureRule measure_rule(const gsr_measure_request* r)
{
    GsrMeasureRule m{};
    std::memcpy(&m, r, offsetof(GsrMeasureRule, hist));
    std::memcpy(m.hist, r->hist, sizeof(GsrHistSpec) * (size_t)r->n_hist);
    return m;
}
// which of gsr_read's arrays a request looks at: 1 P, 2 alpha, 4 scale, 8 Cd (hide_by_volumes: SKIP_HIDDEN under volumes in force)
static int measure_needs(const gsr_measure_request* r, bool hide_by_volumes)
{
    int needs = (r->what & GSR_MEASW_ALL) || hide_by_volumes ? 1 : 0;
    if (r->what & GSR_MEASURE_EXTENT) needs |= 4;
    for (int h = 0; h < r->n_hist; ++h) {
        const int ch = r->hist[h].channel;
        needs |= ch <= GSR_HIST_Z ? 1 : ch == GSR_HIST_ALPHA ? 2 : ch <= GSR_HIST_SCALE_MIN ? 4 : 8;
    }
    return needs;
}
// the words the specs' counts take, back to back
static size_t measure_hist_words(const gsr_measure_request* r)
{
    size_t words = 0;
    for (int h = 0; h < r->n_hist; ++h) words += (size_t)r->hist[h].bins + 3;
    return words;
}
// the empty result: what no splat leaves
static void measure_empty(gsr_measure_result* out)
{
    std::memset(out, 0, sizeof *out);
    for (int k = 0; k < 3; ++k) { out->lo[k] = out->lo_e[k] = INFINITY; out->hi[k] = out->hi_e[k] = -INFINITY; }
}

extern "C" int gsr_hist_prepare(int channel, int flags, double lo, double hi, int bins, gsr_hist_spec* out)
{
    if (!out) return set_err(GSR_E_INVALID, "gsr_hist_prepare: out is NULL");
    if (!std::isfinite(lo) || !std::isfinite(hi)) return set_err(GSR_E_INVALID, "gsr_hist_prepare: a histogram's bounds are not finite");
    gsr_hist_spec s{};
    s.channel = channel; s.flags = flags; s.bins = bins;
    s.lo = (float)lo; s.hi = (float)hi;
    const double width = (double)s.hi - (double)s.lo;
    s.inv_w = width > 0.0 && bins >= 1 ? (float)((double)bins / width) : 1.0f;   // (a bad range or bin count is refused below, not divided by)
    const char* bad = hist_spec_error(&s);
    if (bad) return set_err(GSR_E_INVALID, "gsr_hist_prepare: %s", bad);
    *out = s;
    return GSR_OK;
}

// The tree of k_measure.h on the host, one leaf at a time: level[l] holds the finished node over 2^l leaves that waits for its right
// sibling (a binary counter); root() joins what waits with the +0.0 leaves behind n, level by level, exactly as the tree does.
struct MeasureTree {
    double level[33][9];
    uint64_t leaves = 0;
    void push(const double t[9])
    {
        double carry[9];
        for (int k = 0; k < 9; ++k) carry[k] = t[k];
        int l = 0;
        for (uint64_t c = leaves; c & 1u; c >>= 1, ++l)
            for (int k = 0; k < 9; ++k) carry[k] = level[l][k] + carry[k];
        for (int k = 0; k < 9; ++k) level[l][k] = carry[k];
        ++leaves;
    }
    // the root of the tree over 2^levels >= leaves leaves
    void root(int levels, double out[9]) const
    {
        if (leaves == (1ull << levels)) {
            for (int k = 0; k < 9; ++k) out[k] = level[levels][k];
            return;
        }
        double cur[9];                                   // the node over the aligned 2^l leaves that hold leaf `leaves`: +0.0 at l = 0
        for (int k = 0; k < 9; ++k) cur[k] = 0.0;
        for (int l = 0; l < levels; ++l)
            for (int k = 0; k < 9; ++k) cur[k] = ((leaves >> l) & 1u) ? level[l][k] + cur[k] : cur[k] + 0.0;
        for (int k = 0; k < 9; ++k) out[k] = cur[k];
    }
};
// the levels of the tree over n splats: the smallest 2^levels >= max(n, 64)
static int measure_tree_levels(uint64_t n)
{
    int levels = 6;
    while ((1ull << levels) < n) ++levels;
    return levels;
}

extern "C" int gsr_measure_eval(const gsr_measure_request* r, const gsr_visibility* vis, int64_t n, const uint32_t* mask, const float* P,
                                const float* alpha, const uint16_t* scale, const uint16_t* Cd, gsr_measure_result* out, uint32_t* hist_out)
{
    if (!r || !out) return set_err(GSR_E_INVALID, "gsr_measure_eval: NULL argument");
    const char* bad = measure_request_error(r);
    if (!bad) bad = visibility_error(vis);
    if (bad) return set_err(GSR_E_INVALID, "gsr_measure_eval: %s", bad);
    if ((r->n_hist > 0) != (hist_out != nullptr)) return set_err(GSR_E_INVALID, "gsr_measure_eval: hist_out is NULL iff n_hist is 0");
    if (n < 0 || n > 0x7fffffffll) return set_err(GSR_E_INVALID, "gsr_measure_eval: bad argument");
    const gsr_visibility* const hide = (r->flags & GSR_MEASURE_SKIP_HIDDEN) ? vis : nullptr;   // (no visibility: nothing is hidden)
    const uint32_t* const vmask = hide ? hide->mask : nullptr;
    if (vmask && hide->mask_splats < n)
        return set_err(GSR_E_INVALID, "gsr_measure_eval: the visibility's mask covers %lld of the %lld splats", (long long)hide->mask_splats, (long long)n);
    const int needs = measure_needs(r, hide && hide->n_volumes > 0);
    if (n > 0 && (((needs & 1) && !P) || ((needs & 2) && !alpha) || ((needs & 4) && !scale) || ((needs & 8) && !Cd)))
        return set_err(GSR_E_INVALID, "gsr_measure_eval: an array the request needs is NULL");
    const GsrMeasureRule rule = measure_rule(r);
    const GsrVisRule vr = visibility_rule(hide);
    const int what = r->what;
    gsr_measure_result res;
    measure_empty(&res);
    std::vector<uint32_t> hist(measure_hist_words(r), 0u);
    uint32_t enc[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    std::vector<MeasureTree> tree_box((what & GSR_MEASURE_MOMENTS) && n > 0 ? 1 : 0);
    MeasureTree* const tree = tree_box.empty() ? nullptr : tree_box.data();
    const double zeros[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i) {
        double t[9];
        for (int k = 0; k < 9; ++k) t[k] = zeros[k];
        bool sel = mask ? ((mask[i >> 5] >> (i & 31)) & 1u) != 0u : true;
        const float px = P ? P[3 * i] : 0.0f, py = P ? P[3 * i + 1] : 0.0f, pz = P ? P[3 * i + 2] : 0.0f;
        if (sel && hide && !gsr_splat_visible(vr, px, py, pz, vmask ? vmask[i >> 5] : 0u, (uint32_t)(i & 31))) sel = false;
        if (sel) {
            const uint16_t* const s = scale ? scale + 3 * i : nullptr;
            const uint16_t* const d = Cd ? Cd + 3 * i : nullptr;
            const uint32_t s0 = s ? s[0] : 0u, s1 = s ? s[1] : 0u, s2 = s ? s[2] : 0u;
            res.n_selected += 1;
            if ((what & GSR_MEASW_ALL) && gsr_meas_finite(px) && gsr_meas_finite(py) && gsr_meas_finite(pz)) {
                res.n_measured += 1;
                const float p[3] = {px, py, pz};
                if (what & GSR_MEASURE_BOUNDS)
                    for (int k = 0; k < 3; ++k) {
                        enc[k] = std::max(enc[k], gsr_meas_enc_lo(p[k]));
                        enc[3 + k] = std::max(enc[3 + k], gsr_meas_enc_hi(p[k]));
                    }
                if ((what & GSR_MEASURE_EXTENT) && gsr_meas_half_finite(s0) && gsr_meas_half_finite(s1) && gsr_meas_half_finite(s2)) {
                    res.n_extent += 1;
                    float smax, smin;
                    gsr_meas_scales(s0, s1, s2, &smax, &smin);
                    for (int k = 0; k < 3; ++k) {
                        enc[6 + k] = std::max(enc[6 + k], gsr_meas_enc_lo(__builtin_fmaf(-rule.extent_k, smax, p[k])));
                        enc[9 + k] = std::max(enc[9 + k], gsr_meas_enc_hi(__builtin_fmaf(rule.extent_k, smax, p[k])));
                    }
                }
                if (what & GSR_MEASURE_MOMENTS) gsr_meas_terms(rule.ref, px, py, pz, t);
            }
            size_t at = 0;
            for (int h = 0; h < rule.n_hist; ++h) {
                const float x = gsr_meas_channel(rule.hist[h].channel, px, py, pz, alpha ? alpha[i] : 0.0f, s0, s1, s2, d ? d[0] : 0u, d ? d[1] : 0u, d ? d[2] : 0u);
                hist[at + (size_t)gsr_meas_slot(rule.hist[h], x)] += 1u;
                at += (size_t)rule.hist[h].bins + 3;
            }
        }
        if (tree) tree->push(t);
    }
    for (int k = 0; k < 3; ++k) {
        if (enc[k]) res.lo[k] = gsr_meas_dec_lo(enc[k]);
        if (enc[3 + k]) res.hi[k] = gsr_meas_dec_hi(enc[3 + k]);
        if (enc[6 + k]) res.lo_e[k] = gsr_meas_dec_lo(enc[6 + k]);
        if (enc[9 + k]) res.hi_e[k] = gsr_meas_dec_hi(enc[9 + k]);
    }
    if (tree) tree->root(measure_tree_levels((uint64_t)n), res.sum);
    *out = res;
    if (!hist.empty()) std::memcpy(hist_out, hist.data(), hist.size() * 4);
    return GSR_OK;
}

extern "C" int gsr_get_measure(gsr_context* c, int64_t* calls, int64_t* measured_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_measure: ctx is NULL");
    return c->meas.report(calls, measured_last, ms);
}

extern "C" int gsr_measure(gsr_context* c, const uint32_t* mask, int mask_is_device, const gsr_measure_request* r, gsr_measure_result* out,
                           uint32_t* hist_out)
{
    const char* const who = "gsr_measure";
    if (!c || !r || !out) return set_err(GSR_E_INVALID, "gsr_measure: NULL argument");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const char* bad = measure_request_error(r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_measure: %s", bad);
    if ((r->n_hist > 0) != (hist_out != nullptr)) return set_err(GSR_E_INVALID, "gsr_measure: hist_out is NULL iff n_hist is 0");
    const size_t hist_words = measure_hist_words(r);
    const uint32_t n = c->n;
    if (n == 0) {                                      // the empty cloud: no word of the mask exists, and nothing is launched
        measure_empty(out);
        if (hist_words) std::memset(hist_out, 0, hist_words * 4);
        return GSR_OK;
    }
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const MaskArg mk{mask, mask_is_device != 0, n};
    if ((rc = mk.check(c, who))) return rc;            // before anything is launched: a wrong pointer must never be found out by a kernel
    if (mk.is_device && mask && c->stream) HIP_TRY(hipStreamSynchronize(c->stream));   // a producer of the mask on the public stream has finished
    // ---- the tree above the chunks: level 0 holds a node per chunk, every further level one per 256 of the level below; the last
    // launch joins exactly the power of two the tree still spans and writes the result block
    const bool moments = (r->what & GSR_MEASURE_MOMENTS) != 0;
    const uint32_t nchunks = div_up(n, GSR_MEASURE_THREADS);
    const int levels = measure_tree_levels(n);
    const int top_waves = levels >= 8 ? 4 : 1 << (levels - 6);
    struct Fold { uint32_t m; int span; size_t in, out; };   // (out = 0: the result block)
    std::vector<Fold> folds;
    // ---- everything the call needs, before the launch: a host mask, the result block and the partial sums are placed in the arena
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oMask = place(mk.stage_bytes()), oRes = place((size_t)GSR_MEAS_R_WORDS * 4);
    size_t oPart = 0;                                  // where k_measure's chunk nodes go (0: the result block)
    if (moments && nchunks > 1) {
        oPart = place((size_t)nchunks * 72);
        uint64_t span = 1;
        while (span < nchunks) span <<= 1;
        size_t in = oPart;
        for (uint32_t m = nchunks; m > 1;) {
            const uint32_t m_out = div_up(m, 256u);
            const bool last = span <= 256;
            const size_t o = last ? 0 : place((size_t)m_out * 72);
            folds.push_back(Fold{m, last ? (int)span : 256, in, o});
            m = m_out; span = last ? 1 : span / 256; in = o;
        }
    }
    if ((rc = ensure_stage(c, off)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 3, who, true))) return rc;
    if (!c->meas_h && c->meas_h.alloc((size_t)GSR_MEAS_R_WORDS, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "gsr_measure: no pinned host memory for the result");
    }
    hipStream_t us = c->slot[0].own;
    double copy_ms = 0.0;
    const uint32_t* dmask = nullptr;
    hipError_t e = mk.to_device(c, us, oMask, &copy_ms, &dmask);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_measure: %s", hipGetErrorString(e));
    // what a lane loads (k_select_attrs.h's word): only what the request and the visibility in force need
    const bool vis = c->vis_on, hide = vis && (r->flags & GSR_MEASURE_SKIP_HIDDEN);
    const int needs = measure_needs(r, hide && c->vis.n_volumes > 0);
    int loads = 0;
    if (needs & 1) loads |= GSR_ATTRL_GEOA;
    if (needs & 2) loads |= vis ? GSR_ATTRL_ALPHA0 : GSR_ATTRL_GEOA;
    if (needs & 4) loads |= GSR_ATTRL_GEOB;
    if (needs & 8) loads |= GSR_ATTRL_COL;
    if (hide) loads |= GSR_ATTRL_HIDDEN;
    const GsrMeasureRule rule = measure_rule(r);
    const GsrVisRule vrule = hide ? c->vis : GsrVisRule{};
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    const float* const alpha0 = vis ? (const float*)c->alpha0 : nullptr;
    const uint32_t* const vis_mask = hide ? (const uint32_t*)c->vis_mask : nullptr;
    uint32_t* const dres = reinterpret_cast<uint32_t*>(c->stage + oRes);
    double* const dsums = reinterpret_cast<double*>(dres + GSR_MEAS_R_SUMS);
    auto nodes = [&](size_t at) { return at ? reinterpret_cast<double*>(c->stage + at) : dsums; };
    const size_t res_words = (size_t)GSR_MEAS_R_HIST + hist_words;
    e = hipMemsetAsync(dres, 0, res_words * 4, us);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_measure, dim3(std::min(nchunks, (uint32_t)GSR_MEASURE_BLOCKS)), dim3(GSR_MEASURE_THREADS), 0, us, n, nchunks, loads, top_waves, inv,
                           c->geoA, c->geoB, c->col, alpha0, vis_mask, dmask, rule, vrule, dres, moments ? nodes(oPart) : (double*)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    for (const Fold& f : folds) {
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_measure_fold, dim3(div_up(f.m, 256u)), dim3(256), 0, us, f.m, f.span, nodes(f.in), nodes(f.out));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t1 = up_now_ms();
    if (e == hipSuccess) e = hipMemcpyAsync(c->meas_h, dres, res_words * 4, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_measure: %s", hipGetErrorString(e));
    copy_ms += up_now_ms() - t1;
    const uint32_t* const h = c->meas_h;
    gsr_measure_result res;
    measure_empty(&res);
    res.n_selected = (int64_t)h[GSR_MEAS_R_COUNTS];
    res.n_measured = (int64_t)h[GSR_MEAS_R_COUNTS + 1];
    res.n_extent = (int64_t)h[GSR_MEAS_R_COUNTS + 2];
    if (res.n_selected > (int64_t)n || res.n_measured > res.n_selected || res.n_extent > res.n_measured)
        return set_err(GSR_E_HIP, "gsr_measure: the reduction counted %lld selected, %lld measured, %lld with an extent among %u splats",
                       (long long)res.n_selected, (long long)res.n_measured, (long long)res.n_extent, n);
    const uint32_t* const enc = h + GSR_MEAS_R_BOUNDS;
    for (int k = 0; k < 3; ++k) {
        if (enc[k]) res.lo[k] = gsr_meas_dec_lo(enc[k]);
        if (enc[3 + k]) res.hi[k] = gsr_meas_dec_hi(enc[3 + k]);
        if (enc[6 + k]) res.lo_e[k] = gsr_meas_dec_lo(enc[6 + k]);
        if (enc[9 + k]) res.hi_e[k] = gsr_meas_dec_hi(enc[9 + k]);
    }
    if (moments) std::memcpy(res.sum, h + GSR_MEAS_R_SUMS, sizeof res.sum);
    *out = res;
    if (hist_words) std::memcpy(hist_out, h + GSR_MEAS_R_HIST, hist_words * 4);
    float ms = 0.0f;
    c->meas.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->meas.ms[1] = hipEventElapsedTime(&ms, c->up_ev[1], c->up_ev[2]) == hipSuccess ? (double)ms : 0.0;
    c->meas.ms[2] = copy_ms;
    c->meas.ms[3] = up_now_ms() - t_begin;
    c->meas.calls += 1;
    c->meas.last = res.n_measured;
    return GSR_OK;
}
