// GSplatRenderer.cpp -- HDK-free host side of the drop-in boundary (include/GSplatRenderer.h).
//
// The class keeps the reference's name and its nine verbs, because they are what GR_PrimGsplat and the
// scene render hook call (/root/reference/gsplat_plugin/src/GR_GSplat.C:423-436,472-492,
// src/DM_GSplatHook.C:30-39); everything behind the verbs is this build's own design, written from the
// behaviour that tests/test_host_shim.py pins:
//   * a table of registered primitives keyed by "<detail>__<vertex offset>__<cache version>";
//   * per redraw, a STAGING PLAN -- which table rows are shown, how many splats of each fit the
//     2^23-1 budget, whether the pass carries SH, the common origin -- computed from scratch and
//     compared with the plan that is resident on the GPU: the device copy is rebuilt only when the
//     two differ (or the last rebuild failed);
//   * the camera position as the point the view matrix maps to the eye, found by a linear solve;
//   * libgsplat_hip (one GPU: gsr_*, several: gsr_multi_*) for everything per splat and per pixel.
// Reference behaviour matched (not its code): src/GSplatRenderer.C:141-153 (re-stage only when the
// shown set changes), :218-320 (registry, version purge), :336-376 (budget), :403-418 (origin),
// :551-563 (camera position), :565-577 (OBJ-level notice), :660-678 (per-entry frame counters).
#include "../../include/GSplatRenderer.h"

#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

namespace {

void note(const char* severity, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "gsplat-hip %s: ", severity);
    std::vfprintf(stderr, fmt, ap);
    std::fputc('\n', stderr);
    va_end(ap);
}

// The eye in world space = the point p with V p = (0,0,0,1)^T, V given as GL column-major floats.  One
// 4x4 solve with partial pivoting in double; false when V is singular.
bool eye_of_view(const float* v, float eye[3])
{
    double a[4][5];
    for (int r = 0; r < 4; ++r) {
        for (int c = 0; c < 4; ++c) a[r][c] = v[c * 4 + r];
        a[r][4] = (r == 3) ? 1.0 : 0.0;
    }
    for (int k = 0; k < 4; ++k) {
        int best = k;
        for (int r = k + 1; r < 4; ++r)
            if (std::fabs(a[r][k]) > std::fabs(a[best][k])) best = r;
        if (a[best][k] == 0.0) return false;
        if (best != k)
            for (int c = k; c < 5; ++c) std::swap(a[best][c], a[k][c]);
        for (int r = k + 1; r < 4; ++r) {
            const double m = a[r][k] / a[k][k];
            if (m != 0.0)
                for (int c = k; c < 5; ++c) a[r][c] -= m * a[k][c];
        }
    }
    double p[4];
    for (int r = 3; r >= 0; --r) {
        double s = a[r][4];
        for (int c = r + 1; c < 4; ++c) s -= a[r][c] * p[c];
        p[r] = s / a[r][r];
    }
    if (p[3] == 0.0) return false;
    for (int k = 0; k < 3; ++k) eye[k] = static_cast<float>(p[k] / p[3]);
    return true;
}

std::string make_id(const void* detail, int64_t vtx, const GSplatCacheVersion& ver)
{
    char buf[160];
    std::snprintf(buf, sizeof(buf), "%#" PRIxPTR "__%" PRId64 "__%" PRId64 "_%" PRId64 "_%" PRId64 "_%" PRId64,
                  reinterpret_cast<uintptr_t>(detail), vtx, ver.e[0], ver.e[1], ver.e[2], ver.e[3]);
    return std::string(buf);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
GSplatRenderer& GSplatRenderer::getInstance()
{
    static GSplatRenderer the_one(0);
    return the_one;
}

GSplatRenderer::GSplatRenderer(int device)
{
    if (device < 0) { dry_ = true; return; }
    status_ = gsr_create(device, &engine_);
    if (status_ != GSR_OK) {
        note("error", "no GPU engine: %s", gsr_last_error());
        engine_ = nullptr;
    }
}

GSplatRenderer::GSplatRenderer(const int* devices, int count, int transport)
{
    if (!devices || count < 1) { dry_ = true; return; }
    if (count == 1) {
        status_ = gsr_create(devices[0], &engine_);
        if (status_ != GSR_OK) { note("error", "no GPU engine: %s", gsr_last_error()); engine_ = nullptr; }
        return;
    }
    status_ = gsr_multi_create(devices, count, transport, &multi_);
    if (status_ != GSR_OK) {
        note("error", "no multi-GPU engine: %s", gsr_last_error());
        multi_ = nullptr;
    }
}

GSplatRenderer::~GSplatRenderer()
{
    if (engine_) gsr_destroy(engine_);
    if (multi_) gsr_multi_destroy(multi_);
}

unsigned int GSplatRenderer::closestSqrtPowerOf2(int n)
{
    // side of the smallest power-of-two square texture holding n texels (kept as a known-answer target)
    unsigned int side = 2;
    while (static_cast<uint64_t>(side) * side < static_cast<uint64_t>(n > 0 ? n : 0)) side <<= 1;
    return side;
}

std::string GSplatRenderer::registerUpdate(const void* gdp, const GSplatCacheVersion& gversion, int64_t gVtxOffset,
                                           int64_t splatCount, const float splatOrigin[3], const float* splatPts,
                                           const uint16_t* splatColors, const float* splatAlphas,
                                           const uint16_t* splatScales, const uint16_t* splatOrients,
                                           const uint16_t* splatShxs, const uint16_t* splatShys,
                                           const uint16_t* splatShzs, int64_t shCount)
{
    if (!greeted_) { note("info", "%s", gsr_version()); greeted_ = true; }
    // a new cache version of a detail retires every row that still describes an older one
    for (auto it = table_.begin(); it != table_.end();)
        it = (it->second.detail == gdp && it->second.version != gversion) ? table_.erase(it) : std::next(it);
    const std::string id = make_id(gdp, gVtxOffset, gversion);
    Row row;
    row.detail = gdp;
    row.version = gversion;
    row.count = splatCount < 0 ? 0 : splatCount;
    if (splatOrigin) std::copy(splatOrigin, splatOrigin + 3, row.origin);
    row.P = splatPts; row.Cd = splatColors; row.alpha = splatAlphas; row.scale = splatScales; row.orient = splatOrients;
    const bool sh = splatShxs && splatShys && splatShzs && shCount > 0;
    row.shx = sh ? splatShxs : nullptr; row.shy = sh ? splatShys : nullptr; row.shz = sh ? splatShzs : nullptr;
    row.sh_count = sh ? shCount : 0;
    table_[id] = row;   // (shown = false, frame counters reset)
    return id;
}

void GSplatRenderer::flushEntriesForMatchingDetail(const std::string& id)
{
    const auto hit = table_.find(id);
    if (hit == table_.end()) return;
    const void* detail = hit->second.detail;
    for (auto it = table_.begin(); it != table_.end();) {
        if (it->second.detail != detail) { ++it; continue; }
        // its arrays are about to be freed by the caller: a later registration under the same id must be re-staged
        for (const Plan::Part& part : resident_.parts)
            if (part.id == it->first) resident_ok_ = false;
        it = table_.erase(it);
    }
}

int GSplatRenderer::updateAttributes(const std::string& id, const uint16_t* splatColors, const float* splatAlphas,
                                     const uint16_t* splatScales, const uint16_t* splatOrients, const uint16_t* splatShxs,
                                     const uint16_t* splatShys, const uint16_t* splatShzs, int64_t* first_out, int64_t* n_out)
{
    return editRow(id, nullptr, nullptr, splatColors, splatAlphas, splatScales, splatOrients, splatShxs, splatShys, splatShzs, first_out, n_out);
}

int GSplatRenderer::moveSplats(const std::string& id, const float* splatPts, const float* splatOrigin, const uint16_t* splatColors,
                               const float* splatAlphas, const uint16_t* splatScales, const uint16_t* splatOrients,
                               const uint16_t* splatShxs, const uint16_t* splatShys, const uint16_t* splatShzs, int64_t* first_out,
                               int64_t* n_out)
{
    if (!splatPts) {
        if (first_out) *first_out = 0;
        if (n_out) *n_out = 0;
        return GSR_E_INVALID;
    }
    return editRow(id, splatPts, splatOrigin, splatColors, splatAlphas, splatScales, splatOrients, splatShxs, splatShys, splatShzs, first_out, n_out);
}

// updateAttributes (splatPts == NULL) and moveSplats: one row's new arrays, and its resident splats edited without a re-stage
int GSplatRenderer::editRow(const std::string& id, const float* splatPts, const float* splatOrigin, const uint16_t* splatColors,
                            const float* splatAlphas, const uint16_t* splatScales, const uint16_t* splatOrients,
                            const uint16_t* splatShxs, const uint16_t* splatShys, const uint16_t* splatShzs, int64_t* first_out,
                            int64_t* n_out)
{
    if (first_out) *first_out = 0;
    if (n_out) *n_out = 0;
    const auto hit = table_.find(id);
    if (hit == table_.end()) return GSR_E_INVALID;
    Row& row = hit->second;
    // where the row sits in what is resident: the splats taken from the parts before it, and how many were taken from it
    int64_t first = 0, take = -1;
    if (resident_ok_)
        for (const Plan::Part& part : resident_.parts) {
            if (part.id == id) { take = part.take; break; }
            first += part.take;
        }
    const int nsh = (splatShxs ? 1 : 0) + (splatShys ? 1 : 0) + (splatShzs ? 1 : 0);
    if (nsh != 0 && (nsh != 3 || row.sh_count < (take >= 0 ? take : row.count))) return GSR_E_INVALID;
    // registerUpdate() may have retired another resident row since the plan was recorded: what is resident is then due for a
    // re-stage, which takes this row as it is now -- nothing is moved on the GPU, and no origin is formed over rows that are gone
    if (splatPts && take >= 0)
        for (const Plan::Part& part : resident_.parts)
            if (table_.find(part.id) == table_.end()) { resident_ok_ = false; take = -1; break; }
    if (splatPts) row.P = splatPts;
    if (splatPts && splatOrigin) {
        std::copy(splatOrigin, splatOrigin + 3, row.origin);
        if (take >= 0) planOrigin(resident_);   // the resident pass's origin, by the rule a re-stage forms it with
    }
    if (splatColors) row.Cd = splatColors;
    if (splatAlphas) row.alpha = splatAlphas;
    if (splatScales) row.scale = splatScales;
    if (splatOrients) row.orient = splatOrients;
    if (nsh) { row.shx = splatShxs; row.shy = splatShys; row.shz = splatShzs; }
    if (take < 0) return 0;
    if (first_out) *first_out = first;
    if (n_out) *n_out = take;
    if (dry_) return 1;
    gsr_attr_update u{};
    u.Cd = splatColors; u.alpha = splatAlphas; u.scale = splatScales; u.orient = splatOrients;
    if (nsh && resident_.sh) { u.shx = splatShxs; u.shy = splatShys; u.shz = splatShzs; }
    if (splatPts) {
        const float* const org = splatOrigin ? resident_.origin : nullptr;
        status_ = multi_ ? gsr_multi_move(multi_, first, take, splatPts, org, &u) : engine_ ? gsr_move(engine_, first, take, splatPts, org, &u) : GSR_E_NO_DEVICE;
    } else {
        status_ = multi_ ? gsr_multi_update(multi_, first, take, &u) : engine_ ? gsr_update(engine_, first, take, &u) : GSR_E_NO_DEVICE;
    }
    if (status_ != GSR_OK) {
        note("error", "%s %" PRId64 " splats in place failed: %s", splatPts ? "moving" : "updating", take, gsr_last_error());
        resident_ok_ = false;   // the next redraw stages the edited arrays
        return status_;
    }
    return 1;
}

const void* GSplatRenderer::rowArray(const std::string& id, int what) const
{
    const auto hit = table_.find(id);
    if (hit == table_.end()) return nullptr;
    const Row& r = hit->second;
    const void* const a[8] = {r.P, r.Cd, r.alpha, r.scale, r.orient, r.shx, r.shy, r.shz};
    return what >= 0 && what < 8 ? a[what] : nullptr;
}

void GSplatRenderer::includeInRenderPass(const std::string& id)
{
    const auto hit = table_.find(id);
    if (hit != table_.end()) hit->second.shown = true;
}

// What this redraw would put on the GPU.  Rows are visited in id order; a row joins while the budget is not
// yet used up, and the row that crosses the budget is truncated.
// The origin of a pass: the mean of its rows' origins, summed in packing order (src/GSplatRenderer.C:403-418).  The ONE place the
// rule lives: planFrame() and moveSplats() must give the same plan the same bits.
void GSplatRenderer::planOrigin(Plan& p) const
{
    if (p.parts.empty()) return;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (const Plan::Part& part : p.parts)
        for (int k = 0; k < 3; ++k) sum[k] += table_.at(part.id).origin[k];
    for (int k = 0; k < 3; ++k) p.origin[k] = sum[k] / static_cast<float>(p.parts.size());
}

GSplatRenderer::Plan GSplatRenderer::planFrame() const
{
    const int64_t budget = GSPLAT_COUNT_MAX - 1;
    Plan p;
    for (const auto& kv : table_) {
        const Row& r = kv.second;
        p.registered += r.count;
        if (!r.shown || r.count <= 0 || p.total >= budget) continue;
        const int64_t take = std::min(r.count, budget - p.total);
        p.parts.push_back({kv.first, take});
        p.total += take;
        p.wanted += r.count;
        p.sh = r.sh_count > 0;   // the row joined last decides
    }
    planOrigin(p);
    return p;
}

bool GSplatRenderer::upload(const Plan& p)
{
    const bool multi = multi_ != nullptr;
    status_ = multi ? gsr_multi_upload_begin(multi_, p.total, p.sh ? 1 : 0, p.origin)
                    : gsr_upload_begin(engine_, p.total, p.sh ? 1 : 0, p.origin);
    std::vector<uint16_t> no_sh;   // a row without SH inside an SH pass contributes zero coefficients
    for (size_t k = 0; k < p.parts.size() && status_ == GSR_OK; ++k) {
        const Row& r = table_.at(p.parts[k].id);
        const int64_t n = p.parts[k].take;
        const uint16_t *x = nullptr, *y = nullptr, *z = nullptr;
        if (p.sh) {
            if (r.sh_count >= n) { x = r.shx; y = r.shy; z = r.shz; }
            else { no_sh.assign(static_cast<size_t>(n) * 16, 0); x = y = z = no_sh.data(); }
        }
        status_ = multi ? gsr_multi_upload_append(multi_, n, r.P, r.Cd, r.alpha, r.scale, r.orient, x, y, z)
                        : gsr_upload_append(engine_, n, r.P, r.Cd, r.alpha, r.scale, r.orient, x, y, z);
    }
    if (status_ == GSR_OK) status_ = multi ? gsr_multi_upload_end(multi_) : gsr_upload_end(engine_);
    if (status_ != GSR_OK) {
        note("error", "staging %" PRId64 " splats failed: %s", p.total, gsr_last_error());
        if (multi) gsr_multi_upload_abort(multi_); else gsr_upload_abort(engine_);
        return false;
    }
    return true;
}

void GSplatRenderer::generateRenderGeometry(GSplatRenderContext& /*r*/)
{
    Plan now = planFrame();
    if (now.parts.empty()) return;   // nothing to show this redraw: whatever is resident stays resident
    if (resident_ok_ && now.sameAs(resident_)) return;

    if (now.wanted > now.total)
        note("warning", "%" PRId64 " splats requested but one pass holds %" PRId64 ": the last %" PRId64 " are left out",
             now.wanted, now.total, now.wanted - now.total);
    ++stagings_;
    resident_ = now;
    resident_ok_ = true;
    can_render_ = true;
    if (dry_) return;
    if ((!engine_ && !multi_) || !upload(now)) {
        // keep no record of a failed upload: the next redraw plans the same frame, finds nothing resident, retries
        resident_ = Plan();
        resident_ok_ = false;
        can_render_ = false;
    }
}

void GSplatRenderer::render(GSplatRenderContext& r, bool isObjectLevel)
{
    if (!enabled_ || !can_render_) return;
    if (std::none_of(table_.begin(), table_.end(), [](const std::pair<const std::string, Row>& kv) { return kv.second.shown; }))
        return;

    if (eye_override_) std::copy(eye_explicit_, eye_explicit_ + 3, eye_);
    else if (!eye_of_view(r.view, eye_)) return;

    if (isObjectLevel && !obj_notice_given_)
        note("warning", "object-level redraw, eye at (%g, %g, %g): object transforms other than identity are drawn as identity",
             eye_[0], eye_[1], eye_[2]);
    obj_notice_given_ = isObjectLevel;

    if (dry_) { ++frames_; return; }
    if ((!engine_ && !multi_) || !r.target) return;

    gsr_camera cam;
    std::memcpy(cam.obj_view, r.obj_view, sizeof(cam.obj_view));
    std::memcpy(cam.object, r.object, sizeof(cam.object));
    std::memcpy(cam.inv_object, r.inv_object, sizeof(cam.inv_object));
    std::memcpy(cam.view, r.view, sizeof(cam.view));
    std::memcpy(cam.proj, r.proj, sizeof(cam.proj));
    std::copy(eye_, eye_ + 3, cam.cam_pos);
    cam.width = r.width;
    cam.height = r.height;
    cam.sh_order = (sh_order_ > 0 && resident_.sh) ? sh_order_ : 0;   // SH needs an order AND data
    status_ = multi_ ? gsr_multi_render_depth(multi_, &cam, r.depth, r.depth_is_device, r.target, r.target_is_device)
                     : bg_.kind != 0 ? gsr_render_over(engine_, &cam, r.depth, r.depth_is_device, &bg_, r.target, r.target_is_device)
                     : gsr_render_aov(engine_, &cam, r.depth, r.depth_is_device, r.target, r.target_is_device, aov_, aov_plane_);
    if (status_ != GSR_OK) { note("error", "frame failed: %s", gsr_last_error()); return; }
    ++frames_;
}

void GSplatRenderer::postRender()
{
    for (auto& kv : table_) {
        Row& r = kv.second;
        if (r.shown) r.redraws_since_shown = 0;
        else if (r.redraws_since_shown >= 0) ++r.redraws_since_shown;
        r.shown = false;
        ++r.redraws;
    }
    eye_override_ = false;
}

void GSplatRenderer::setRenderingEnabled(bool on) { enabled_ = on; }

void GSplatRenderer::setExplicitCameraPos(const float p[3])
{
    std::copy(p, p + 3, eye_explicit_);
    eye_override_ = true;
}

void GSplatRenderer::setSphericalHarmonicsOrder(int order) { sh_order_ = order; }

int GSplatRenderer::setTargetFormat(int format)
{
    if (gsr_target_pixel_bytes(format) < 0) return GSR_E_INVALID;
    int rc = GSR_OK;
    if (multi_) rc = gsr_multi_set_target_format(multi_, format);
    else if (engine_) rc = gsr_set_target_format(engine_, format);
    if (rc == GSR_OK) target_format_ = format;
    return rc;
}

int GSplatRenderer::setAovTarget(int aov, float* plane)
{
    if ((aov != 0 && aov != GSR_AOV_DEPTH) || (multi_ && aov != 0 && plane)) return GSR_E_INVALID;
    if (aov != 0 && plane && bg_.kind != 0) return GSR_E_INVALID;   // (no AOV + background verb)
    aov_ = plane ? aov : 0;
    aov_plane_ = aov_ ? plane : nullptr;
    return GSR_OK;
}

int GSplatRenderer::setBackground(const gsr_background* bg)
{
    if (!bg || bg->kind == 0) { bg_ = gsr_background{}; return GSR_OK; }
    if (bg->kind != GSR_BG_COLOUR && bg->kind != GSR_BG_IMAGE) return GSR_E_INVALID;
    if (bg->kind == GSR_BG_IMAGE && (gsr_target_pixel_bytes(bg->format) < 0 || !bg->image)) return GSR_E_INVALID;
    if (multi_ || aov_ != 0) return GSR_E_INVALID;
    bg_ = *bg;
    return GSR_OK;
}

int GSplatRenderer::setVisibility(const gsr_visibility* v)
{
    if (v && v->mask) return GSR_E_INVALID;            // (a mask belongs to one upload: the next re-stage would lose it)
    // the struct is checked by the one function that knows the rule: an evaluation over no splats
    if (gsr_visibility_eval(v, nullptr, 0, 0, nullptr) != GSR_OK) return GSR_E_INVALID;
    int rc = GSR_OK;
    if (multi_) rc = gsr_multi_set_visibility(multi_, v);
    else if (engine_) rc = gsr_set_visibility(engine_, v);
    status_ = rc;
    return rc;
}

int64_t GSplatRenderer::query(int what, const std::string& id) const
{
    switch (what) {
    case Q_REGISTRY_SIZE: return static_cast<int64_t>(table_.size());
    case Q_ACTIVE_STAGED: return static_cast<int64_t>(resident_.parts.size());
    case Q_SPLAT_COUNT: return resident_.total;
    case Q_CAN_RENDER: return can_render_ ? 1 : 0;
    case Q_STAGING_COUNT: return stagings_;
    case Q_RENDER_COUNT: return frames_;
    case Q_SH_PRESENT: return resident_.sh ? 1 : 0;
    case Q_LAST_STATUS: return status_;
    case Q_ENTRY_AGE:
    case Q_ENTRY_AGE_SINCE_ACTIVE: {
        const auto hit = table_.find(id);
        if (hit == table_.end()) return -1000;
        return what == Q_ENTRY_AGE ? hit->second.redraws : hit->second.redraws_since_shown;
    }
    default: return -1;
    }
}

void GSplatRenderer::origin(float out[3]) const { std::copy(resident_.origin, resident_.origin + 3, out); }
void GSplatRenderer::lastCameraPos(float out[3]) const { std::copy(eye_, eye_ + 3, out); }

// ---------------------------------------------------------------------------------------------
// flat C wrappers
struct gsplat_renderer {
    GSplatRenderer* impl;
    bool owned;
};

extern "C" {

gsplat_renderer* gsplat_renderer_create(int device)
{
    GSplatRenderer* p = new (std::nothrow) GSplatRenderer(device);
    if (!p) return nullptr;
    if (device >= 0 && !p->engine()) { delete p; return nullptr; }
    gsplat_renderer* h = new (std::nothrow) gsplat_renderer{p, true};
    if (!h) delete p;
    return h;
}

gsplat_renderer* gsplat_renderer_create_multi(const int* devices, int count, int transport)
{
    GSplatRenderer* p = new (std::nothrow) GSplatRenderer(devices, count, transport);
    if (!p) return nullptr;
    if (!p->engine() && !p->multi()) { delete p; return nullptr; }
    gsplat_renderer* h = new (std::nothrow) gsplat_renderer{p, true};
    if (!h) delete p;
    return h;
}

gsplat_renderer* gsplat_renderer_get_instance(void)
{
    static gsplat_renderer single{&GSplatRenderer::getInstance(), false};
    return &single;
}

void gsplat_renderer_destroy(gsplat_renderer* h)
{
    if (!h || !h->owned) return;
    delete h->impl;
    delete h;
}

int gsplat_renderer_register_update(gsplat_renderer* h, uint64_t gdp, const int64_t gversion[4], int64_t gvtx_offset,
                                    int64_t splat_count, const float origin[3], const float* P, const uint16_t* Cd,
                                    const float* alpha, const uint16_t* scale, const uint16_t* orient,
                                    const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, int64_t sh_count,
                                    char* id_out, int id_cap)
{
    if (!h || !gversion) return -1;
    GSplatCacheVersion v;
    for (int k = 0; k < 4; ++k) v.e[k] = gversion[k];
    const std::string id = h->impl->registerUpdate(reinterpret_cast<const void*>(static_cast<uintptr_t>(gdp)), v,
                                                   gvtx_offset, splat_count, origin, P, Cd, alpha, scale, orient, shx,
                                                   shy, shz, sh_count);
    if (id_out && id_cap > 0) {
        std::strncpy(id_out, id.c_str(), static_cast<size_t>(id_cap) - 1);
        id_out[id_cap - 1] = '\0';
    }
    return static_cast<int>(id.size());
}

void gsplat_renderer_include_in_render_pass(gsplat_renderer* h, const char* id) { if (h && id) h->impl->includeInRenderPass(id); }
void gsplat_renderer_flush_entries_for_matching_detail(gsplat_renderer* h, const char* id) { if (h && id) h->impl->flushEntriesForMatchingDetail(id); }
void gsplat_renderer_generate_render_geometry(gsplat_renderer* h, GSplatRenderContext* r) { if (h && r) h->impl->generateRenderGeometry(*r); }
void gsplat_renderer_render(gsplat_renderer* h, GSplatRenderContext* r, int is_object_level) { if (h && r) h->impl->render(*r, is_object_level != 0); }
void gsplat_renderer_post_render(gsplat_renderer* h) { if (h) h->impl->postRender(); }
void gsplat_renderer_redraw(gsplat_renderer* h, const char* const* ids, int n, GSplatRenderContext* r, int is_object_level)
{
    if (!h || !r) return;
    for (int k = 0; k < n; ++k)
        if (ids && ids[k]) h->impl->includeInRenderPass(ids[k]);
    h->impl->generateRenderGeometry(*r);
    h->impl->render(*r, is_object_level != 0);
    h->impl->postRender();
}
void gsplat_renderer_set_rendering_enabled(gsplat_renderer* h, int enabled) { if (h) h->impl->setRenderingEnabled(enabled != 0); }
void gsplat_renderer_set_explicit_camera_pos(gsplat_renderer* h, const float pos[3]) { if (h && pos) h->impl->setExplicitCameraPos(pos); }
void gsplat_renderer_set_spherical_harmonics_order(gsplat_renderer* h, int order) { if (h) h->impl->setSphericalHarmonicsOrder(order); }
int gsplat_renderer_set_target_format(gsplat_renderer* h, int format) { return h ? h->impl->setTargetFormat(format) : GSR_E_INVALID; }
int gsplat_renderer_set_aov_target(gsplat_renderer* h, int aov, float* plane) { return h ? h->impl->setAovTarget(aov, plane) : GSR_E_INVALID; }
int gsplat_renderer_set_background(gsplat_renderer* h, const gsr_background* bg) { return h ? h->impl->setBackground(bg) : GSR_E_INVALID; }
int gsplat_renderer_set_visibility(gsplat_renderer* h, const gsr_visibility* v) { return h ? h->impl->setVisibility(v) : GSR_E_INVALID; }
int gsplat_renderer_update_attributes(gsplat_renderer* h, const char* id, const uint16_t* Cd, const float* alpha, const uint16_t* scale,
                                      const uint16_t* orient, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz,
                                      int64_t* first_out, int64_t* n_out)
{
    return h && id ? h->impl->updateAttributes(id, Cd, alpha, scale, orient, shx, shy, shz, first_out, n_out) : GSR_E_INVALID;
}
int gsplat_renderer_move_splats(gsplat_renderer* h, const char* id, const float* P, const float* origin, const uint16_t* Cd, const float* alpha,
                                const uint16_t* scale, const uint16_t* orient, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz,
                                int64_t* first_out, int64_t* n_out)
{
    return h && id ? h->impl->moveSplats(id, P, origin, Cd, alpha, scale, orient, shx, shy, shz, first_out, n_out) : GSR_E_INVALID;
}
const void* gsplat_renderer_row_array(gsplat_renderer* h, const char* id, int what) { return h && id ? h->impl->rowArray(id, what) : nullptr; }
int gsplat_renderer_get_target_format(gsplat_renderer* h) { return h ? h->impl->targetFormat() : GSR_E_INVALID; }
int64_t gsplat_renderer_query(gsplat_renderer* h, int what, const char* id) { return h ? h->impl->query(what, id ? std::string(id) : std::string()) : -1; }
void gsplat_renderer_get_origin(gsplat_renderer* h, float out[3]) { if (h && out) h->impl->origin(out); }
void gsplat_renderer_get_last_camera_pos(gsplat_renderer* h, float out[3]) { if (h && out) h->impl->lastCameraPos(out); }
gsr_context* gsplat_renderer_engine(gsplat_renderer* h) { return h ? h->impl->engine() : nullptr; }
gsr_multi* gsplat_renderer_multi(gsplat_renderer* h) { return h ? h->impl->multi() : nullptr; }
unsigned int gsplat_closest_sqrt_power_of_2(int n) { return GSplatRenderer::closestSqrtPowerOf2(n); }
GSplatRenderer* gsplat_renderer_impl(gsplat_renderer* h) { return h ? h->impl : nullptr; }

}  // extern "C"
