// gsr_resident_edit.h -- the verbs that edit the resident cloud without a re-upload: gsr_update, gsr_move, the
// device sources, gsr_set_visibility, gsr_remove, gsr_add, gsr_duplicate, gsr_transform, gsr_grade.  Host code only; included once, at the end of gsr_api.hip, which has the
// context, the frame slots, the upload arena (ensure_stage, ensure_up_events, stage_host_rows), the ordering of an upload (position_box,
// morton_order), new_cloud_state / drop_geometry, and the <SH> launches of k_update, k_update_f32 and k_repack (launch_update,
// queue_repack).
//
// Every edit promises "bit for bit a fresh upload of the result" and "a failure before the first write leaves the context as it was".
// Move, remove and add keep both through ONE pipeline (Reorder): prepare -- everything the new storage order needs, before the first
// write; order -- the ordering of an upload over every position of the new cloud; commit / finish -- the swap of the spare planes, the
// counts, the visibility rule over the whole cloud, a new generation.  What a call allocated and did not hand over goes with its
// Reorder (handles, gsr_host_buffers.h): a failure before the first write is a plain return (the context as it was), one after it
// goes through Reorder::lost (no geometry, as a failed gsr_upload_end leaves it).
#pragma once

// ---------------------------------------------------------------------------
// What every verb of the family refuses first (GSR_E_INVALID, the context untouched).  The order in which a verb looks at its own
// arguments around these two is the verb's: it decides which message a doubly wrong call gets.
static int refuse_edit(const gsr_context* c, const char* who, bool need_geometry = true)
{
    if (!c) return set_err(GSR_E_INVALID, "%s: ctx is NULL", who);
    if (c->uploading) return set_err(GSR_E_INVALID, "%s: upload in progress", who);
    if (need_geometry && !c->has_geometry) return set_err(GSR_E_INVALID, "%s: no geometry: nothing uploaded", who);
    return GSR_OK;
}
static int refuse_range(const gsr_context* c, int64_t first, int64_t n, const char* who)
{
    if (first < 0 || n < 0 || first > (int64_t)c->n || n > (int64_t)c->n - first)
        return set_err(GSR_E_INVALID, "%s: splats [%lld, %lld + %lld) are not within the %u resident", who, (long long)first, (long long)first, (long long)n, c->n);
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// What the resident cloud's frames may keep after an attribute update (the invalidation table).  The cached depth orders go
// in every case: their records hold the colours.  Colours change neither visibility, order nor opacity: horizons, prefixes, hints and
// policies survive a Cd / SH update; anything else (`shape`: alpha, scale or orient changed) is treated like a new cloud at the same
// positions.  e: the state of the call so far; the first failure is what comes back.
static hipError_t after_update(gsr_context* c, bool shape, hipStream_t us, hipError_t e)
{
    for (int k = 0; k < GSR_MAX_SLOTS; ++k) c->slot[k].sort_valid = false;
    return shape ? forget_frame_learning(c, us, e) : e;
}

// The launch of an attribute update and what follows it, shared by the host and the device form.  On `us`, between up_ev[0] and
// up_ev[1]: k_update / k_update_f32 over rows [first, first + n), the cluster extents when scale or orient changed, the visibility
// hook when alpha did; then the invalidation, and the update's two clock entries (link_ms: what the staging took).  vis_rule: see update_rows.
template <class Src>
static int queue_update(gsr_context* c, const char* who, hipStream_t us, uint32_t first, uint32_t n, const Src& src, bool alpha, bool extents, bool vis_rule, double link_ms)
{
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    hipError_t e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        launch_update(c, us, first, n, src, inv);
        // (the bounds of ALL clusters: a Morton-ordered store scatters the range over them, and the pass reads 32 bytes per splat)
        if (extents) hipLaunchKernelGGL(k_cluster_extents, dim3(div_up(c->nclus, 4)), dim3(256), 0, us, c->n, c->nclus, c->geoA, c->geoB, c->clusA, c->clusB);
        e = hipGetLastError();
        // a visibility in force: the new alphas are put aside, and the hidden ones among them go back to +0.0f (a move does that itself)
        if (e == hipSuccess && c->vis_on && alpha) e = vis_apply(c, us, first, n, vis_rule, c->vis, c->vis_mask, nullptr);
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);   // (a device source: the caller's arrays may be overwritten on return)
    e = after_update(c, alpha || extents, us, e);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    float ms = 0.0f;
    c->st.upload_ms[4] = link_ms;
    if (hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess) c->st.upload_ms[5] = ms;
    return GSR_OK;
}

// Where gsr_update stages the given arrays of u, rows [0, n), in the arena: alpha, Cd, scale, orient, shx, shy, shz in 256-byte aligned
// sections (none for an array not given), and the bytes in all.  gsr_move sizes the arena by it, before its first write.
struct UpdateStage {
    const void* given[7];
    size_t row[7], at[7], bytes;
};
static UpdateStage update_stage(const gsr_attr_update* u, size_t n)
{
    UpdateStage s{{u->alpha, u->Cd, u->scale, u->orient, u->shx, u->shy, u->shz}, {4, 6, 6, 8, 32, 32, 32}, {}, 0};
    for (int k = 0; k < 7; ++k) { s.at[k] = s.bytes; if (s.given[k]) s.bytes += pad256(n * s.row[k]); }
    return s;
}

// ---------------------------------------------------------------------------
// Attributes of resident splats rewritten in place ("Attribute updates").  No position: the storage order, the bounding
// box, the Morton scratch and the cluster boxes' xyz depend on P alone and stay as they are.
// vis_rule: with a visibility in force and new alphas, put them aside AND apply the rule (gsr_update); false: put them aside only (the
// attribute step of a move, which applies the rule itself once the splats sit at their new positions, in the new order)
static int update_rows(gsr_context* c, int64_t first, int64_t n64, const gsr_attr_update* u, bool vis_rule)
{
    const char* const who = "gsr_update";
    if (!c || !u) return set_err(GSR_E_INVALID, "gsr_update: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    const int nsh = (u->shx ? 1 : 0) + (u->shy ? 1 : 0) + (u->shz ? 1 : 0);
    if (nsh != 0 && nsh != 3) return set_err(GSR_E_INVALID, "gsr_update: the three SH arrays come together or not at all");
    if (nsh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_update: SH arrays for a cloud uploaded without SH");
    if (n64 == 0 || !(u->Cd || u->alpha || u->scale || u->orient || nsh)) return GSR_OK;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = sync_all(c))) return rc;      // no in-place write under a frame in flight (two frames in flight, deferred-check frames included)
    const uint32_t n = (uint32_t)n64;
    hipStream_t us = c->slot[0].own;
    const UpdateStage s = update_stage(u, n);
    if ((rc = ensure_stage(c, s.bytes)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    const double t0 = up_now_ms();
    const void* d[7];                  // the given arrays in the arena (NULL: not given)
    hipError_t e = hipSuccess;
    for (int k = 0; k < 7; ++k) {
        d[k] = s.given[k] ? c->stage + s.at[k] : nullptr;
        if (s.given[k] && e == hipSuccess) e = hipMemcpyAsync(c->stage + s.at[k], s.given[k], (size_t)n * s.row[k], hipMemcpyHostToDevice, us);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(us);   // the caller's arrays may be freed on return
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_update: %s", hipGetErrorString(e));
    const double link_ms = up_now_ms() - t0;
    auto h16 = [&](int k) { return static_cast<const uint16_t*>(d[k]); };
    const GsrUpdateSrc src{static_cast<const float*>(d[0]), h16(1), h16(2), h16(3), h16(4), h16(5), h16(6)};
    return queue_update(c, who, us, (uint32_t)first, n, src, u->alpha != nullptr, u->scale || u->orient, vis_rule, link_ms);
}

extern "C" int gsr_update(gsr_context* c, int64_t first, int64_t n64, const gsr_attr_update* u)
{
    return update_rows(c, first, n64, u, true);
}

// ---------------------------------------------------------------------------
// The SPARE copy of the planes (at the capacity `cap`: c->cap for a move, a removal and an add that fits; the new capacity for an add
// that grows, which has released the old set first) and, with `bounds`, of the cluster bounds (at the cluster count in force: a
// removal only ever needs fewer, and an add brings its own).  Allocated at the first call that writes a new storage order, kept until
// the geometry is freed or an add grows the capacity.  A failure leaves no half of a set behind.
static int ensure_spare_planes(gsr_context* c, size_t cap, bool bounds)
{
    int rc = GSR_OK;
    if (!c->geoA2 && ((rc = c->geoA2.alloc(cap)) || (rc = c->geoB2.alloc(cap)) || (rc = c->col2.alloc(cap * c->col_chunks)) ||
                      (c->has_sh && (rc = c->colrow2.alloc(cap * 8))))) {
        free_spare_planes(c);
        return rc;
    }
    if (bounds && !c->clusA2 && ((rc = c->clusA2.alloc(c->nclus)) || (rc = c->clusB2.alloc(c->nclus)))) {
        c->clusA2.reset();
        return rc;
    }
    return GSR_OK;
}

// The spare set becomes the resident one, under the storage order perm_new (taken over; empty: upload order).  Nothing is in flight, and
// every frame takes the planes from the context.
static void swap_planes(gsr_context* c, DevMem<uint32_t>& perm_new)
{
    c->geoA.swap(c->geoA2); c->geoB.swap(c->geoB2); c->col.swap(c->col2); c->colrow.swap(c->colrow2);
    c->clusA.swap(c->clusA2); c->clusB.swap(c->clusB2);
    c->perm = std::move(perm_new);
}

// The re-order pipeline of move, remove and add.  The verb forms every position of the NEW cloud in upload order (device memory) and
// writes the spare planes in the new order; the object runs the steps around that, and owns what is allocated for the call until the
// context takes it over: the new permutation, and what a verb brings beside it.  It keeps the verb's clock too.
struct Reorder {
    gsr_context* const c;
    const char* const who;
    const bool oom_code;               // (ensure_up_events; the wait for the inverse maps hipErrorOutOfMemory the same way)
    const hipStream_t us;              // slot 0's stream: everything the pipeline queues
    const double t_begin = up_now_ms();
    double link_ms = 0.0;              // what the verb's staging took
    const uint32_t* inv_old = nullptr; // (not owned: c->wire_inv) upload index -> slot of the OLD order (NULL: upload order), from old_inverse() on
    bool may_order = false;            // GSR_OPT_STORAGE_ORDER and more than one splat: whether the new cloud IS ordered is known only once its box is
    DevMem<uint32_t> perm_new;         // the new storage order: until the swap takes it over, or the new cloud turns out to stay in upload order
    DevMem<uint32_t> mask_new;         // remove, add: the mask of a visibility in force, at the new upload indices (commit hands it over)
    // gsr_add's: the true alphas at a grown capacity, the spare cluster bounds of the larger cloud, the slot arrays at a grown capacity
    DevMem<float> alpha0_new;
    DevMem<float4> clusA_new, clusB_new;
    SlotSplatArrays slot_new[GSR_MAX_SLOTS];
    bool spare_outgrown = false;       // gsr_add, growing: the spare planes are at the new capacity, and go when the geometry is lost

    Reorder(gsr_context* ctx, const char* verb, bool oom) : c(ctx), who(verb), oom_code(oom), us(ctx->slot[0].stream) {}

    // A failure before the first write is a plain `return rc`: the context stays as it was, and what the call allocated goes with the
    // object.  A failure after it: no geometry (as a failed gsr_upload_end leaves the context)
    int lost(int code)
    {
        if (spare_outgrown) free_spare_planes(c);      // (the planes that stay are at the old capacity)
        drop_geometry(c);
        return code;
    }
    int lost(hipError_t e) { return lost(set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e))); }

    // ---- before the first write
    // the sort of a new storage order over n_new splats: the bounding-box partials, the Morton scratch, slot 0's histogram, perm_new
    int prepare(uint32_t n_new)
    {
        FrameSlot& sl = c->slot[0];
        int rc = GSR_OK;
        if (!c->up_part && (rc = c->up_part.alloc((size_t)512 * 6))) return rc;
        may_order = c->opt_morton && n_new > 1;
        if (!may_order) return GSR_OK;
        if (c->up_sort.hold(n_new)) return set_err(GSR_E_OOM, "%s: no room for the sort of the storage order", who);
        if ((rc = ensure_counts(sl.hist, (size_t)512 * div_up(n_new, (uint32_t)RS_THREADS * (uint32_t)RS_ITEMS) + 8))) return rc;
        return perm_new.alloc((size_t)n_new);
    }
    // the OLD order's inverse (built on slot 0's own stream, and waited for) and the three events of the clock.  events_first: gsr_remove
    // and gsr_add create the events in front of the inverse, gsr_move behind it; each keeps its sequence.
    int old_inverse(bool events_first)
    {
        int rc = GSR_OK;
        if (events_first && (rc = ensure_up_events(c, 3, who, oom_code))) return rc;
        if ((rc = ensure_inverse_perm(c))) return rc;
        if (!events_first && (rc = ensure_up_events(c, 3, who, oom_code))) return rc;
        const hipError_t e = hipStreamSynchronize(c->slot[0].own);
        if (e != hipSuccess) return set_err(oom_code && e == hipErrorOutOfMemory ? GSR_E_OOM : GSR_E_HIP, "%s: the inverse of the storage order: %s", who, hipGetErrorString(e));
        inv_old = c->perm ? c->wire_inv : nullptr;
        return GSR_OK;
    }

    // ---- the ordering of an upload over P (every position of the new cloud, upload order, device memory): the box, the Morton order
    // into perm_new where the cloud is ordered (perm_new == NULL afterwards: upload order), and up_ev[1] behind it.  A failure: lost().
    int order(const float* P, uint32_t n_new)
    {
        int rc = position_box(c, P, n_new, us, who);
        if (rc) return rc;
        const bool ordered = may_order && c->bbox_ok;
        if (ordered && (rc = morton_order(c, P, n_new, perm_new, who))) return rc;
        if (!ordered) perm_new.reset();
        const hipError_t e = hipEventRecord(c->up_ev[1], us);
        return e == hipSuccess ? GSR_OK : set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }

    // ---- behind the wait for the planes: nothing is in flight, and every frame takes the planes from the context.
    // swap: the spare set becomes the resident one, under the storage order perm_new (taken over; NULL: upload order) -- false only for
    // the move that rewrote the cluster bounds in place.  Then the counts of the new cloud, and its mask.
    void commit(uint32_t n_new, uint32_t nclus_new, bool swap)
    {
        if (swap) swap_planes(c, perm_new);
        c->h_perm.clear();
        c->n = n_new; c->nclus = nclus_new; c->up_total = c->up_filled = n_new;
        c->st.n_splats = n_new;
        if (mask_new) c->vis_mask = std::move(mask_new);
    }
    // a visibility in force: the rule over the whole cloud, at the positions the splats have now, in the order they sit in now; and a new
    // cloud to everything a frame keeps; then the clock as ms[4]: the link, up_ev[0] -> [1] (the ordering), up_ev[1] -> [2] (the planes),
    // the whole call.  keep_unread: an interval whose events cannot be read keeps what the entry held (gsr_move) or reads 0 (gsr_remove,
    // gsr_add).  A failure drops the geometry.
    int finish(double ms[4], bool keep_unread)
    {
        hipError_t e = hipSuccess;
        if (c->vis_on && (e = vis_apply(c, us, 0u, 0u, true, c->vis, c->vis_mask, nullptr)) != hipSuccess)
            return lost(set_err(GSR_E_HIP, "%s: applying the visibility: %s", who, hipGetErrorString(e)));
        const int rc = new_cloud_state(c, who);        // (the policy word could not be reset: a HIP failure like any other)
        if (rc) return lost(rc);
        ms[0] = link_ms;
        for (int k = 1; k <= 2; ++k) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, c->up_ev[k - 1], c->up_ev[k]) == hipSuccess) ms[k] = t;
            else if (!keep_unread) ms[k] = 0.0;
        }
        ms[3] = up_now_ms() - t_begin;
        return GSR_OK;
    }
};

// ---------------------------------------------------------------------------
// The body of every verb that gives resident splats new positions and keeps their number: gsr_move, gsr_move_device, gsr_transform.
// stage_bytes: what the call needs of the staging arena; ms: the verb's clock (keep_unread: Reorder::finish).
//   before_write(ro, &nothing)   behind the last allocation and in front of the first write: what the verb can still find out
//                                without changing anything; nothing = true: the call is over, GSR_OK, and nothing was changed
//   positions(ro, &Pall)         the position step: the verb's own writes into the resident planes (from here on a failure leaves no
//                                geometry: the step goes through ro.lost itself), up_ev[0] in front of its kernel, and Pall = every
//                                position of the cloud in upload order, device memory, for the ordering of an upload
template <class BeforeWrite, class Positions>
static int reposition_body(gsr_context* c, const char* who, size_t stage_bytes, const float origin[3], double ms[4], bool keep_unread,
                           BeforeWrite&& before_write, Positions&& positions)
{
    HIP_TRY(hipSetDevice(c->device));
    Reorder ro(c, who, false);
    int rc = sync_all(c);      // no write under a frame in flight
    if (rc) return rc;
    const uint32_t n = c->n;
    // ---- everything the call needs, before the first write: an allocation failure leaves the context as it was
    // (whether the new cloud is ordered is known only once its box is: with GSR_OPT_STORAGE_ORDER = 1 the sort and the spare planes are provided for)
    if ((rc = ensure_stage(c, stage_bytes))) return rc;
    if ((rc = ro.prepare(n))) return rc;
    if ((ro.may_order || c->perm) && (rc = ensure_spare_planes(c, c->cap, true))) return rc;
    if ((rc = ro.old_inverse(false))) return rc;
    bool nothing = false;
    if ((rc = before_write(ro, &nothing)) || nothing) return rc;
    // ---- from here on a failure leaves no geometry
    const float* Pall = nullptr;
    if ((rc = positions(ro, &Pall))) return rc;
    // the ordering of an upload
    if ((rc = ro.order(Pall, n))) return ro.lost(rc);
    // the planes into the new order (the spare copy), or -- upload order before and after -- only the cluster bounds again, in place
    hipStream_t us = ro.us;
    hipError_t e = hipSuccess;
    const bool repack = ro.perm_new || c->perm;
    if (repack) {
        e = queue_repack(c, us, n, ro.perm_new, ro.inv_old);
    } else {
        hipLaunchKernelGGL(k_cluster_bounds, dim3(c->nclus), dim3(GSR_PACK_THREADS), 0, us, n, c->geoA, c->geoB, c->clusA, c->clusB);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return ro.lost(e);
    // the swap, and the cloud at its new positions
    ro.commit(n, c->nclus, repack);
    if (origin) for (int k = 0; k < 3; ++k) c->origin[k] = origin[k];
    return ro.finish(ms, keep_unread);
}

// The body of gsr_move and gsr_move_device, behind their refusals.  new_bytes: what the new rows take at the head of the arena (0: they
// stay in the caller's device memory); upd_bytes: what the attribute step stages there; attr_step(): the update verb for the same rows
// (attrs: whether there is one; it leaves its link time in upload_ms[4]); new_rows(arena, stream, &Pnew, &link_ms): the device pointer
// of the new rows, after whatever copy brings them there.
template <class AttrStep, class NewRows>
static int move_body(gsr_context* c, const char* who, int64_t first, int64_t n64, const float origin[3], size_t new_bytes, size_t upd_bytes,
                     bool attrs, AttrStep&& attr_step, NewRows&& new_rows)
{
    const uint32_t n = c->n, cnt = (uint32_t)n64;
    const size_t oNew = 0, oAll = pad256(new_bytes);
    const int rc = reposition_body(c, who, std::max(oAll + pad256((size_t)n * 12), upd_bytes), origin, c->st.move_ms, true,
        [](Reorder&, bool*) { return GSR_OK; },
        [&](Reorder& ro, const float** Pout) {
            // 1. the attributes of the same rows, through the old inverse: the update verb as it is (it refuses nothing here that was not refused before)
            if (attrs) {
                const int rca = attr_step();   // (a visibility in force: the step puts new alphas aside; the rule is applied at the end, at the new positions)
                // (stricter than promised: gsr_update does not say whether a HIP failure of its own came before or after its first write --
                //  hipSetDevice, a host -> device copy into the arena, or a kernel -- so ANY of them counts as after it)
                if (rca == GSR_E_HIP) return ro.lost(rca);
                if (rca) return rca;  // (refused before its first write)
                ro.link_ms = c->st.upload_ms[4];
            }
            // 2. the new rows where the splats sit now, and every position in upload order
            float* const Pall = reinterpret_cast<float*>(c->stage + oAll);
            const float* Pnew = nullptr;       // the new rows, in device memory
            hipError_t e = new_rows(reinterpret_cast<float*>(c->stage + oNew), ro.us, &Pnew, &ro.link_ms);
            if (e != hipSuccess) return ro.lost(e);
            e = hipEventRecord(c->up_ev[0], ro.us);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_move_positions, dim3(div_up(n, 256)), dim3(256), 0, ro.us, (uint32_t)first, cnt, n, Pnew, ro.inv_old, c->geoA, c->has_sh ? c->colrow : (uint4*)nullptr, Pall);
                e = hipGetLastError();
            }
            if (e != hipSuccess) return ro.lost(e);
            *Pout = Pall;
            return GSR_OK;
        });
    if (rc) return rc;
    c->st.moves += 1;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// New positions for resident splats ("Position updates").  Only the P rows cross the link; the ordering of an upload runs
// over all positions (formed on the device in upload order), and k_repack carries the resident planes into the new storage order,
// into a spare copy that is then swapped in.  Everything is allocated before the first write to resident memory.
extern "C" int gsr_move(gsr_context* c, int64_t first, int64_t n64, const float* P, const float origin[3], const gsr_attr_update* u)
{
    const char* const who = "gsr_move";
    if (!c || !P) return set_err(GSR_E_INVALID, "gsr_move: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    const int nsh = u ? (u->shx ? 1 : 0) + (u->shy ? 1 : 0) + (u->shz ? 1 : 0) : 0;
    if (nsh != 0 && nsh != 3) return set_err(GSR_E_INVALID, "gsr_move: the three SH arrays come together or not at all");
    if (nsh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_move: SH arrays for a cloud uploaded without SH");
    if (n64 == 0) return GSR_OK;
    const bool attrs = u && (u->Cd || u->alpha || u->scale || u->orient || nsh);
    const size_t cnt = (size_t)n64;
    const size_t upd_bytes = attrs ? update_stage(u, cnt).bytes : 0;   // (so that gsr_update does not grow the arena behind this call's back)
    return move_body(c, who, first, n64, origin, cnt * 12, upd_bytes, attrs,
                     [&]() { return update_rows(c, first, n64, u, false); },
                     [&](float* arena, hipStream_t us, const float** Pnew, double* link_ms) {
                         const double t0 = up_now_ms();
                         hipError_t e = hipMemcpyAsync(arena, P, cnt * 12, hipMemcpyHostToDevice, us);
                         if (e == hipSuccess) e = hipStreamSynchronize(us);   // the caller's array may be freed on return
                         *link_ms += up_now_ms() - t0;
                         *Pnew = arena;
                         return e;
                     });
}

// ---------------------------------------------------------------------------
// Device sources ("Device sources"): upload, update, move and add from float32 arrays that already sit in device memory.
// What the verbs ask of a source pointer, before anything is written or launched -- a wrong pointer must never be found out by
// a kernel: 4-byte aligned; device memory of the context's device, or pinned host memory; and, where the runtime reports the
// allocation's range, every byte inside it.  Pageable host memory fails the attribute query or comes back "unregistered", depending
// on the ROCm version: both are refused, and the runtime's sticky error is cleared.
static int check_device_source(gsr_context* c, const void* p, size_t bytes, const char* who, const char* name)
{
    if (reinterpret_cast<uintptr_t>(p) & 3u) return set_err(GSR_E_INVALID, "%s: %s is not 4-byte aligned", who, name);
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(GSR_E_INVALID, "%s: %s is not device memory (the runtime does not know the pointer)", who, name);
    }
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != c->device) return set_err(GSR_E_INVALID, "%s: %s is memory of device %d, the context renders on device %d", who, name, at.device, c->device);
    } else if (at.type != hipMemoryTypeHost) {      // (host = pinned: hipHostMalloc, hipHostRegister)
        return set_err(GSR_E_INVALID, "%s: %s is neither device memory nor pinned host memory (memory type %d)", who, name, (int)at.type);
    }
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(p))) != hipSuccess) {
        (void)hipGetLastError();                     // (no range on record: the type is what there is to go by)
        return GSR_OK;
    }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at_p = reinterpret_cast<uintptr_t>(p);
    if (at_p < lo || at_p - lo > size || bytes > size - (at_p - lo))
        return set_err(GSR_E_INVALID, "%s: %s: %zu bytes from the pointer reach past the end of its allocation (%zu bytes left)", who, name, bytes,
                       at_p >= lo && at_p - lo <= size ? size - (at_p - lo) : (size_t)0);
    return GSR_OK;
}

extern "C" int gsr_debug_check_device_source(gsr_context* c, const void* p, int64_t bytes)
{
    if (!c || !p || bytes < 0) return set_err(GSR_E_INVALID, "gsr_debug_check_device_source: bad argument");
    return check_device_source(c, p, (size_t)bytes, "gsr_debug_check_device_source", "the pointer");
}

// every non-NULL array of a, for n rows (sh_vec3_per_point is in range when sh is given: the callers looked)
static int check_device_attrs(gsr_context* c, const gsr_device_attrs* a, size_t n, const char* who)
{
    int rc = GSR_OK;
    auto look = [&](const float* p, size_t floats_per_row, const char* name) {
        if (p && !rc) rc = check_device_source(c, p, n * floats_per_row * 4, who, name);
    };
    look(a->P, 3, "P"); look(a->Cd, 3, "Cd"); look(a->alpha, 1, "alpha"); look(a->scale, 3, "scale"); look(a->orient, 4, "orient");
    look(a->sh, a->sh ? (size_t)a->sh_vec3_per_point * 3 : 0, "sh");
    return rc;
}

// n rows of a device source into the arena behind its first `at` rows, on `us`; complete on return, so the caller's arrays may be
// overwritten.  P and alpha as they are (the runtime picks the direction: a source may be pinned host memory); the rest is quantised
// straight from the caller's arrays.
static hipError_t stage_device_rows(const gsr_context* c, const UpArena& A, size_t at, uint32_t n, const gsr_device_attrs* a, hipStream_t us)
{
    hipError_t e = hipMemcpyAsync(A.P + 3 * at, a->P, (size_t)n * 12, hipMemcpyDefault, us);
    if (e == hipSuccess)
        e = a->alpha ? hipMemcpyAsync(A.alpha + at, a->alpha, (size_t)n * 4, hipMemcpyDefault, us)
                     : hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(A.alpha + at), 0x3f800000, n, us);      // missing opacity: opaque
    if (e == hipSuccess) {
        GsrRawSh sh{};
        sh.scheme = a->sh ? 1 : 0;
        sh.vec3_per_point = a->sh_vec3_per_point;
        sh.array = a->sh;
        hipLaunchKernelGGL(k_quantize_raw, dim3(div_up(n, 256)), dim3(256), 0, us, n, a->Cd, a->scale, a->orient, sh, A.Cd + 3 * at, A.scale + 3 * at, A.orient + 4 * at,
                           c->has_sh ? A.shx + 16 * at : (uint16_t*)nullptr, c->has_sh ? A.shy + 16 * at : (uint16_t*)nullptr, c->has_sh ? A.shz + 16 * at : (uint16_t*)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    return e;
}

extern "C" int gsr_upload_append_device(gsr_context* c, int64_t n64, const gsr_device_attrs* a)
{
    if (!c || !c->uploading) return set_err(GSR_E_INVALID, "gsr_upload_append_device: no upload in progress");
    if (!a) return set_err(GSR_E_INVALID, "gsr_upload_append_device: attrs is NULL");
    if (n64 < 0 || (uint64_t)n64 + c->up_filled > c->up_total)
        return set_err(GSR_E_INVALID, "gsr_upload_append_device: %lld splats exceed the %u announced", (long long)n64, c->up_total);
    if (n64 == 0) return GSR_OK;
    if (!a->P) return set_err(GSR_E_INVALID, "gsr_upload_append_device: P is NULL");
    if (c->has_sh != (a->sh != nullptr)) return set_err(GSR_E_INVALID, "gsr_upload_append_device: SH presence differs from gsr_upload_begin");
    if (a->sh && (a->sh_vec3_per_point < 1 || a->sh_vec3_per_point > 16))
        return set_err(GSR_E_INVALID, "gsr_upload_append_device: sh_vec3_per_point = %d is not within 1..16", a->sh_vec3_per_point);
    const uint32_t n = (uint32_t)n64;
    int rc = check_device_attrs(c, a, n, "gsr_upload_append_device");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));          // a producer queued on the public stream has finished
    // behind the entries before this one
    const hipError_t e = stage_device_rows(c, up_arena(c->stage, c->up_total, c->has_sh), c->up_filled, n, a, c->slot[0].own);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_upload_append_device: %s", hipGetErrorString(e));
    c->up_filled += n;
    return GSR_OK;
}

// what gsr_update_device and gsr_move_device refuse of a before they look at its pointers (the range is the caller's to check first)
static int refuse_device_update(gsr_context* c, const gsr_device_attrs* a, const char* who)
{
    if (a->sh && !c->has_sh) return set_err(GSR_E_INVALID, "%s: sh for a cloud uploaded without SH", who);
    if (a->sh && (a->sh_vec3_per_point < 1 || a->sh_vec3_per_point > 16))
        return set_err(GSR_E_INVALID, "%s: sh_vec3_per_point = %d is not within 1..16", who, a->sh_vec3_per_point);
    return GSR_OK;
}

// gsr_update_device behind its refusals: gsr_update without the staging -- k_update_f32 reads the caller's rows where they are
static int update_device_rows(gsr_context* c, int64_t first, uint32_t n, const gsr_device_attrs* a, const char* who, bool vis_rule /* as update_rows takes it */)
{
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);      // the public stream (a producer queued there has finished), and no in-place write under a frame in flight
    if (rc) return rc;
    if ((rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    const GsrUpdateSrcF32 src{a->alpha, a->Cd, a->scale, a->orient, a->sh, a->sh ? a->sh_vec3_per_point : 0};
    return queue_update(c, who, c->slot[0].own, (uint32_t)first, n, src, a->alpha != nullptr, a->scale || a->orient, vis_rule, 0.0 /* nothing crossed the link */);
}

extern "C" int gsr_update_device(gsr_context* c, int64_t first, int64_t n64, const gsr_device_attrs* a)
{
    const char* const who = "gsr_update_device";
    if (!c || !a) return set_err(GSR_E_INVALID, "gsr_update_device: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    if (a->P) return set_err(GSR_E_INVALID, "gsr_update_device: P is given: a position is gsr_move_device");
    if ((rc = refuse_device_update(c, a, who))) return rc;
    if (n64 == 0 || !(a->Cd || a->alpha || a->scale || a->orient || a->sh)) return GSR_OK;
    if ((rc = check_device_attrs(c, a, (size_t)n64, who))) return rc;
    return update_device_rows(c, first, (uint32_t)n64, a, who, true);
}

extern "C" int gsr_move_device(gsr_context* c, int64_t first, int64_t n64, const float origin[3], const gsr_device_attrs* a)
{
    const char* const who = "gsr_move_device";
    if (!c || !a) return set_err(GSR_E_INVALID, "gsr_move_device: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    if (!a->P) return set_err(GSR_E_INVALID, "gsr_move_device: P is NULL");
    if ((rc = refuse_device_update(c, a, who))) return rc;
    if (n64 == 0) return GSR_OK;
    if ((rc = check_device_attrs(c, a, (size_t)n64, who))) return rc;
    const bool attrs = a->Cd || a->alpha || a->scale || a->orient || a->sh;
    // (k_move_positions reads the caller's P where it is, and the attribute step stages nothing: the arena holds the positions in upload order only)
    return move_body(c, who, first, n64, origin, 0, 0, attrs,
                     [&]() { return update_device_rows(c, first, (uint32_t)n64, a, who, false); },
                     [&](float*, hipStream_t, const float** Pnew, double*) { *Pnew = a->P; return hipSuccess; });
}

// ---------------------------------------------------------------------------
// Visibility (k_visibility.h): resident splats hidden by crop volumes or a mask.  The verb and its hooks -- behind a
// complete upload, behind an alpha update, behind a move, a removal and an add -- that run only while a visibility is in force.
static_assert(sizeof(gsr_crop_volume) == sizeof(GsrVisVolume) && offsetof(gsr_visibility, mask) == sizeof(GsrVisRule) &&
              offsetof(gsr_visibility, volume) == offsetof(GsrVisRule, vol) && GSR_VIS_MAX_VOLUMES == GSR_VIS_VOLUMES &&
              GSR_VOL_BOX == GSR_VISK_BOX && GSR_VOL_ELLIPSOID == GSR_VISK_ELLIPSOID, "gsr_visibility begins with the kernel's rule");

// what is wrong with the caller's struct (NULL: nothing; v == NULL is "everything visible")
static const char* visibility_error(const gsr_visibility* v)
{
    if (!v) return nullptr;
    if (v->n_volumes < 0 || v->n_volumes > GSR_VIS_MAX_VOLUMES) return "n_volumes is not within 0..GSR_VIS_MAX_VOLUMES";
    if (v->reserved_ != 0) return "reserved_ is not 0";
    for (int k = 0; k < v->n_volumes; ++k) {
        if (v->volume[k].kind != GSR_VOL_BOX && v->volume[k].kind != GSR_VOL_ELLIPSOID) return "unknown volume kind";
        if (v->volume[k].invert != 0 && v->volume[k].invert != 1) return "invert is neither 0 nor 1";
    }
    return nullptr;
}
// the rule of v as the kernel takes it (volumes beyond n_volumes zeroed)
static GsrVisRule visibility_rule(const gsr_visibility* v)
{
    GsrVisRule r{};
    if (v) {
        r.n_volumes = v->n_volumes;
        std::memcpy(r.vol, v->volume, sizeof(GsrVisVolume) * (size_t)v->n_volumes);
    }
    return r;
}

extern "C" int gsr_visibility_eval(const gsr_visibility* v, const float* P, int64_t first, int64_t n, uint8_t* visible_out)
{
    const char* bad = visibility_error(v);
    if (bad) return set_err(GSR_E_INVALID, "gsr_visibility_eval: %s", bad);
    if (first < 0 || n < 0 || (n > 0 && (!P || !visible_out))) return set_err(GSR_E_INVALID, "gsr_visibility_eval: bad argument");
    const uint32_t* const mask = v ? v->mask : nullptr;
    if (mask && (v->mask_splats < 0 || first > v->mask_splats || n > v->mask_splats - first))
        return set_err(GSR_E_INVALID, "gsr_visibility_eval: splats [%lld, %lld + %lld) are not within the %lld of the mask", (long long)first, (long long)first,
                       (long long)n, (long long)v->mask_splats);
    const GsrVisRule rule = visibility_rule(v);
    for (int64_t k = 0; k < n; ++k) {
        const uint64_t i = (uint64_t)(first + k);
        visible_out[k] = gsr_splat_visible(rule, P[3 * k], P[3 * k + 1], P[3 * k + 2], mask ? mask[i >> 5] : 0u, (uint32_t)(i & 31u)) ? 1 : 0;
    }
    return GSR_OK;
}

// room for the true alphas and the counters: before the first write of whoever applies the rule
static int vis_ensure_buffers(gsr_context* c)
{
    int rc = GSR_OK;
    if (!c->alpha0 && (rc = c->alpha0.alloc((size_t)c->cap))) return rc;
    const size_t words = (size_t)GSR_VIS_COUNTER_SLOTS * GSR_VIS_COUNTER_STRIDE;
    if (!c->vis_counters && (rc = c->vis_counters.alloc(words))) return rc;
    if (!c->vis_h_counters && c->vis_h_counters.alloc(words, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "no pinned host memory for the visibility counters");
    }
    return GSR_OK;
}

// On `us`: the true alphas of the splats [cap_first, cap_first + cap_cnt) (upload order; geoA holds them; 0: none) into alpha0 -- through
// the inverse of the storage order, which the caller has ensured -- then, with `apply`, the rule over every storage slot.  Waits for
// the counters: *changed = a resident bit changed, c->vis_hidden = what is hidden now.
static hipError_t vis_apply(gsr_context* c, hipStream_t us, uint32_t cap_first, uint32_t cap_cnt, bool apply, const GsrVisRule& rule,
                            const uint32_t* mask, bool* changed)
{
    const uint32_t n = c->n;
    if (changed) *changed = false;
    if (n == 0) { c->vis_hidden = 0; return hipSuccess; }
    if (!c->alpha0 || !c->vis_counters || !c->vis_h_counters) return hipErrorInvalidValue;       // (the callers allocate before their first write)
    if (cap_cnt) hipLaunchKernelGGL(k_alpha_capture, dim3(div_up(cap_cnt, 256)), dim3(256), 0, us, cap_first, cap_cnt,
                                    c->perm ? c->wire_inv : (const uint32_t*)nullptr, c->geoA, c->alpha0);
    if (!apply) return hipGetLastError();
    const size_t words = (size_t)GSR_VIS_COUNTER_SLOTS * GSR_VIS_COUNTER_STRIDE;
    hipError_t e = hipMemsetAsync(c->vis_counters, 0, words * 8, us);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_visibility, dim3(div_up(n, 256)), dim3(256), 0, us, n, c->perm, c->geoA, c->has_sh ? c->colrow : (uint4*)nullptr, c->alpha0,
                       mask, rule, c->vis_counters);
    e = hipGetLastError();
    const unsigned long long* const h = c->vis_h_counters;
    if (e == hipSuccess) e = hipMemcpyAsync(c->vis_h_counters, c->vis_counters, words * 8, hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return e;
    unsigned long long n_hidden = 0, n_changed = 0;        // (a slot's words cannot carry: each counts at most n <= 2^31 splats)
    for (size_t k = 0; k < words; k += GSR_VIS_COUNTER_STRIDE) { n_hidden += h[k] & 0xffffffffull; n_changed += h[k] >> 32; }
    c->vis_hidden = (int64_t)n_hidden;
    if (changed) *changed = n_changed != 0;
    return hipSuccess;
}

// behind a complete upload (the generation is the new cloud's): its mask is gone; the volumes in force hide their share of it
static int vis_after_upload(gsr_context* c)
{
    vis_drop_mask(c);
    c->vis_hidden = 0;
    if (!c->vis_on || c->n == 0) return GSR_OK;
    int rc = vis_ensure_buffers(c);
    if (!rc) rc = ensure_inverse_perm(c);
    if (rc) return rc;
    const hipError_t e = vis_apply(c, c->slot[0].own, 0u, c->n, true, c->vis, nullptr, nullptr);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_upload_end: applying the visibility: %s", hipGetErrorString(e));
    return GSR_OK;
}

extern "C" int gsr_set_visibility(gsr_context* c, const gsr_visibility* v)
{
    const char* const who = "gsr_set_visibility";
    if (!c) return set_err(GSR_E_INVALID, "gsr_set_visibility: ctx is NULL");
    const char* bad = visibility_error(v);
    if (bad) return set_err(GSR_E_INVALID, "gsr_set_visibility: %s", bad);
    int rc = refuse_edit(c, who, false);               // (without geometry the volumes wait for gsr_upload_end; only a mask needs a cloud)
    if (rc) return rc;
    const bool has_mask = v && v->mask;
    if (has_mask && !c->has_geometry) return set_err(GSR_E_INVALID, "gsr_set_visibility: a mask belongs to a cloud, and none is resident");
    if (has_mask && v->mask_splats != (int64_t)c->n)
        return set_err(GSR_E_INVALID, "gsr_set_visibility: the mask covers %lld splats, %u are resident", (long long)v->mask_splats, c->n);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = sync_all(c))) return rc;      // no in-place write under a frame in flight
    const GsrVisRule rule = visibility_rule(v);
    if (!c->has_geometry || c->n == 0) {               // nothing to hide yet: the volumes wait for gsr_upload_end
        c->vis_mask.reset();
        c->vis = rule; c->vis_on = rule.n_volumes > 0; c->vis_hidden = 0;
        return GSR_OK;
    }
    const bool on = rule.n_volumes > 0 || has_mask;
    if (!on && !c->vis_on) return GSR_OK;              // everything is visible already
    // ---- everything the call needs, before the first write
    if ((rc = vis_ensure_buffers(c))) return rc;
    const size_t words = ((size_t)c->n + 31) / 32;
    DevMem<uint32_t> mask_new;
    if (has_mask && (rc = mask_new.alloc(words))) return rc;
    // (geoA holds every true alpha exactly while no visibility is in force: that is when they are put aside)
    const bool capture = !c->vis_on;
    if (capture && (rc = ensure_inverse_perm(c))) return rc;
    hipStream_t us = c->slot[0].own;
    hipError_t e = has_mask ? hipMemcpyAsync(mask_new, v->mask, words * 4, hipMemcpyHostToDevice, us) : hipSuccess;
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_set_visibility: %s", hipGetErrorString(e));
    // ---- from here on a failure leaves no geometry (as a failed gsr_move does), and no visibility
    bool changed = false;
    e = vis_apply(c, us, 0u, capture ? c->n : 0u, true, rule, mask_new, &changed);
    // a change of the hidden set is a shape edit, like new alphas: horizons, prefixes, hints and policies of the cloud's frames go
    if (e == hipSuccess && changed) e = after_update(c, true, us, e);
    if (e != hipSuccess) {
        c->vis = GsrVisRule{}; c->vis_on = false;
        drop_geometry(c);
        return set_err(GSR_E_HIP, "gsr_set_visibility: %s", hipGetErrorString(e));
    }
    c->vis_mask = std::move(mask_new);
    c->vis = rule;
    c->vis_on = on;
    return GSR_OK;
}

extern "C" int gsr_get_visibility(gsr_context* c, gsr_visibility* out, int64_t* hidden)
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_visibility: ctx is NULL");
    if (out) {
        std::memset(out, 0, sizeof(*out));
        std::memcpy(out, &c->vis, sizeof(GsrVisRule));
        out->mask_splats = c->vis_mask ? (int64_t)c->n : 0;
    }
    if (hidden) *hidden = c->vis_hidden;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// The mask intake of gsr_remove, gsr_read_masked*, gsr_duplicate, gsr_transform and gsr_grade: the caller's
// ceil(n / 32) words over the n resident splats, in host or device memory (NULL: the verb says what).  Where each verb checks, waits
// and stages is the verb's own.
struct MaskArg {
    const uint32_t* mask;
    bool is_device;
    uint32_t n;

    size_t words() const { return ((size_t)n + 31) / 32; }
    // what a host mask takes of the staging arena (0: a device or NULL mask)
    size_t stage_bytes() const { return mask && !is_device ? words() * 4 : 0; }
    // a device mask before anything is launched (the empty cloud has no word to look at)
    int check(gsr_context* c, const char* who) const
    {
        return mask && is_device && n ? check_device_source(c, mask, words() * 4, who, "mask") : GSR_OK;
    }
    // *dmask = the words the kernels read: a host mask copied to `at` of the arena and waited for (the caller's mask may be freed on
    // return; link_ms, may be NULL, += what that took), a device mask as it is, NULL for NULL
    hipError_t to_device(gsr_context* c, hipStream_t us, size_t at, double* link_ms, const uint32_t** dmask) const
    {
        *dmask = mask;
        if (!stage_bytes()) return hipSuccess;
        const double t0 = up_now_ms();
        uint32_t* const staged = reinterpret_cast<uint32_t*>(c->stage + at);
        hipError_t e = hipMemcpyAsync(staged, mask, words() * 4, hipMemcpyHostToDevice, us);
        if (e == hipSuccess) e = hipStreamSynchronize(us);
        if (e != hipSuccess) return e;
        if (link_ms) *link_ms += up_now_ms() - t0;
        *dmask = staged;
        return hipSuccess;
    }
};

// the pinned words a mask verb's count is read back into
static int ensure_h_word(gsr_context* c, const char* who)
{
    if (!c->h_word && c->h_word.alloc(2, 0)) {
        (void)hipGetLastError();
        return set_err(GSR_E_OOM, "%s: no pinned host memory for the count", who);
    }
    return GSR_OK;
}

// *count = the set bits of the device mask dmask below n (k_mask_count into the word at `at` of the arena; waited for).  The caller
// has ensured the arena and the pinned words.  More than n is a HIP failure.
static int count_mask_bits(gsr_context* c, hipStream_t us, uint32_t n, const uint32_t* dmask, size_t at, const char* who, uint32_t* count)
{
    uint32_t* const dcount = reinterpret_cast<uint32_t*>(c->stage + at);
    HIP_TRY(hipMemsetAsync(dcount, 0, 4, us));
    hipLaunchKernelGGL(k_mask_count, dim3(div_up((uint32_t)(((size_t)n + 31) / 32), 256)), dim3(256), 0, us, n, dmask, dcount);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_word, dcount, 4, hipMemcpyDeviceToHost, us));
    HIP_TRY(hipStreamSynchronize(us));
    *count = c->h_word[0];
    if (*count > n) return set_err(GSR_E_HIP, "%s: the reduction counted %u bits below %u", who, *count, n);
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Removal (k_remove.h): resident splats deleted on the GPU.  A move whose source is a subset: mark, scan and compact in
// upload order, then the ordering of an upload over the survivors' positions, k_repack into the spare planes, the swap.
extern "C" int gsr_remove_map(const uint32_t* mask, int64_t n, int32_t* new_index, int64_t* n_left)
{
    if (n < 0 || n > 0x7fffffffll || (n > 0 && !mask)) return set_err(GSR_E_INVALID, "gsr_remove_map: bad argument");
    int64_t left = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool gone = ((mask[i >> 5] >> (i & 31)) & 1u) != 0u;
        if (new_index) new_index[i] = gone ? -1 : (int32_t)left;
        if (!gone) ++left;
    }
    if (n_left) *n_left = left;
    return GSR_OK;
}

extern "C" int gsr_get_removal(gsr_context* c, int64_t* removals, int64_t* removed_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_removal: ctx is NULL");
    return c->rm.report(removals, removed_last, ms);
}

extern "C" int gsr_remove(gsr_context* c, const uint32_t* mask, int mask_is_device, int flags, int64_t* n_left)
{
    const char* const who = "gsr_remove";
    if (!c) return set_err(GSR_E_INVALID, "gsr_remove: ctx is NULL");
    if (flags & ~GSR_REMOVE_HIDDEN) return set_err(GSR_E_INVALID, "gsr_remove: unknown flag bits %#x", flags & ~GSR_REMOVE_HIDDEN);
    if (!mask && !(flags & GSR_REMOVE_HIDDEN)) return set_err(GSR_E_INVALID, "gsr_remove: mask is NULL and GSR_REMOVE_HIDDEN is not set");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const uint32_t n = c->n;
    const MaskArg mk{mask, mask_is_device != 0, n};
    const size_t words = mk.words();
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = mk.check(c, who))) return rc;
    Reorder ro(c, who, true);
    if ((rc = sync_all(c))) return rc;   // the public stream (a producer of a device mask queued there has finished), and no write under a frame in flight
    const bool hidden = (flags & GSR_REMOVE_HIDDEN) && c->vis_on;
    if (n == 0 || (!mask && !hidden)) {                // nothing can go
        if (n_left) *n_left = (int64_t)n;
        return GSR_OK;
    }
    hipStream_t us = ro.us;
    // ---- the scratch of mark, scan and compaction, in the staging arena
    const uint32_t nblocks = div_up(n, (uint32_t)GSR_REMOVE_BLOCK);
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oMask = place(mk.stage_bytes()), oKeep = place((size_t)nblocks * GSR_REMOVE_SLOTS * 8), oCnt = place((size_t)nblocks * 4),
                 oOff = place(((size_t)nblocks + 1) * 4), oP = place((size_t)n * 12), oSlot = place((size_t)n * 4);
    if ((rc = ensure_stage(c, off)) || (rc = ensure_h_word(c, who))) return rc;
    if ((rc = ro.old_inverse(true))) return rc;        // (the mark reads through it)
    const uint32_t* const inv_old = ro.inv_old;
    unsigned long long* const keep = reinterpret_cast<unsigned long long*>(c->stage + oKeep);
    uint32_t* const counts = reinterpret_cast<uint32_t*>(c->stage + oCnt);
    uint32_t* const offsets = reinterpret_cast<uint32_t*>(c->stage + oOff);
    float* const Pup = reinterpret_cast<float*>(c->stage + oP);
    uint32_t* const src_slot = reinterpret_cast<uint32_t*>(c->stage + oSlot);
    // ---- 1, 2. which splats stay, and how many: nothing resident is written yet
    const uint32_t* dmask = nullptr;
    HIP_TRY(mk.to_device(c, us, oMask, &ro.link_ms, &dmask));
    HIP_TRY(hipEventRecord(c->up_ev[0], us));
    if (hidden)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_remove_mark<true>), dim3(nblocks), dim3(GSR_REMOVE_THREADS), 0, us, n, dmask, inv_old, c->geoA, c->vis_mask, c->vis, keep, counts);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_remove_mark<false>), dim3(nblocks), dim3(GSR_REMOVE_THREADS), 0, us, n, dmask, inv_old, c->geoA, (const uint32_t*)nullptr, GsrVisRule{}, keep, counts);
    hipLaunchKernelGGL(k_remove_scan, dim3(1), dim3(GSR_REMOVE_SCAN_THREADS), 0, us, nblocks, counts, offsets);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_word, offsets + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, us));
    HIP_TRY(hipStreamSynchronize(us));
    const uint32_t n1 = c->h_word[0];
    if (n1 > n) return set_err(GSR_E_HIP, "gsr_remove: the scan counted %u survivors of %u splats", n1, n);
    if (n1 == n) {                                     // nothing goes: no resident bit changes, nothing is invalidated
        if (n_left) *n_left = (int64_t)n;
        return GSR_OK;
    }
    // ---- everything the rest needs, before the first write to resident memory or to the visibility's state
    const bool vis = c->vis_on;
    if (n1 > 0) {
        if ((rc = ro.prepare(n1)) || (rc = ensure_spare_planes(c, c->cap, true))) return rc;
        if (vis) {
            if (!(rc = vis_ensure_buffers(c)) && !c->alpha0_2) rc = c->alpha0_2.alloc((size_t)c->cap);
            if (!rc && c->vis_mask) rc = ro.mask_new.alloc(words);
            if (rc) return rc;
        }
    }
    // ---- from here on a failure leaves no geometry
    hipError_t e = hipSuccess;
    if (n1 == 0) {
        // the empty cloud, as gsr_upload of 0 splats leaves it: no order, no clusters, no mask
        drop_order(c);
        c->n = 0; c->bbox_ok = false; c->up_total = c->up_filled = 0; c->st.n_splats = 0;
        vis_drop_mask(c);
        c->vis_hidden = 0;
        e = hipEventRecord(c->up_ev[1], us);
        if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
        if (e == hipSuccess) e = hipStreamSynchronize(us);
        if (e != hipSuccess) return ro.lost(e);
    } else {
        // 3. the survivors' positions, old slots, true alphas and mask bits at their new upload indices
        if (ro.mask_new) e = hipMemsetAsync(ro.mask_new, 0, words * 4, us);
        if (e == hipSuccess) {
            if (vis)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_remove_compact<true>), dim3(nblocks), dim3(GSR_REMOVE_THREADS), 0, us, keep, offsets, inv_old, c->geoA, Pup, src_slot,
                                   c->alpha0, c->alpha0_2, c->vis_mask, ro.mask_new);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_remove_compact<false>), dim3(nblocks), dim3(GSR_REMOVE_THREADS), 0, us, keep, offsets, inv_old, c->geoA, Pup, src_slot,
                                   (const float*)nullptr, (float*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
            e = hipGetLastError();
        }
        if (e != hipSuccess) return ro.lost(e);
        // 4. the ordering of an upload over the survivors, and their planes into the spare set: k_repack as a move runs it, with the
        // survivors' old slots in the place of the old order's inverse
        if ((rc = ro.order(Pup, n1))) return ro.lost(rc);
        e = queue_repack(c, us, n1, ro.perm_new, src_slot);
        if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
        if (e == hipSuccess) e = hipStreamSynchronize(us);
        if (e != hipSuccess) return ro.lost(e);
        // 5. the swap, and the upload-ordered state of the visibility with it
        ro.commit(n1, div_up(n1, GSR_CLUSTER), true);
        if (vis) c->alpha0.swap(c->alpha0_2);
    }
    // 6. the volumes against the survivors, in the order they sit in now; a new cloud to everything a frame keeps
    if ((rc = ro.finish(c->rm.ms, false))) return rc;
    c->rm.calls += 1;
    c->rm.last = (int64_t)n - (int64_t)n1;
    if (n_left) *n_left = (int64_t)n1;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Adding (k_add.h): splats appended to the resident cloud on the GPU.  gsr_remove the other way round: the new rows are
// staged, every position goes through the ordering of an upload, k_add_pack writes the spare planes from the resident planes (old
// splats) and the staged rows (new ones), the swap.  The one verb that can need MORE room than the context has: the capacity policy.
extern "C" int64_t gsr_add_capacity(int64_t capacity, int64_t n_needed)
{
    if (capacity < 0 || n_needed < 0 || n_needed > 0x7fffffffll)
        return (int64_t)set_err(GSR_E_INVALID, "gsr_add_capacity: bad argument (%lld, %lld)", (long long)capacity, (long long)n_needed);
    if (n_needed <= capacity) return capacity;
    return std::min<int64_t>(n_needed + n_needed / 4, 0x7fffffffll);     // (the 25 % headroom the list buffers take)
}

extern "C" int gsr_get_add(gsr_context* c, int64_t* adds, int64_t* added_last, int64_t* capacity, int64_t* grows, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_add: ctx is NULL");
    if (capacity) *capacity = (int64_t)c->cap;
    if (grows) *grows = c->add_grows;
    return c->add.report(adds, added_last, ms);
}

// what both forms refuse before they look at their arrays; *done: m == 0, there is nothing to do
static int add_refuse(gsr_context* c, int64_t m, int64_t* n_total, const char* who, bool* done)
{
    *done = false;
    if (!c) return set_err(GSR_E_INVALID, "%s: ctx is NULL", who);
    if (m < 0) return set_err(GSR_E_INVALID, "%s: bad splat count %lld", who, (long long)m);
    const int rc = refuse_edit(c, who);
    if (rc) return rc;
    if ((int64_t)c->n + m > 0x7fffffffll) return set_err(GSR_E_INVALID, "%s: %u + %lld splats are more than a context holds", who, c->n, (long long)m);
    if (m == 0) {                                      // nothing changes, nothing is invalidated
        if (n_total) *n_total = (int64_t)c->n;
        *done = true;
    }
    return GSR_OK;
}

// The body of gsr_add and gsr_add_device, behind their refusals.  stage_rows(arena of m rows, stream, &link_ms): the new rows into the
// arena in gsr_upload_append's layout, complete when it returns.
template <class StageRows>
static int add_body(gsr_context* c, const char* who, uint32_t m, StageRows&& stage_rows, int64_t* n_total)
{
    HIP_TRY(hipSetDevice(c->device));
    Reorder ro(c, who, false);
    int rc = sync_all(c);      // the public stream (a producer of a device source queued there has finished), and no write under a frame in flight
    if (rc) return rc;
    const uint32_t n0 = c->n, n1 = n0 + m, nclus1 = div_up(n1, GSR_CLUSTER);
    hipStream_t us = ro.us;
    const uint32_t cap0 = c->cap, cap1 = (uint32_t)gsr_add_capacity((int64_t)cap0, (int64_t)n1);
    const bool grow = cap1 != cap0;
    const bool vis = c->vis_on;
    // ---- everything the call needs, before the first write to resident memory or to the visibility's state
    const size_t oAll = pad256(up_arena(nullptr, m, c->has_sh).bytes);
    if ((rc = ensure_stage(c, oAll + pad256((size_t)n1 * 12)))) return rc;
    if ((rc = ro.prepare(n1))) return rc;
    if (grow) {
        // the spare set is at the old capacity: it goes first (nothing reads it), and the destination set comes at the new one
        free_spare_planes(c);
        if ((rc = ensure_spare_planes(c, cap1, false))) return rc;
        for (int k = 0; k < GSR_MAX_SLOTS; ++k)
            if ((rc = alloc_splat_arrays(ro.slot_new[k], cap1))) {
                free_spare_planes(c);
                return rc;
            }
    } else if ((rc = ensure_spare_planes(c, cap0, true))) {
        return rc;
    }
    // (the spare cluster bounds in force are sized for a removal, which only ever needs fewer: an add brings its own)
    if ((rc = ro.clusA_new.alloc(nclus1)) || (rc = ro.clusB_new.alloc(nclus1))) return rc;
    if (vis) {
        if ((rc = vis_ensure_buffers(c))) return rc;
        if (grow && (rc = ro.alpha0_new.alloc((size_t)cap1))) return rc;
        if (c->vis_mask && (rc = ro.mask_new.alloc(((size_t)n1 + 31) / 32))) return rc;
    }
    if ((rc = ro.old_inverse(true))) return rc;
    // nothing can fail for lack of memory any more: the larger buffers take their places (none of them holds anything a frame keeps)
    c->clusA2 = std::move(ro.clusA_new); c->clusB2 = std::move(ro.clusB_new);
    if (grow) {
        for (int k = 0; k < GSR_MAX_SLOTS; ++k) slot_take_splat_arrays(c->slot[k], std::move(ro.slot_new[k]));
        c->alpha0_2.reset();
        if (!vis) c->alpha0.reset();                 // (at the old capacity, and valid only while a visibility is in force)
    }
    // ---- from here on a failure leaves no geometry
    ro.spare_outgrown = grow;
    // 1. the new rows, staged
    const UpArena A = up_arena(c->stage, m, c->has_sh);
    hipError_t e = stage_rows(A, us, &ro.link_ms);
    if (e != hipSuccess) return ro.lost(set_err(GSR_E_HIP, "%s: staging the new rows: %s", who, hipGetErrorString(e)));
    // 2. every position in upload order: the resident ones from geoA through the old order's inverse, the new ones behind them
    float* const Pall = reinterpret_cast<float*>(c->stage + oAll);
    const uint32_t* const inv_old = ro.inv_old;
    e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess && n0) {
        hipLaunchKernelGGL(k_move_positions, dim3(div_up(n0, 256)), dim3(256), 0, us, 0u, 0u, n0, (const float*)nullptr, inv_old, c->geoA, (uint4*)nullptr, Pall);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(Pall + 3 * (size_t)n0, A.P, (size_t)m * 12, hipMemcpyDeviceToDevice, us);
    if (e != hipSuccess) return ro.lost(e);
    // 3. the ordering of an upload over all of them
    if ((rc = ro.order(Pall, n1))) return ro.lost(rc);
    // 4. the planes of the larger cloud into the spare set: resident splats from the planes, new ones from the staged rows
    const GsrPackSrc src{A.P, A.alpha, A.Cd, A.scale, A.orient, A.shx, A.shy, A.shz};
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_add_pack<decltype(sh)::value>), dim3(nclus1), dim3(GSR_PACK_THREADS), 0, us, n1, n0, cap0, cap1, src, ro.perm_new, inv_old,
                           c->geoA, c->geoB, c->col, c->colrow, c->geoA2, c->geoB2, c->col2, c->colrow2, c->clusA2, c->clusB2);
    });
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
    // ... and the upload-ordered state of a visibility in force: the true alphas of the new rows behind the old ones, the mask extended
    // by clear bits
    if (e == hipSuccess && vis) {
        float* const a0 = grow ? ro.alpha0_new : c->alpha0;
        if (grow && n0) e = hipMemcpyAsync(a0, c->alpha0, (size_t)n0 * 4, hipMemcpyDeviceToDevice, us);
        if (e == hipSuccess) e = hipMemcpyAsync(a0 + n0, A.alpha, (size_t)m * 4, hipMemcpyDeviceToDevice, us);
        if (e == hipSuccess && ro.mask_new) {
            const uint32_t words1 = (uint32_t)(((size_t)n1 + 31) / 32);
            hipLaunchKernelGGL(k_add_mask_extend, dim3(div_up(words1, 256)), dim3(256), 0, us, n0, words1, c->vis_mask, ro.mask_new);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return ro.lost(e);
    // 5. the swap.  What becomes the spare set is the cloud before: its cluster bounds are too few for the next edit of this one, and
    // after a growth its planes are at the wrong capacity -- both go, and the next edit that needs spare planes allocates them again
    ro.commit(n1, nclus1, true);
    c->clusA2.reset(); c->clusB2.reset();
    if (grow) {
        free_spare_planes(c);
        c->cap = cap1;
        if (vis) c->alpha0 = std::move(ro.alpha0_new);
    }
    // 6, 7. the rule of a visibility in force over the whole cloud; a new cloud to everything a frame keeps
    if ((rc = ro.finish(c->add.ms, false))) return rc;
    c->add.calls += 1;
    c->add.last = (int64_t)m;
    if (grow) c->add_grows += 1;
    if (n_total) *n_total = (int64_t)n1;
    return GSR_OK;
}

extern "C" int gsr_add(gsr_context* c, int64_t m64, const float* P, const uint16_t* Cd, const float* alpha, const uint16_t* scale,
                       const uint16_t* orient, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, int64_t* n_total)
{
    const char* const who = "gsr_add";
    bool done = false;
    int rc = add_refuse(c, m64, n_total, who, &done);
    if (rc || done) return rc;
    if (!P || !Cd || !alpha || !scale || !orient) return set_err(GSR_E_INVALID, "gsr_add: NULL attribute array");
    const int nsh = (shx ? 1 : 0) + (shy ? 1 : 0) + (shz ? 1 : 0);
    if (nsh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_add: SH arrays for a cloud uploaded without SH");
    if (c->has_sh && nsh != 3) return set_err(GSR_E_INVALID, "gsr_add: the cloud has SH and the three SH arrays are not all given");
    const uint32_t m = (uint32_t)m64;
    return add_body(c, who, m, [&](const UpArena& A, hipStream_t us, double* link_ms) {
        const double t0 = up_now_ms();
        const hipError_t e = stage_host_rows(A, 0, m, GsrPackSrc{P, alpha, Cd, scale, orient, shx, shy, shz}, c->has_sh, us);
        *link_ms = up_now_ms() - t0;
        return e;
    }, n_total);
}

extern "C" int gsr_add_device(gsr_context* c, int64_t m64, const gsr_device_attrs* a, int64_t* n_total)
{
    const char* const who = "gsr_add_device";
    bool done = false;
    int rc = add_refuse(c, m64, n_total, who, &done);
    if (rc || done) return rc;
    if (!a) return set_err(GSR_E_INVALID, "gsr_add_device: attrs is NULL");
    if (!a->P) return set_err(GSR_E_INVALID, "gsr_add_device: P is NULL");
    if (c->has_sh != (a->sh != nullptr)) return set_err(GSR_E_INVALID, "gsr_add_device: SH presence differs from the resident cloud's");
    if (a->sh && (a->sh_vec3_per_point < 1 || a->sh_vec3_per_point > 16))
        return set_err(GSR_E_INVALID, "gsr_add_device: sh_vec3_per_point = %d is not within 1..16", a->sh_vec3_per_point);
    const uint32_t m = (uint32_t)m64;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = check_device_attrs(c, a, m, who))) return rc;
    return add_body(c, who, m, [&](const UpArena& A, hipStream_t us, double*) { return stage_device_rows(c, A, 0, m, a, us); }, n_total);
}

// ---------------------------------------------------------------------------
// Copying (k_copy.h): selected resident splats read out (gsr_read_masked*, gsr_resident_read.h) or duplicated.  Both
// begin with gsr_remove's compaction, the SELECTED splats in the survivors' place.
extern "C" int gsr_copy_map(const uint32_t* mask, int64_t n, int32_t* rows, int64_t* m)
{
    if (n < 0 || n > 0x7fffffffll || (n > 0 && !mask)) return set_err(GSR_E_INVALID, "gsr_copy_map: bad argument");
    int64_t r = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (((mask[i >> 5] >> (i & 31)) & 1u) == 0u) continue;
        if (rows) rows[r] = (int32_t)i;
        ++r;
    }
    if (m) *m = r;
    return GSR_OK;
}

// The selection of a mask over the n resident splats, counted: the scratch of mark and scan at the head of the staging arena (a host
// mask staged, the bitmap, the block counts, the block offsets; `bytes` in all), and the two launches.  What a verb needs behind the
// count -- the row list, the positions, the destination rows -- lies behind `bytes`, sized by the count: grow() makes that room, and
// counts again if the arena had to move (a host mask is still the caller's until the verb returns).
struct CopySelection {
    const MaskArg mask;                // the caller's (NULL: every splat)
    const uint32_t n, nblocks;
    size_t oMask = 0, oSel = 0, oCnt = 0, oOff = 0, bytes = 0;

    explicit CopySelection(const MaskArg& m) : mask(m), n(m.n), nblocks(div_up(m.n, (uint32_t)GSR_REMOVE_BLOCK))
    {
        auto place = [&](size_t b) { const size_t at = bytes; bytes += pad256(b); return at; };
        oMask = place(mask.stage_bytes()); oSel = place((size_t)nblocks * GSR_REMOVE_SLOTS * 8); oCnt = place((size_t)nblocks * 4);
        oOff = place(((size_t)nblocks + 1) * 4);
    }
    const unsigned long long* sel(const gsr_context* c) const { return reinterpret_cast<const unsigned long long*>(c->stage + oSel); }
    const uint32_t* offsets(const gsr_context* c) const { return reinterpret_cast<const uint32_t*>(c->stage + oOff); }

    // what the call needs before count(): the arena for the scratch, the pinned word of the count
    int prepare(gsr_context* c, const char* who) const
    {
        const int rc = ensure_stage(c, bytes);
        return rc ? rc : ensure_h_word(c, who);
    }
    // mark and scan on `us`, and the wait for the total: *m = the selected splats.  link_ms (may be NULL) += what a host mask took.
    hipError_t count(gsr_context* c, hipStream_t us, uint32_t* m, double* link_ms) const
    {
        const uint32_t* dmask = nullptr;
        hipError_t e = mask.to_device(c, us, oMask, link_ms, &dmask);
        if (e != hipSuccess) return e;
        uint32_t* const counts = reinterpret_cast<uint32_t*>(c->stage + oCnt);
        uint32_t* const offs = reinterpret_cast<uint32_t*>(c->stage + oOff);
        hipLaunchKernelGGL(k_copy_mark, dim3(nblocks), dim3(GSR_REMOVE_THREADS), 0, us, n, dmask, reinterpret_cast<unsigned long long*>(c->stage + oSel), counts);
        hipLaunchKernelGGL(k_remove_scan, dim3(1), dim3(GSR_REMOVE_SCAN_THREADS), 0, us, nblocks, counts, offs);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(c->h_word, offs + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, us);
        if (e == hipSuccess) e = hipStreamSynchronize(us);
        if (e == hipSuccess) *m = c->h_word[0];
        return e;
    }
    // room for `total` bytes of the arena (the scratch included), behind count(): the bitmap and the offsets are there afterwards.
    // Whether the arena was replaced is read off its CAPACITY: ensure_stage releases before it allocates, and the larger allocation
    // may well come back at the address of the one released, with nothing of its content.
    int grow(gsr_context* c, hipStream_t us, size_t total, uint32_t m, const char* who) const
    {
        const bool replaced = total > c->stage.cap();
        const int rc = ensure_stage(c, total);
        if (rc || !replaced) return rc;
        uint32_t again = 0;
        const hipError_t e = count(c, us, &again, nullptr);
        if (e != hipSuccess) return set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
        if (again != m) return set_err(GSR_E_HIP, "%s: the mask changed during the call (%u selected, then %u)", who, m, again);
        return GSR_OK;
    }
};

extern "C" int64_t gsr_debug_stage_bytes(gsr_context* c)
{
    if (!c) return (int64_t)set_err(GSR_E_INVALID, "gsr_debug_stage_bytes: ctx is NULL");
    return (int64_t)c->stage.cap();
}

extern "C" int gsr_get_duplicate(gsr_context* c, int64_t* calls, int64_t* copied_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_duplicate: ctx is NULL");
    return c->dup.report(calls, copied_last, ms);
}

// A copy of each selected splat appended.  A move whose source is a multiset: the compaction leaves the n + m positions and the slot
// each of them is carried from (a copy: its original's), the ordering of an upload runs over them, k_repack writes the spare planes at
// the capacity gsr_add's policy gives, the swap.  The steps around that are add_body's.
extern "C" int gsr_duplicate(gsr_context* c, const uint32_t* mask, int mask_is_device, int64_t* m_out, int64_t* n_total)
{
    const char* const who = "gsr_duplicate";
    if (!c) return set_err(GSR_E_INVALID, "gsr_duplicate: ctx is NULL");
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const uint32_t n0 = c->n;
    HIP_TRY(hipSetDevice(c->device));
    const CopySelection s(MaskArg{mask, mask_is_device != 0, n0});
    if ((rc = s.mask.check(c, who))) return rc;
    Reorder ro(c, who, false);
    if ((rc = sync_all(c))) return rc;   // the public stream (a producer of a device mask queued there has finished), and no write under a frame in flight
    auto nothing = [&]() {             // nothing is selected: no resident bit changes, nothing is invalidated
        if (m_out) *m_out = 0;
        if (n_total) *n_total = (int64_t)n0;
        return GSR_OK;
    };
    if (n0 == 0) return nothing();
    hipStream_t us = ro.us;
    // ---- 1, 2. which splats are copied, and how many: nothing resident is written yet
    if ((rc = s.prepare(c, who)) || (rc = ro.old_inverse(true))) return rc;
    HIP_TRY(hipEventRecord(c->up_ev[0], us));
    uint32_t m = 0;
    HIP_TRY(s.count(c, us, &m, &ro.link_ms));
    if (m > n0) return set_err(GSR_E_HIP, "gsr_duplicate: the scan counted %u selected of %u splats", m, n0);
    if (m == 0) return nothing();
    if ((int64_t)n0 + (int64_t)m > 0x7fffffffll) return set_err(GSR_E_INVALID, "gsr_duplicate: %u + %u splats are more than a context holds", n0, m);
    const uint32_t n1 = n0 + m, nclus1 = div_up(n1, GSR_CLUSTER);
    const uint32_t cap0 = c->cap, cap1 = (uint32_t)gsr_add_capacity((int64_t)cap0, (int64_t)n1);
    const bool grow = cap1 != cap0;
    const bool vis = c->vis_on;
    // ---- everything the rest needs, before the first write to resident memory or to the visibility's state (add_body's list)
    size_t off = s.bytes;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oRows = place((size_t)m * 4), oP = place((size_t)n1 * 12), oSlot = place((size_t)n1 * 4);
    if ((rc = s.grow(c, us, off, m, who))) return rc;
    if ((rc = ro.prepare(n1))) return rc;
    if (grow) {
        free_spare_planes(c);
        if ((rc = ensure_spare_planes(c, cap1, false))) return rc;
        for (int k = 0; k < GSR_MAX_SLOTS; ++k)
            if ((rc = alloc_splat_arrays(ro.slot_new[k], cap1))) {
                free_spare_planes(c);
                return rc;
            }
    } else if ((rc = ensure_spare_planes(c, cap0, true))) {
        return rc;
    }
    if ((rc = ro.clusA_new.alloc(nclus1)) || (rc = ro.clusB_new.alloc(nclus1))) return rc;
    if (vis) {
        if ((rc = vis_ensure_buffers(c))) return rc;
        if (grow && (rc = ro.alpha0_new.alloc((size_t)cap1))) return rc;
        if (c->vis_mask && (rc = ro.mask_new.alloc(((size_t)n1 + 31) / 32))) return rc;
    }
    // nothing can fail for lack of memory any more: the larger buffers take their places (none of them holds anything a frame keeps)
    c->clusA2 = std::move(ro.clusA_new); c->clusB2 = std::move(ro.clusB_new);
    if (grow) {
        for (int k = 0; k < GSR_MAX_SLOTS; ++k) slot_take_splat_arrays(c->slot[k], std::move(ro.slot_new[k]));
        c->alpha0_2.reset();
        if (!vis) c->alpha0.reset();
    }
    // ---- from here on a failure leaves no geometry
    ro.spare_outgrown = grow;
    // 3. every position of the larger cloud in upload order, the slot each splat is carried from, the copies' true alphas
    uint32_t* const rows = reinterpret_cast<uint32_t*>(c->stage + oRows);
    float* const Pall = reinterpret_cast<float*>(c->stage + oP);
    uint32_t* const src_slot = reinterpret_cast<uint32_t*>(c->stage + oSlot);
    float* const a0 = !vis ? (float*)nullptr : grow ? (float*)ro.alpha0_new : (float*)c->alpha0;
    hipError_t e = hipSuccess;
    if (vis && grow) e = hipMemcpyAsync(a0, c->alpha0, (size_t)n0 * 4, hipMemcpyDeviceToDevice, us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_compact<true>), dim3(s.nblocks), dim3(GSR_REMOVE_THREADS), 0, us, n0, s.sel(c), s.offsets(c), rows, ro.inv_old, c->geoA,
                           Pall, src_slot, vis ? (const float*)c->alpha0 : (const float*)nullptr, a0);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return ro.lost(e);
    // 4. the ordering of an upload over all of them, and the planes into the spare set: k_repack as a move runs it, with the slot list in
    // the place of the old order's inverse and the spare planes' own capacity
    if ((rc = ro.order(Pall, n1))) return ro.lost(rc);
    e = queue_repack(c, us, n1, ro.perm_new, src_slot, cap1);
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[2], us);
    // ... and the mask of a visibility in force, extended by clear bits
    if (e == hipSuccess && ro.mask_new) {
        const uint32_t words1 = (uint32_t)(((size_t)n1 + 31) / 32);
        hipLaunchKernelGGL(k_add_mask_extend, dim3(div_up(words1, 256)), dim3(256), 0, us, n0, words1, c->vis_mask, ro.mask_new);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return ro.lost(e);
    // 5. the swap; what becomes the spare set goes as after an add
    ro.commit(n1, nclus1, true);
    c->clusA2.reset(); c->clusB2.reset();
    if (grow) {
        free_spare_planes(c);
        c->cap = cap1;
        if (vis) c->alpha0 = std::move(ro.alpha0_new);
    }
    // 6, 7. the rule of a visibility in force over the whole cloud; a new cloud to everything a frame keeps
    if ((rc = ro.finish(c->dup.ms, false))) return rc;
    c->dup.calls += 1;
    c->dup.last = (int64_t)m;
    if (grow) c->add_grows += 1;
    if (m_out) *m_out = (int64_t)m;
    if (n_total) *n_total = (int64_t)n1;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Transform (k_transform.h): selected resident splats rotated, scaled and translated where they are.  A move whose new
// positions, shapes and SH rows are formed on the GPU from the resident ones: k_transform in the place of k_move_positions, then
// reposition_body as gsr_move runs it.
static_assert(sizeof(gsr_xform_rule) == sizeof(GsrXformRule) && offsetof(gsr_xform_rule, t) == offsetof(GsrXformRule, t) &&
              offsetof(gsr_xform_rule, s) == offsetof(GsrXformRule, s) && offsetof(gsr_xform_rule, q) == offsetof(GsrXformRule, q) &&
              offsetof(gsr_xform_rule, D1) == offsetof(GsrXformRule, D1) && offsetof(gsr_xform_rule, D2) == offsetof(GsrXformRule, D2) &&
              offsetof(gsr_xform_rule, D3) == offsetof(GsrXformRule, D3), "gsr_xform_rule is the kernel's rule");

// Y_l(d), l = 1..3, in double: the 2l + 1 polynomials gsr_shade_sh (k_preprocess.h) multiplies band l's coefficients with, its float32
// constants and its signs included
static void xform_sh_basis(int l, const double d[3], double* y)
{
    const double x = d[0], yy_ = d[1], z = d[2];
    const double xx = x * x, yy = yy_ * yy_, zz = z * z, xy = x * yy_, yz = yy_ * z, xz = x * z;
    if (l == 1) {
        const double C1 = 0.4886025f;
        y[0] = -C1 * yy_; y[1] = C1 * z; y[2] = -C1 * x;
    } else if (l == 2) {
        const double C0 = 1.0925484f, C1 = -1.0925484f, C2 = 0.3153916f, C3 = -1.0925484f, C4 = 0.5462742f;
        y[0] = C0 * xy; y[1] = C1 * yz; y[2] = C2 * (2.0 * zz - xx - yy); y[3] = C3 * xz; y[4] = C4 * (xx - yy);
    } else {
        const double C0 = -0.5900436f, C1 = 2.8906114f, C2 = -0.4570458f, C3 = 0.3731763f, C4 = -0.4570458f, C5 = 1.4453057f, C6 = -0.5900436f;
        y[0] = C0 * yy_ * (3.0 * xx - yy); y[1] = C1 * xy * z; y[2] = C2 * yy_ * (4.0 * zz - xx - yy);
        y[3] = C3 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy); y[4] = C4 * x * (4.0 * zz - xx - yy); y[5] = C5 * z * (xx - yy);
        y[6] = C6 * x * (xx - 3.0 * yy);
    }
}

// D_l with Y_l(R d)^T D_l = Y_l(d)^T for every unit d, by a linear solve over N = 2l + 1 fixed sample directions e_i built from those
// same polynomials (so the sign conventions are right by construction): with d = R^T e the condition reads Y_l(e)^T D_l = Y_l(R^T e)^T,
// i.e. B D = C with the rows B_i = Y_l(e_i), C_i = Y_l(R^T e_i).  Solved as D = I + B^-1 (C - B): the correction is exactly zero where R
// is the identity, without a special case.  The e_i spiral down the sphere off any symmetry (cond(B) < 8 in every band).  Gaussian
// elimination with partial pivoting, double.
static void xform_band_matrix(int l, const double R[9], float* D)
{
    const int N = 2 * l + 1;
    double B[7][7], X[7][7];
    for (int i = 0; i < N; ++i) {
        const double th = 0.4 + 2.2 * (double)i / (double)N, ph = (double)i * 2.399963229728653;
        const double e[3] = {std::sin(th) * std::cos(ph), std::sin(th) * std::sin(ph), std::cos(th)};
        const double re[3] = {R[0] * e[0] + R[3] * e[1] + R[6] * e[2], R[1] * e[0] + R[4] * e[1] + R[7] * e[2], R[2] * e[0] + R[5] * e[1] + R[8] * e[2]};   // R^T e
        double c[7];
        xform_sh_basis(l, e, B[i]);
        xform_sh_basis(l, re, c);
        for (int k = 0; k < N; ++k) X[i][k] = c[k] - B[i][k];
    }
    for (int k = 0; k < N; ++k) {
        int p = k;
        for (int i = k + 1; i < N; ++i) if (std::fabs(B[i][k]) > std::fabs(B[p][k])) p = i;
        if (p != k) for (int j = 0; j < N; ++j) { std::swap(B[k][j], B[p][j]); std::swap(X[k][j], X[p][j]); }
        for (int i = k + 1; i < N; ++i) {
            const double f = B[i][k] / B[k][k];
            for (int j = k; j < N; ++j) B[i][j] -= f * B[k][j];
            for (int j = 0; j < N; ++j) X[i][j] -= f * X[k][j];
        }
    }
    for (int i = N - 1; i >= 0; --i)
        for (int j = 0; j < N; ++j) {
            double v = X[i][j];
            for (int k = i + 1; k < N; ++k) v -= B[i][k] * X[k][j];
            X[i][j] = v / B[i][i];
        }
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) D[i * N + j] = (float)((i == j ? 1.0 : 0.0) + X[i][j]);
}

// what is wrong with the caller's transform (NULL: nothing)
static const char* xform_error(const gsr_xform* x)
{
    const float* f = x->rotate;        // rotate[4], scale, translate[3], pivot[3]: eleven floats in a row
    static_assert(offsetof(gsr_xform, reserved_) == 11 * sizeof(float), "gsr_xform begins with eleven floats");
    for (int k = 0; k < 11; ++k) if (!std::isfinite(f[k])) return "a field is not finite";
    if (!(x->scale > 0.0f)) return "scale is not > 0";
    if (x->rotate[0] == 0.0f && x->rotate[1] == 0.0f && x->rotate[2] == 0.0f && x->rotate[3] == 0.0f) return "the quaternion is zero";
    if (x->reserved_ != 0) return "reserved_ is not 0";
    return nullptr;
}
static GsrXformRule xform_rule(const gsr_xform* x)
{
    GsrXformRule r{};
    const double qx = x->rotate[0], qy = x->rotate[1], qz = x->rotate[2], qw = x->rotate[3];
    const double len = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    const double i = qx / len, j = qy / len, k = qz / len, w = qw / len, s = x->scale;
    const double R[9] = {1.0 - 2.0 * (j * j + k * k), 2.0 * (i * j - w * k), 2.0 * (i * k + w * j),
                         2.0 * (i * j + w * k), 1.0 - 2.0 * (i * i + k * k), 2.0 * (j * k - w * i),
                         2.0 * (i * k - w * j), 2.0 * (j * k + w * i), 1.0 - 2.0 * (i * i + j * j)};
    for (int e = 0; e < 9; ++e) r.A[e] = (float)(s * R[e]);
    for (int a = 0; a < 3; ++a) {
        const double sRp = s * R[3 * a] * (double)x->pivot[0] + s * R[3 * a + 1] * (double)x->pivot[1] + s * R[3 * a + 2] * (double)x->pivot[2];
        r.t[a] = (float)((double)x->pivot[a] + (double)x->translate[a] - sRp);
    }
    r.s = x->scale;
    r.q[0] = (float)i; r.q[1] = (float)j; r.q[2] = (float)k; r.q[3] = (float)w;
    xform_band_matrix(1, R, r.D1);
    xform_band_matrix(2, R, r.D2);
    xform_band_matrix(3, R, r.D3);
    return r;
}

extern "C" int gsr_xform_prepare(const gsr_xform* x, gsr_xform_rule* rule)
{
    if (!x || !rule) return set_err(GSR_E_INVALID, "gsr_xform_prepare: NULL argument");
    const char* bad = xform_error(x);
    if (bad) return set_err(GSR_E_INVALID, "gsr_xform_prepare: %s", bad);
    const GsrXformRule r = xform_rule(x);
    std::memcpy(rule, &r, sizeof(r));
    return GSR_OK;
}

extern "C" int gsr_transform_eval(const gsr_xform* x, int64_t n, const uint32_t* mask, float* P, uint16_t* scale, uint16_t* orient,
                                  uint16_t* shx, uint16_t* shy, uint16_t* shz)
{
    if (!x) return set_err(GSR_E_INVALID, "gsr_transform_eval: x is NULL");
    const char* bad = xform_error(x);
    if (bad) return set_err(GSR_E_INVALID, "gsr_transform_eval: %s", bad);
    if (n < 0 || n > 0x7fffffffll || (n > 0 && (!P || !scale || !orient))) return set_err(GSR_E_INVALID, "gsr_transform_eval: bad argument");
    const int nsh = (shx ? 1 : 0) + (shy ? 1 : 0) + (shz ? 1 : 0);
    if (nsh != 0 && nsh != 3) return set_err(GSR_E_INVALID, "gsr_transform_eval: the three SH arrays come together or not at all");
    const GsrXformRule r = xform_rule(x);
    uint16_t* const sh[3] = {shx, shy, shz};
    for (int64_t i = 0; i < n; ++i) {
        if (mask && !((mask[i >> 5] >> (i & 31)) & 1u)) continue;
        float* p = P + 3 * i;
        const float px = p[0], py = p[1], pz = p[2];
        for (int a = 0; a < 3; ++a) p[a] = gsr_xf_position(r, a, px, py, pz);
        uint16_t* s = scale + 3 * i;
        for (int k = 0; k < 3; ++k) s[k] = gsr_xf_scale(r, s[k]);
        uint16_t* o = orient + 4 * i;
        gsr_xf_orient(r, o[0], o[1], o[2], o[3]);
        if (nsh)
            for (int ch = 0; ch < 3; ++ch)
                for (int part = 0; part < 2; ++part) gsr_xf_sh_part(r, part, sh[ch] + 16 * i);
    }
    return GSR_OK;
}

extern "C" int gsr_get_transform(gsr_context* c, int64_t* calls, int64_t* moved_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_transform: ctx is NULL");
    return c->xf.report(calls, moved_last, ms);
}

extern "C" int gsr_transform(gsr_context* c, const uint32_t* mask, int mask_is_device, const gsr_xform* x, int64_t* n_moved)
{
    const char* const who = "gsr_transform";
    if (!c || !x) return set_err(GSR_E_INVALID, "gsr_transform: NULL argument");
    const char* bad = xform_error(x);
    if (bad) return set_err(GSR_E_INVALID, "gsr_transform: %s", bad);
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const uint32_t n = c->n;
    const MaskArg mk{mask, mask_is_device != 0, n};
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = mk.check(c, who))) return rc;
    if (n == 0) {                      // the empty cloud: no word of the mask exists
        rc = sync_all(c);
        if (rc) return rc;
        c->xf.calls += 1; c->xf.last = 0;
        if (n_moved) *n_moved = 0;
        return GSR_OK;
    }
    const GsrXformRule rule = xform_rule(x);
    // ---- the arena: every position in upload order, the rule, the count, a host mask's copy
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t oP = place((size_t)n * 12), oRule = place(sizeof(GsrXformRule)), oCount = place(4), oMask = place(mk.stage_bytes());
    if ((rc = ensure_h_word(c, who))) return rc;
    const uint32_t* dmask = nullptr;
    uint32_t count = n;
    rc = reposition_body(c, who, off, nullptr, c->xf.ms, false,
        [&](Reorder& ro, bool* nothing) {
            // the rule and a host mask into the arena (no resident byte), then the count: a mask with no bit set below n ends the call here
            hipStream_t us = ro.us;
            const double t0 = up_now_ms();
            HIP_TRY(hipMemcpyAsync(c->stage + oRule, &rule, sizeof(rule), hipMemcpyHostToDevice, us));
            HIP_TRY(mk.to_device(c, us, oMask, nullptr, &dmask));
            if (!mk.stage_bytes()) HIP_TRY(hipStreamSynchronize(us));      // (to_device has waited for a host mask, the rule with it)
            ro.link_ms = up_now_ms() - t0;
            const int counted = dmask ? count_mask_bits(c, us, n, dmask, oCount, who, &count) : GSR_OK;
            *nothing = count == 0;
            return counted;
        },
        [&](Reorder& ro, const float** Pout) {
            float* const Pup = reinterpret_cast<float*>(c->stage + oP);
            hipError_t e = hipEventRecord(c->up_ev[0], ro.us);
            if (e == hipSuccess) {
                launch_sh(c->has_sh, [&](auto sh) {
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_transform<decltype(sh)::value>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, ro.us, n, c->cap, dmask,
                                       reinterpret_cast<const GsrXformRule*>(c->stage + oRule), ro.inv_old, c->geoA, c->geoB, c->col, c->colrow, Pup);
                });
                e = hipGetLastError();
            }
            if (e != hipSuccess) return ro.lost(e);
            *Pout = Pup;
            return GSR_OK;
        });
    if (rc) return rc;
    c->xf.calls += 1;
    c->xf.last = (int64_t)count;
    if (n_moved) *n_moved = (int64_t)count;
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Grade (k_grade.h): the colour and the opacity of selected resident splats changed where they are.  An update whose
// new Cd, SH and alpha are formed on the GPU from the resident ones: k_grade in the place of k_update, then gsr_update's invalidation.
// No position changes: the storage order, the cluster bounds and the spare planes are not touched.
static_assert(sizeof(gsr_grade_rule) == sizeof(GsrGradeRule) && offsetof(gsr_grade_rule, M) == offsetof(GsrGradeRule, M) &&
              offsetof(gsr_grade_rule, b) == offsetof(GsrGradeRule, b) && offsetof(gsr_grade_rule, ag) == offsetof(GsrGradeRule, ag) &&
              offsetof(gsr_grade_rule, ab) == offsetof(GsrGradeRule, ab) && offsetof(gsr_grade_rule, flags) == offsetof(GsrGradeRule, flags) &&
              GSR_GRADE_COLOUR == GSR_GRADEF_COLOUR && GSR_GRADE_ALPHA == GSR_GRADEF_ALPHA, "gsr_grade_rule is the kernel's rule");

// what is wrong with the caller's rule (NULL: nothing)
static const char* grade_rule_error(const gsr_grade_rule* r)
{
    const float* f = r->M;             // M[9], b[3], ag, ab: fourteen floats in a row
    static_assert(offsetof(gsr_grade_rule, flags) == 14 * sizeof(float), "gsr_grade_rule begins with fourteen floats");
    for (int k = 0; k < 14; ++k) if (!std::isfinite(f[k])) return "a float of the rule is not finite";
    if (r->flags & ~(GSR_GRADE_COLOUR | GSR_GRADE_ALPHA)) return "unknown flag bit";
    return nullptr;
}

extern "C" int gsr_grade_prepare(const gsr_grade_params* p, gsr_grade_rule* rule)
{
    if (!p || !rule) return set_err(GSR_E_INVALID, "gsr_grade_prepare: NULL argument");
    const float* f = &p->exposure;     // exposure, gain[3], saturation, contrast, pivot, offset[3], alpha_gain, alpha_offset: twelve floats in a row
    static_assert(sizeof(gsr_grade_params) == 12 * sizeof(float) && offsetof(gsr_grade_params, alpha_offset) == 11 * sizeof(float), "gsr_grade_params is twelve floats");
    for (int k = 0; k < 12; ++k) if (!std::isfinite(f[k])) return set_err(GSR_E_INVALID, "gsr_grade_prepare: a field is not finite");
    // c1 = 2^exposure gain o c;  c2 = L + saturation (c1 - L), L = w . c1;  c3 = contrast (c2 - pivot) + pivot + offset -- in double
    const double w[3] = {0.2126, 0.7152, 0.0722};
    const double ex = std::exp2((double)p->exposure), sat = p->saturation, con = p->contrast;
    gsr_grade_rule r{};
    for (int row = 0; row < 3; ++row) {
        for (int k = 0; k < 3; ++k) r.M[3 * row + k] = (float)(con * ((row == k ? sat : 0.0) + (1.0 - sat) * w[k]) * (ex * (double)p->gain[k]));
        r.b[row] = (float)((double)p->pivot * (1.0 - con) + (double)p->offset[row]);
    }
    r.ag = p->alpha_gain;
    r.ab = p->alpha_offset;
    bool identity = true;
    for (int k = 0; k < 9; ++k) identity = identity && r.M[k] == ((k % 4 == 0) ? 1.0f : 0.0f);
    for (int k = 0; k < 3; ++k) identity = identity && r.b[k] == 0.0f;
    r.flags = (identity ? 0u : GSR_GRADE_COLOUR) | ((r.ag == 1.0f && r.ab == 0.0f) ? 0u : GSR_GRADE_ALPHA);
    const char* bad = grade_rule_error(&r);
    if (bad) return set_err(GSR_E_INVALID, "gsr_grade_prepare: the parameters overflow float32: %s", bad);
    *rule = r;
    return GSR_OK;
}

static GsrGradeRule grade_kernel_rule(const gsr_grade_rule* rule)
{
    GsrGradeRule g;
    std::memcpy(&g, rule, sizeof(g));
    return g;
}

extern "C" int gsr_grade_eval(const gsr_grade_rule* rule, int64_t n, const uint32_t* mask, int has_sh, uint16_t* Cd, float* alpha,
                              uint16_t* shx, uint16_t* shy, uint16_t* shz)
{
    if (!rule) return set_err(GSR_E_INVALID, "gsr_grade_eval: rule is NULL");
    const char* bad = grade_rule_error(rule);
    if (bad) return set_err(GSR_E_INVALID, "gsr_grade_eval: %s", bad);
    const bool colour = rule->flags & GSR_GRADE_COLOUR, alph = rule->flags & GSR_GRADE_ALPHA;
    if (n < 0 || n > 0x7fffffffll || (n > 0 && ((colour && !Cd) || (alph && !alpha) || (colour && has_sh && (!shx || !shy || !shz)))))
        return set_err(GSR_E_INVALID, "gsr_grade_eval: bad argument");
    const GsrGradeRule g = grade_kernel_rule(rule);
    for (int64_t i = 0; i < n; ++i) {
        if (mask && !((mask[i >> 5] >> (i & 31)) & 1u)) continue;
        if (alph) alpha[i] = gsr_grade_alpha(g, alpha[i]);
        if (!colour) continue;
        uint16_t* c = Cd + 3 * i;
        const uint16_t cr = c[0], cg = c[1], cb = c[2];
        for (int r = 0; r < 3; ++r) c[r] = gsr_grade_half(g, r, true, cr, cg, cb);
        if (!has_sh) continue;
        uint16_t* const row[3] = {shx + 16 * i, shy + 16 * i, shz + 16 * i};
        for (int s = 0; s < 15; ++s) {                 // (slot 15 stays)
            const uint16_t hr = row[0][s], hg = row[1][s], hb = row[2][s];
            for (int r = 0; r < 3; ++r) row[r][s] = gsr_grade_half(g, r, false, hr, hg, hb);
        }
    }
    return GSR_OK;
}

extern "C" int gsr_get_grade(gsr_context* c, int64_t* calls, int64_t* graded_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_grade: ctx is NULL");
    return c->gr.report(calls, graded_last, ms);
}

extern "C" int gsr_grade(gsr_context* c, const uint32_t* mask, int mask_is_device, const gsr_grade_rule* rule, int64_t* n_graded)
{
    const char* const who = "gsr_grade";
    if (!c || !rule) return set_err(GSR_E_INVALID, "gsr_grade: NULL argument");
    const char* bad = grade_rule_error(rule);
    if (bad) return set_err(GSR_E_INVALID, "gsr_grade: %s", bad);
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    const double t_begin = up_now_ms();
    const uint32_t n = c->n;
    const MaskArg mk{mask, mask_is_device != 0, n};
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = mk.check(c, who))) return rc;
    if ((rc = sync_all(c))) return rc;      // the public stream (a select queued there has written the mask), and no in-place write under a frame in flight
    auto nothing = [&]() {                  // empty work: a call that changes, invalidates and writes nothing
        c->gr.calls += 1; c->gr.last = 0;
        if (n_graded) *n_graded = 0;
        return GSR_OK;
    };
    if (n == 0 || !rule->flags) return nothing();
    const GsrGradeRule g = grade_kernel_rule(rule);
    const bool alph = g.flags & GSR_GRADEF_ALPHA, vis = c->vis_on && alph;
    // ---- everything the call needs, before the first write: the arena (the count, a host mask's copy), the inverse of the storage
    // order, the clock's events, the pinned word of the count, the visibility's buffers
    const size_t oCount = 0, oMask = 256;
    hipStream_t us = c->slot[0].own;
    if ((rc = ensure_stage(c, oMask + pad256(mk.stage_bytes()))) || (rc = ensure_inverse_perm(c)) ||
        (rc = ensure_up_events(c, 2, who, true)) || (vis && (rc = vis_ensure_buffers(c))) || (rc = ensure_h_word(c, who))) return rc;
    // ---- a host mask into the arena (no resident byte), then the count: a mask with no bit set below n ends the call here
    const uint32_t* dmask = nullptr;
    uint32_t count = n;
    HIP_TRY(mk.to_device(c, us, oMask, nullptr, &dmask));
    if (dmask && (rc = count_mask_bits(c, us, n, dmask, oCount, who, &count))) return rc;
    if (count == 0) return nothing();
    const double t_counted = up_now_ms();
    // ---- the kernel, in place; with a visibility in force and a new opacity, the rule in force over the graded true alphas (no
    // capture: the hidden splats' resident zeros never reach alpha0); then gsr_update's invalidation
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    hipError_t e = hipEventRecord(c->up_ev[0], us);
    double t_kernel = t_counted;
    if (e == hipSuccess) {
        launch_sh(c->has_sh, [&](auto sh) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grade<decltype(sh)::value>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, us, n, c->cap, dmask, g, inv,
                               c->geoA, c->col, c->has_sh ? c->colrow : (uint4*)nullptr, vis ? c->alpha0 : (float*)nullptr);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(c->up_ev[1], us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    t_kernel = up_now_ms();
    if (e == hipSuccess && vis) e = vis_apply(c, us, 0u, 0u, true, c->vis, c->vis_mask, nullptr);
    const double t_vis = up_now_ms();
    e = after_update(c, alph, us, e);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_grade: %s", hipGetErrorString(e));
    float ms = 0.0f;
    c->gr.ms[0] = t_counted - t_begin;
    c->gr.ms[1] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->gr.ms[2] = vis ? t_vis - t_kernel : 0.0;
    c->gr.ms[3] = up_now_ms() - t_begin;
    c->gr.calls += 1;
    c->gr.last = (int64_t)count;
    if (n_graded) *n_graded = (int64_t)count;
    return GSR_OK;
}
