// gsr_resident_read.h -- the verbs that read the resident cloud back in UPLOAD order: gsr_read_info, gsr_read,
// gsr_read_device, gsr_get_read, and over a mask in the place of a range gsr_read_masked, gsr_read_masked_device.  Host code only; included once, behind gsr_resident_edit.h, whose refusals (refuse_edit,
// refuse_range) and pointer check (check_device_source) it shares.  The kernel is k_unpack (k_read.h).
//
// A read writes NOTHING the context keeps: no resident bit, no horizon, no cached order, no policy, no visibility state, no entry of
// gsr_stats.  It therefore does not wait for the frames in flight (they only read the planes too), and the next frame runs the
// launches it would have run.  What it uses of the context: slot 0's own stream, the first two events of the upload clock, the
// inverse of the storage order (built on first use per geometry, as gsr_update builds it) and -- the host form -- the staging arena,
// which is idle because an upload in progress is refused.
#pragma once

extern "C" int gsr_read_info(gsr_context* c, int64_t* n_splats, int* has_sh, float origin[3])
{
    const int rc = refuse_edit(c, "gsr_read_info");
    if (rc) return rc;
    if (n_splats) *n_splats = (int64_t)c->n;
    if (has_sh) *has_sh = c->has_sh ? 1 : 0;
    if (origin) for (int k = 0; k < 3; ++k) origin[k] = c->origin[k];
    return GSR_OK;
}

extern "C" int gsr_get_read(gsr_context* c, int64_t* reads, int64_t* rows_last, double ms[4])
{
    if (!c) return set_err(GSR_E_INVALID, "gsr_get_read: ctx is NULL");
    return c->rd.report(reads, rows_last, ms);
}

// k_unpack over rows [first, first + n) on slot 0's own stream, between up_ev[0] and up_ev[1]; the caller has ensured the inverse of
// the storage order and the events, and waits for the stream.  rows (device memory, n upload indices; NULL: none): the row list of a
// masked read in the place of the range; its caller has recorded up_ev[0] in front of the compaction that wrote the list.
template <bool F32>
static hipError_t queue_unpack(gsr_context* c, hipStream_t us, uint32_t first, uint32_t n, const GsrReadDst<F32>& dst, const uint32_t* rows = nullptr)
{
    const uint32_t* const inv = c->perm ? c->wire_inv : (const uint32_t*)nullptr;
    const float* const alpha0 = c->vis_on ? c->alpha0 : (const float*)nullptr;       // (a visibility in force: geoA holds +0.0f for the hidden)
    hipError_t e = rows ? hipSuccess : hipEventRecord(c->up_ev[0], us);
    if (e != hipSuccess) return e;
    launch_sh(c->has_sh, [&](auto sh) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_unpack<decltype(sh)::value, F32>), dim3(div_up(n, GSR_CLUSTER)), dim3(GSR_PACK_THREADS), 0, us, first, n, dst, inv,
                           c->geoA, c->geoB, c->col, c->colrow, alpha0, rows);
    });
    e = hipGetLastError();
    return e == hipSuccess ? hipEventRecord(c->up_ev[1], us) : e;
}

// the call's entries of gsr_get_read, once the destinations are complete
static void read_done(gsr_context* c, int64_t rows, double copy_ms, double t_begin)
{
    float ms = 0.0f;
    c->rd.ms[0] = hipEventElapsedTime(&ms, c->up_ev[0], c->up_ev[1]) == hipSuccess ? (double)ms : 0.0;
    c->rd.ms[1] = copy_ms;
    c->rd.ms[2] = 0.0;
    c->rd.ms[3] = up_now_ms() - t_begin;
    c->rd.calls += 1;
    c->rd.last = rows;
}

// ---------------------------------------------------------------------------
// The host form: k_unpack into device rows in gsr_upload_append's layout (the staging arena: 256-byte aligned sections, one per array
// that is wanted, sized for the range), then one device -> host copy per array.
extern "C" int gsr_read(gsr_context* c, int64_t first, int64_t n64, const gsr_read_arrays* out)
{
    const char* const who = "gsr_read";
    if (!c || !out) return set_err(GSR_E_INVALID, "gsr_read: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    const int nsh = (out->shx ? 1 : 0) + (out->shy ? 1 : 0) + (out->shz ? 1 : 0);
    if (nsh != 0 && nsh != 3) return set_err(GSR_E_INVALID, "gsr_read: the three SH arrays come together or not at all");
    if (nsh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_read: SH arrays for a cloud uploaded without SH");
    if (n64 == 0 || !(out->P || out->Cd || out->alpha || out->scale || out->orient || nsh)) return GSR_OK;
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)n64;
    // ---- everything the call needs, before the launch
    void* const host[8] = {out->P, out->alpha, out->Cd, out->scale, out->orient, out->shx, out->shy, out->shz};
    const size_t row[8] = {12, 4, 6, 6, 8, 32, 32, 32};
    size_t at[8], bytes = 0;
    for (int k = 0; k < 8; ++k) { at[k] = bytes; if (host[k]) bytes += pad256(n * row[k]); }
    if ((rc = ensure_stage(c, bytes)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    char* d[8];
    for (int k = 0; k < 8; ++k) d[k] = host[k] ? c->stage + at[k] : nullptr;
    auto f32 = [&](int k) { return reinterpret_cast<float*>(d[k]); };
    auto h16 = [&](int k) { return reinterpret_cast<uint16_t*>(d[k]); };
    const GsrReadDst<false> dst{f32(0), f32(1), h16(2), h16(3), h16(4), h16(5), h16(6), h16(7)};
    hipStream_t us = c->slot[0].own;
    hipError_t e = queue_unpack(c, us, (uint32_t)first, (uint32_t)n, dst);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    const double t0 = up_now_ms();
    for (int k = 0; k < 8; ++k)
        if (host[k] && e == hipSuccess) e = hipMemcpyAsync(host[k], d[k], n * row[k], hipMemcpyDeviceToHost, us);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_read: %s", hipGetErrorString(e));
    read_done(c, n64, up_now_ms() - t0, t_begin);
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// The device form: k_unpack writes the caller's float32 arrays where they are; nothing is staged and nothing crosses the link.
extern "C" int gsr_read_device(gsr_context* c, int64_t first, int64_t n64, const gsr_device_out* out)
{
    const char* const who = "gsr_read_device";
    if (!c || !out) return set_err(GSR_E_INVALID, "gsr_read_device: NULL argument");
    int rc = GSR_OK;
    if ((rc = refuse_edit(c, who)) || (rc = refuse_range(c, first, n64, who))) return rc;
    if (out->reserved_ != 0) return set_err(GSR_E_INVALID, "gsr_read_device: reserved_ is not 0");
    if (out->sh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_read_device: sh for a cloud uploaded without SH");
    if (out->sh && (out->sh_vec3_per_point < 1 || out->sh_vec3_per_point > 16))
        return set_err(GSR_E_INVALID, "gsr_read_device: sh_vec3_per_point = %d is not within 1..16", out->sh_vec3_per_point);
    if (n64 == 0 || !(out->P || out->Cd || out->alpha || out->scale || out->orient || out->sh)) return GSR_OK;
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)n64;
    // every destination, before anything is launched: a wrong pointer must never be found out by a kernel
    auto look = [&](const float* p, size_t floats_per_row, const char* name) {
        if (p && !rc) rc = check_device_source(c, p, n * floats_per_row * 4, who, name);
    };
    look(out->P, 3, "P"); look(out->Cd, 3, "Cd"); look(out->alpha, 1, "alpha"); look(out->scale, 3, "scale"); look(out->orient, 4, "orient");
    look(out->sh, out->sh ? (size_t)out->sh_vec3_per_point * 3 : 0, "sh");
    if (rc) return rc;
    if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));     // a consumer of the destinations queued on the public stream has finished
    if ((rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    const GsrReadDst<true> dst{out->P, out->alpha, out->Cd, out->scale, out->orient, out->sh, out->sh ? out->sh_vec3_per_point : 0};
    hipStream_t us = c->slot[0].own;
    hipError_t e = queue_unpack(c, us, (uint32_t)first, (uint32_t)n, dst);
    if (e == hipSuccess) e = hipStreamSynchronize(us);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "gsr_read_device: %s", hipGetErrorString(e));
    read_done(c, n64, 0.0 /* nothing crossed the link */, t_begin);
    return GSR_OK;
}

// ---------------------------------------------------------------------------
// Reading by a mask (k_copy.h): gsr_remove's compaction, the selected splats in the survivors' place, writes the row
// list k_unpack then reads.  Both forms share everything up to the destinations: the refusals, the count (mark, scan, one word over the
// link), max_rows, and the row list behind the selection's scratch in the staging arena.
//   wanted                   whether the caller's struct names a destination (none: the call is a count); wait_public: the device form
//   check()                  the device destinations' pointer check for max_rows rows, before anything is launched
//   out_bytes(m)             what the form stages of m rows in the arena, behind the row list
//   unpack(us, m, rows, arena behind the row list, &copy_ms)   k_unpack and the copies; complete on return
template <class Check, class Bytes, class Unpack>
static int read_masked_body(gsr_context* c, const char* who, const uint32_t* mask, int mask_is_device, int64_t max_rows, bool wanted, bool wait_public,
                            int64_t* m_out, Check&& check, Bytes&& out_bytes, Unpack&& unpack)
{
    if (wanted && max_rows < 0) return set_err(GSR_E_INVALID, "%s: max_rows = %lld", who, (long long)max_rows);
    const uint32_t n = c->n;
    const double t_begin = up_now_ms();
    HIP_TRY(hipSetDevice(c->device));
    const MaskArg mk{mask, mask_is_device != 0, n};
    const CopySelection s(mk);
    int rc = GSR_OK;
    if ((rc = mk.check(c, who))) return rc;
    if (wanted && (rc = check())) return rc;
    if (n == 0) {                                      // the empty cloud selects no row
        if (m_out) *m_out = 0;
        return GSR_OK;
    }
    // a producer of a device mask, or a consumer of device destinations, queued on the public stream has finished
    if (c->stream && (wait_public || (mask && mk.is_device))) HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = s.prepare(c, who)) || (rc = ensure_inverse_perm(c)) || (rc = ensure_up_events(c, 2, who, true))) return rc;
    hipStream_t us = c->slot[0].own;
    uint32_t m = 0;
    HIP_TRY(s.count(c, us, &m, nullptr));
    if (m > n) return set_err(GSR_E_HIP, "%s: the scan counted %u selected of %u splats", who, m, n);
    if (m_out) *m_out = (int64_t)m;
    if (!wanted) return GSR_OK;                        // a count
    if ((int64_t)m > max_rows) return set_err(GSR_E_INVALID, "%s: the selection holds %u rows, the destinations %lld", who, m, (long long)max_rows);
    if (m == 0) return GSR_OK;
    const size_t oRows = s.bytes, oOut = oRows + pad256((size_t)m * 4);
    if ((rc = s.grow(c, us, oOut + out_bytes((size_t)m), m, who))) return rc;
    uint32_t* const rows = reinterpret_cast<uint32_t*>(c->stage + oRows);
    hipError_t e = hipEventRecord(c->up_ev[0], us);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_compact<false>), dim3(s.nblocks), dim3(GSR_REMOVE_THREADS), 0, us, n, s.sel(c), s.offsets(c), rows, (const uint32_t*)nullptr,
                           (const float4*)nullptr, (float*)nullptr, (uint32_t*)nullptr, (const float*)nullptr, (float*)nullptr);
        e = hipGetLastError();
    }
    double copy_ms = 0.0;
    if (e == hipSuccess) e = unpack(us, m, rows, c->stage + oOut, &copy_ms);
    if (e != hipSuccess) return set_err(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    read_done(c, (int64_t)m, copy_ms, t_begin);
    return GSR_OK;
}

extern "C" int gsr_read_masked(gsr_context* c, const uint32_t* mask, int mask_is_device, int64_t max_rows, const gsr_read_arrays* out, int64_t* m_out)
{
    const char* const who = "gsr_read_masked";
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    static const gsr_read_arrays none{};
    if (!out) out = &none;
    const int nsh = (out->shx ? 1 : 0) + (out->shy ? 1 : 0) + (out->shz ? 1 : 0);
    if (nsh != 0 && nsh != 3) return set_err(GSR_E_INVALID, "gsr_read_masked: the three SH arrays come together or not at all");
    if (nsh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_read_masked: SH arrays for a cloud uploaded without SH");
    const bool wanted = out->P || out->Cd || out->alpha || out->scale || out->orient || nsh;
    void* const host[8] = {out->P, out->alpha, out->Cd, out->scale, out->orient, out->shx, out->shy, out->shz};
    const size_t row[8] = {12, 4, 6, 6, 8, 32, 32, 32};
    size_t at[8];
    return read_masked_body(c, who, mask, mask_is_device, max_rows, wanted, false, m_out,
        []() { return GSR_OK; },
        [&](size_t m) {                                // device rows in gsr_upload_append's layout, one section per array that is wanted
            size_t bytes = 0;
            for (int k = 0; k < 8; ++k) { at[k] = bytes; if (host[k]) bytes += pad256(m * row[k]); }
            return bytes;
        },
        [&](hipStream_t us, uint32_t m, const uint32_t* rows, char* arena, double* copy_ms) {
            char* d[8];
            for (int k = 0; k < 8; ++k) d[k] = host[k] ? arena + at[k] : nullptr;
            auto f32 = [&](int k) { return reinterpret_cast<float*>(d[k]); };
            auto h16 = [&](int k) { return reinterpret_cast<uint16_t*>(d[k]); };
            const GsrReadDst<false> dst{f32(0), f32(1), h16(2), h16(3), h16(4), h16(5), h16(6), h16(7)};
            hipError_t e = queue_unpack(c, us, 0u, m, dst, rows);
            if (e == hipSuccess) e = hipStreamSynchronize(us);
            const double t0 = up_now_ms();
            for (int k = 0; k < 8; ++k)
                if (host[k] && e == hipSuccess) e = hipMemcpyAsync(host[k], d[k], (size_t)m * row[k], hipMemcpyDeviceToHost, us);
            if (e == hipSuccess) e = hipStreamSynchronize(us);
            *copy_ms = up_now_ms() - t0;
            return e;
        });
}

extern "C" int gsr_read_masked_device(gsr_context* c, const uint32_t* mask, int mask_is_device, int64_t max_rows, const gsr_device_out* out, int64_t* m_out)
{
    const char* const who = "gsr_read_masked_device";
    int rc = refuse_edit(c, who);
    if (rc) return rc;
    static const gsr_device_out none{};
    if (!out) out = &none;
    if (out->reserved_ != 0) return set_err(GSR_E_INVALID, "gsr_read_masked_device: reserved_ is not 0");
    if (out->sh && !c->has_sh) return set_err(GSR_E_INVALID, "gsr_read_masked_device: sh for a cloud uploaded without SH");
    if (out->sh && (out->sh_vec3_per_point < 1 || out->sh_vec3_per_point > 16))
        return set_err(GSR_E_INVALID, "gsr_read_masked_device: sh_vec3_per_point = %d is not within 1..16", out->sh_vec3_per_point);
    const bool wanted = out->P || out->Cd || out->alpha || out->scale || out->orient || out->sh;
    return read_masked_body(c, who, mask, mask_is_device, max_rows, wanted, true, m_out,
        [&]() {                                        // every destination for max_rows rows: a wrong pointer must never be found out by a kernel
            int bad = GSR_OK;
            auto look = [&](const float* p, size_t floats_per_row, const char* name) {
                if (p && !bad) bad = check_device_source(c, p, (size_t)max_rows * floats_per_row * 4, who, name);
            };
            look(out->P, 3, "P"); look(out->Cd, 3, "Cd"); look(out->alpha, 1, "alpha"); look(out->scale, 3, "scale"); look(out->orient, 4, "orient");
            look(out->sh, out->sh ? (size_t)out->sh_vec3_per_point * 3 : 0, "sh");
            return bad;
        },
        [](size_t) { return (size_t)0; },              // k_unpack writes the caller's arrays where they are
        [&](hipStream_t us, uint32_t m, const uint32_t* rows, char*, double*) {
            const GsrReadDst<true> dst{out->P, out->alpha, out->Cd, out->scale, out->orient, out->sh, out->sh ? out->sh_vec3_per_point : 0};
            hipError_t e = queue_unpack(c, us, 0u, m, dst, rows);
            if (e == hipSuccess) e = hipStreamSynchronize(us);
            return e;
        });
}
