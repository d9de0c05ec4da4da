// k_select_attrs.h -- resident splats selected by what they are (gsr_select_attrs): opacity, size, needles, base colour,
// crop volumes.
//
// THE rule, in one place: gsr_attr_hit is __host__ __device__, as gsr_select_hit and gsr_splat_visible are; k_select_attrs and
// gsr_select_attrs_eval (host) both go through it.  The only arithmetic is the half -> float conversion (exact on both sides), one f32
// multiply (the anisotropy clause) and the volumes' explicit fmaf chains (gsr_volume_inside; the translation units are compiled with
// -ffp-contract=off): x86 and gfx950 agree in every bit.  Every comparison is written so that a NaN operand means "no hit" -- never
// through fmaxf / fminf, which drop a NaN.  No frame kernel changes, and a context that never selects by attribute launches nothing
// of this file.
#pragma once
#include "k_select.h"

// the clauses and flags of gsplat_hip.h (GSR_ATTR_*; gsr_resident_select.h holds the two sets equal)
#define GSR_ATTRC_ALPHA       1
#define GSR_ATTRC_SCALE_MAX   2
#define GSR_ATTRC_SCALE_MIN   4
#define GSR_ATTRC_ANISOTROPY  8
#define GSR_ATTRC_COLOUR     16
#define GSR_ATTRC_VOLUME     32
#define GSR_ATTRC_ALL        63
#define GSR_ATTRC_SCALES     (GSR_ATTRC_SCALE_MAX | GSR_ATTRC_SCALE_MIN | GSR_ATTRC_ANISOTROPY)
#define GSR_ATTRF_SKIP_HIDDEN 1

// gsr_attr_rule's layout (by value in the kernel's argument segment: uniform, read through the scalar cache where it is used)
struct GsrAttrRule {
    int32_t clauses, flags, op, n_volumes;
    float alpha_lo, alpha_hi, smax_lo, smax_hi, smin_lo, smin_hi, anisotropy;
    float colour_lo[3], colour_hi[3];
    int32_t reserved_;
    GsrVisVolume vol[GSR_VIS_VOLUMES];
};
static_assert(sizeof(GsrAttrRule) == 74 * 4, "the rule is a run of 74 dwords");

__host__ __device__ __forceinline__ float gsr_attr_h2f(uint32_t bits16)
{
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);      // exact (v_cvt_f32_f16 on the device)
}
// lo <= x <= hi, false for a NaN anywhere (lo > hi: false)
__host__ __device__ __forceinline__ bool gsr_attr_in(float lo, float x, float hi) { return lo <= x && x <= hi; }

// Is a splat hit?  (px, py, pz): the raw position bits, what geoA holds; a: its TRUE alpha; s0..s2: the resident scale halves; c0..c2:
// the resident Cd halves; hidden: the visibility in force hides it (false without one).  What no set clause looks at is not read.
__host__ __device__ __forceinline__ bool gsr_attr_hit(const GsrAttrRule& r, float px, float py, float pz, float a, uint32_t s0, uint32_t s1,
                                                      uint32_t s2, uint32_t c0, uint32_t c1, uint32_t c2, bool hidden)
{
    const int cl = r.clauses;
    if ((r.flags & GSR_ATTRF_SKIP_HIDDEN) && hidden) return false;
    if ((cl & GSR_ATTRC_ALPHA) && !gsr_attr_in(r.alpha_lo, a, r.alpha_hi)) return false;
    if (cl & GSR_ATTRC_SCALES) {
        const float a0 = __builtin_fabsf(gsr_attr_h2f(s0)), a1 = __builtin_fabsf(gsr_attr_h2f(s1)), a2 = __builtin_fabsf(gsr_attr_h2f(s2));
        if (!(a0 == a0 && a1 == a1 && a2 == a2)) return false;          // a NaN half: no scale clause passes
        const float hi01 = a0 > a1 ? a0 : a1, lo01 = a0 < a1 ? a0 : a1;
        const float smax = hi01 > a2 ? hi01 : a2, smin = lo01 < a2 ? lo01 : a2;
        if ((cl & GSR_ATTRC_SCALE_MAX) && !gsr_attr_in(r.smax_lo, smax, r.smax_hi)) return false;
        if ((cl & GSR_ATTRC_SCALE_MIN) && !gsr_attr_in(r.smin_lo, smin, r.smin_hi)) return false;
        if ((cl & GSR_ATTRC_ANISOTROPY) && !(smax > 0.0f && smax >= r.anisotropy * smin)) return false;
    }
    if ((cl & GSR_ATTRC_COLOUR) && !(gsr_attr_in(r.colour_lo[0], gsr_attr_h2f(c0), r.colour_hi[0]) &&
                                     gsr_attr_in(r.colour_lo[1], gsr_attr_h2f(c1), r.colour_hi[1]) &&
                                     gsr_attr_in(r.colour_lo[2], gsr_attr_h2f(c2), r.colour_hi[2])))
        return false;
    if (cl & GSR_ATTRC_VOLUME) {
        if (!(px == px && py == py && pz == pz)) return false;         // (an inverted volume would pass a NaN position: "not inside")
        for (int k = 0; k < r.n_volumes; ++k)
            if (gsr_volume_inside(r.vol[k], px, py, pz) == (r.vol[k].invert != 0)) return false;
    }
    return true;
}

// What a lane loads: the host derives it from the clauses and the visibility in force; uniform, so every load below sits behind a
// scalar branch and an alpha-only rule gathers what k_select gathers (one 16-byte geoA row), or reads alpha0 alone.
#define GSR_ATTRL_GEOA    1            // geoA[j]: P (volumes, hidden) and, without a visibility in force, the alpha
#define GSR_ATTRL_GEOB    2            // geoB[j]: the scale halves
#define GSR_ATTRL_COL     4            // col[j], chunk 0: the Cd halves
#define GSR_ATTRL_ALPHA0  8            // alpha0[i]: the TRUE alpha under a visibility in force (upload order: coalesced)
#define GSR_ATTRL_HIDDEN 16            // the visibility's rule and its mask word of i (SKIP_HIDDEN with a visibility in force)

// One thread per UPLOAD index i, k_select's shape: slot j = inv[i] (inv: upload index -> storage slot; NULL: upload order), the loads
// `loads` names (each a 16-byte gather, or 4 bytes of alpha0 / the visibility mask), the rule, and k_select's epilogue
// (gsr_select_epilogue: one ballot, the two mask words of lanes 0 and 32 with plain vector stores, the slotted counts).  No LDS, no
// barrier, no atomic on the mask.
__global__ void __launch_bounds__(GSR_SELECT_THREADS)
k_select_attrs(uint32_t n, int loads, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA, const uint4* __restrict__ geoB,
               const uint4* __restrict__ col, const float* __restrict__ alpha0, const uint32_t* __restrict__ vis_mask /* NULL: none */,
               GsrAttrRule rule, GsrVisRule vis, uint32_t* __restrict__ mask, unsigned long long* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * (uint32_t)GSR_SELECT_THREADS + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const bool gathers = (loads & (GSR_ATTRL_GEOA | GSR_ATTRL_GEOB | GSR_ATTRL_COL)) != 0;
        const uint32_t j = gathers && inv ? inv[i] : i;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint4 b = make_uint4(0u, 0u, 0u, 0u), c = make_uint4(0u, 0u, 0u, 0u);
        if (loads & GSR_ATTRL_GEOA) a = geoA[j];
        if (loads & GSR_ATTRL_GEOB) b = geoB[j];
        if (loads & GSR_ATTRL_COL) c = col[j];
        const float alpha = (loads & GSR_ATTRL_ALPHA0) ? alpha0[i] : a.w;
        const bool hidden = (loads & GSR_ATTRL_HIDDEN) && !gsr_splat_visible(vis, a.x, a.y, a.z, vis_mask ? vis_mask[i >> 5] : 0u, i);
        hit = gsr_attr_hit(rule, a.x, a.y, a.z, alpha, b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, c.x & 0xffffu, c.x >> 16, c.y & 0xffffu, hidden);
    }
    gsr_select_epilogue(n, i, hit, rule.op, mask, counters);
}
