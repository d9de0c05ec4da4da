// k_marks.h -- the selection overlay (gsr_render_marks): the splats a mask selects, drawn into a finished frame as
// centre dots or as the outlines of their +-2 quads, nearest first.
//
// Nothing here restates a rule.  A dot's centre, clip test and opacity test are gsr_select_hit's (k_select.h) -- so a radius-0 dot lies
// on the pixel gsr_select looks at -- an outline is gsr_wire_splat's (k_wire.h), fragment for fragment what k_wire_splats emits, and the
// resolve step decodes, composites and stores through the functions k_blend_over does (gsr_device.h).  Both shapes go through the wire
// overlay's 64-bit z-buffer: atomicMin of (bits(zw) << 32) | upload index, so the nearest fragment wins and the lower upload index on
// equal depth, whatever order the waves run in.  No frame kernel changes, and a context that never draws marks launches nothing of this
// file.  No LDS, no scratch.
#pragma once
#include "gsr_device.h"
#include "k_select.h"
#include "k_wire.h"

#define GSR_MARKK_DOT      1           // = GSR_MARK_DOT
#define GSR_MARKK_OUTLINE  2           // = GSR_MARK_OUTLINE
#define GSR_MARKC_FIXED    0           // = GSR_MARK_COLOUR_FIXED
#define GSR_MARKC_CD       1           // = GSR_MARK_COLOUR_CD
#define GSR_MARK_THREADS   256

// the constants a shape's kernel takes by value: a dot needs the selection rule's 41 dwords, an outline the frame (the covariance)
template <int SHAPE> struct GsrMarkConsts;
template <> struct GsrMarkConsts<GSR_MARKK_DOT> { typedef GsrSelectRule type; };
template <> struct GsrMarkConsts<GSR_MARKK_OUTLINE> { typedef GsrFrame type; };

// the fragments of one dot: the square of pixels around the centre's, clipped to the image (the caller has looked: the centre lies
// inside it, so qx and qy are pixels of it)
__device__ __forceinline__ void gsr_mark_dot(float cx, float cy, int radius, int width, int height, unsigned long long frag,
                                             unsigned long long* __restrict__ zbuf)
{
    const int qx = (int)cx, qy = (int)cy;
    const int x0 = qx - radius > 0 ? qx - radius : 0, x1 = qx + radius < width - 1 ? qx + radius : width - 1;
    const int y0 = qy - radius > 0 ? qy - radius : 0, y1 = qy + radius < height - 1 ? qy + radius : height - 1;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) atomicMin(&zbuf[(size_t)y * (size_t)width + (size_t)x], frag);
}

// One thread per UPLOAD index i, in k_select's shape.  The wave's two mask words are uniform: loaded once per wave, never at or behind
// ceil(n / 32) (mask = NULL: every splat).  A wave none of whose splats is selected leaves on one ballot, before any gather: a sparse
// selection costs a pass over the mask.  The lanes that stay gather geoA[inv[i]] (inv: upload index -> storage slot; NULL: upload
// order), an outline geoB[inv[i]] too, and send their fragments into the z-buffer.
// rule: the selection rule with the rect (-inf, -inf, +inf, +inf) and GSR_SELF_ANY_OPACITY as the style says (DOT), or the frame
// (OUTLINE); any_opacity: OUTLINE's opacity test dropped; radius: DOT's.
template <int SHAPE>
__global__ void __launch_bounds__(GSR_MARK_THREADS)
k_mark(uint32_t n, const uint32_t* __restrict__ mask /* NULL: every splat */, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA,
       const uint4* __restrict__ geoB, typename GsrMarkConsts<SHAPE>::type rule, int any_opacity, int radius,
       unsigned long long* __restrict__ zbuf)
{
    const uint32_t i = blockIdx.x * (uint32_t)GSR_MARK_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((i - lane) >> 5)), words = (n >> 5) + ((n & 31u) ? 1u : 0u);
    uint32_t lo = ~0u, hi = ~0u;
    if (mask) {
        lo = w0 < words ? mask[w0] : 0u;
        hi = w0 + 1u < words ? mask[w0 + 1u] : 0u;
    }
    const bool marked = i < n && (((lane < 32u ? lo : hi) >> (lane & 31u)) & 1u);
    if (!__ballot(marked)) return;                     // nothing of this wave is selected: no gather
    if (!marked) return;
    const uint32_t slot = inv ? inv[i] : i;
    const float4 a = geoA[slot];
    if constexpr (SHAPE == GSR_MARKK_DOT) {
        float centre[3];
        if (!gsr_select_hit(rule, a.x, a.y, a.z, a.w, nullptr, nullptr, centre)) return;
        const float cx = centre[0], cy = centre[1];
        if (!(cx >= 0.0f && cx < rule.W && cy >= 0.0f && cy < rule.H)) return;
        const unsigned long long frag = ((unsigned long long)__builtin_bit_cast(uint32_t, centre[2]) << 32) | (unsigned long long)i;
        gsr_mark_dot(cx, cy, radius, rule.width, rule.height, frag, zbuf);
    } else {
        if (!any_opacity && !(a.w >= (1.0f / 255.0f))) return;   // the RESIDENT opacity: +0.0f for a splat a visibility hides
        gsr_wire_splat(rule, a, geoB[slot], i, nullptr, zbuf);
    }
}

// One thread per pixel: the winner (zw, i) of the z-buffer, if any, against the depth buffer (zw <= depth[p] + bias: one f32 add, one
// compare -- the winner has the smallest zw of the pixel's fragments, so testing it is the per-fragment test), then colour c over the
// decoded target pixel D, out = fmaf(1 - c.a, D, c) per channel, stored by the target format's store.  Every other pixel keeps its
// bytes.  A wave's written pixels leave as ONE 64-bit vector atomic from its first lane into the workgroup's counter slot (k_select's
// scheme); the host adds the slots up.  Plain vector stores only.
__global__ void __launch_bounds__(GSR_MARK_THREADS)
k_mark_resolve(const unsigned long long* __restrict__ zbuf, size_t npix, const uint4* __restrict__ col0,
               const uint32_t* __restrict__ inv /* upload index -> storage slot, or NULL */, int colour_mode, float4 fixed,
               const float* __restrict__ depth /* NULL: no test */, float depth_bias, void* target /* read and written: npix pixels */,
               int format, unsigned long long* __restrict__ counters)
{
    const size_t p = (size_t)blockIdx.x * (size_t)GSR_MARK_THREADS + threadIdx.x;
    const unsigned long long v = p < npix ? zbuf[p] : GSR_WIRE_EMPTY;
    bool write = v != GSR_WIRE_EMPTY;
    if (write && depth) {
        const float zw = __builtin_bit_cast(float, (uint32_t)(v >> 32));
        write = zw <= depth[p] + depth_bias;
    }
    if (write) {
        float4 c = fixed;
        if (colour_mode == GSR_MARKC_CD) {
            const uint32_t idx = (uint32_t)(v & 0xffffffffull);
            const uint4 h = col0[inv ? inv[idx] : idx];           // chunk 0 starts with Cd.rgb (f16), as k_wire_resolve reads it
            c = make_float4(gsr_h2f(h.x & 0xffffu), gsr_h2f(h.x >> 16), gsr_h2f(h.y & 0xffffu), 1.0f);
        }
        const float4 o = gsr_composite_over_pixel(gsr_background_pixel(target, format, p), c);
        if (format == GSR_FMT_RGBA32F) reinterpret_cast<float4*>(target)[p] = o;
        else gsr_store_packed(target, format, p, o.x, o.y, o.z, o.w);
    }
    const unsigned long long wrote = (unsigned long long)__popcll(__ballot(write));   // (every lane of the wave is here: nobody has left)
    if ((threadIdx.x & 63u) == 0u && wrote)
        atomicAdd(counters + (size_t)(blockIdx.x & (GSR_SEL_COUNTER_SLOTS - 1u)) * GSR_SEL_COUNTER_STRIDE, wrote);
}
