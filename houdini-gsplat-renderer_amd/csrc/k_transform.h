// k_transform.h -- selected resident splats rotated, scaled and translated in place (gsr_transform).
//
// A similarity x = (rotate q, uniform scale s, translate, pivot) is BAKED into the resident planes of the splats a bit mask selects:
// p' = s R (p - pivot) + pivot + translate.  gsr_xform_prepare derives the float32 rule below from x in double, once per call; the
// per-splat arithmetic is written once, as __host__ __device__ functions, and is evaluated by the kernel and by gsr_transform_eval
// (host) alike.  Every multiply-add is an explicit fmaf and no product feeds an add anywhere else (the translation units are compiled
// with -ffp-contract=off), conversions between half and float are the IEEE ones (half -> float exact, float -> half to nearest even):
// x86 and gfx950 agree in every bit that is not a NaN's sign or payload.  No frame kernel changes, and a context that never transforms
// launches nothing of this file.
//
// THE RULE -- this comment is the normative statement of each chain.  For a splat whose mask bit is set:
//   P       raw position bits (x, y, z); for each axis r = 0, 1, 2
//             P'.r = fmaf(A[3r], x, fmaf(A[3r+1], y, fmaf(A[3r+2], z, t[r])))
//   scale   each of the three halves: scale'_k = f2h(s * h2f(scale_k))                                 (one float32 product)
//   orient  o = (b_i, b_j, b_k, b_r) = h2f of the four resident halves AS THEY ARE (unnormalised, as K1 uses them); with the rule's unit
//           quaternion q = (a_i, a_j, a_k, a_r) the product q (x) o, the transform first; each component one product under three fmaf:
//             i' = f2h(fmaf(a_r, b_i, fmaf(a_i, b_r, fmaf(a_j, b_k, (-a_k) * b_j))))
//             j' = f2h(fmaf(a_r, b_j, fmaf(a_j, b_r, fmaf(a_k, b_i, (-a_i) * b_k))))
//             k' = f2h(fmaf(a_r, b_k, fmaf(a_k, b_r, fmaf(a_i, b_j, (-a_j) * b_i))))
//             r' = f2h(fmaf(a_r, b_r, fmaf(-a_i, b_i, fmaf(-a_j, b_j, (-a_k) * b_k))))
//           R(q (x) o) = R(q) R(o) holds for quaternions of any length, so the splat's axes turn with the transform and its length
//           |o| stays (up to the rounding to halves).  For a non-unit orient this is what a Transform SOP does to the attribute; it is
//           NOT an exact rotation of the matrix K1 forms from the unnormalised orient, which is not a rotation to begin with.
//   SH      per channel (x, y, z rows) and per band l = 1, 2, 3 with the 2l + 1 coefficients c_0 .. c_2l of the band (slots 0..2, 3..7,
//           8..14 of the channel's 16-half row: gsr_shade_sh's sh[0..2], sh[3..7], sh[8..14]), D = D_l, rows of 2l + 1:
//             c'_m = f2h(fmaf(D[m][2l], h2f(c_2l), .. fmaf(D[m][1], h2f(c_1), D[m][0] * h2f(c_0)) ..))   (k ascending, the product first)
//           slot 15 of a row, Cd and alpha stay as they are; a cloud without SH has no SH step.
// A splat whose bit is clear keeps every bit.  NaN and infinite inputs follow the arithmetic; a half that comes out NaN is a NaN on
// both sides, sign and payload unspecified.
#pragma once
#include "k_resident.h"

// what gsr_xform_prepare derives (= gsr_xform_rule of the public header): 100 dwords.  Too many for scalar registers beside a kernel's
// pointers (k_select.h notes where that limit lies), so the kernel reads them through a uniform pointer to a small device buffer
// the host fills in front of the launch: scalar loads, each D row fetched where its band is computed.
struct GsrXformRule {
    float A[9];                        // fl32(s R), rows
    float t[3];                        // fl32(pivot + translate - (s R) pivot)
    float s;                           // fl32(scale)
    float q[4];                        // the unit quaternion (i, j, k, r)
    float D1[9], D2[25], D3[49];       // the SH band matrices, rows
};
static_assert(sizeof(GsrXformRule) == 100 * 4, "the rule is a run of 100 dwords");

__host__ __device__ __forceinline__ float gsr_xf_h2f(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }    // exact
__host__ __device__ __forceinline__ uint16_t gsr_xf_f2h(float f)
{
    const _Float16 h = (_Float16)f;    // round to nearest even, overflow to infinity
    return __builtin_bit_cast(uint16_t, h);
}

__host__ __device__ __forceinline__ float gsr_xf_position(const GsrXformRule& r, int axis, float x, float y, float z)
{
    const float* a = r.A + 3 * axis;
    return __builtin_fmaf(a[0], x, __builtin_fmaf(a[1], y, __builtin_fmaf(a[2], z, r.t[axis])));
}
__host__ __device__ __forceinline__ uint16_t gsr_xf_scale(const GsrXformRule& r, uint16_t h) { return gsr_xf_f2h(r.s * gsr_xf_h2f(h)); }
// o[4]: the resident orient halves (i, j, k, r), replaced by those of q (x) o
__host__ __device__ __forceinline__ void gsr_xf_orient(const GsrXformRule& r, uint16_t& o0, uint16_t& o1, uint16_t& o2, uint16_t& o3)
{
    const float ai = r.q[0], aj = r.q[1], ak = r.q[2], ar = r.q[3];
    const float bi = gsr_xf_h2f(o0), bj = gsr_xf_h2f(o1), bk = gsr_xf_h2f(o2), br = gsr_xf_h2f(o3);
    o0 = gsr_xf_f2h(__builtin_fmaf(ar, bi, __builtin_fmaf(ai, br, __builtin_fmaf(aj, bk, (-ak) * bj))));
    o1 = gsr_xf_f2h(__builtin_fmaf(ar, bj, __builtin_fmaf(aj, br, __builtin_fmaf(ak, bi, (-ai) * bk))));
    o2 = gsr_xf_f2h(__builtin_fmaf(ar, bk, __builtin_fmaf(ak, br, __builtin_fmaf(ai, bj, (-aj) * bi))));
    o3 = gsr_xf_f2h(__builtin_fmaf(ar, br, __builtin_fmaf(-ai, bi, __builtin_fmaf(-aj, bj, (-ak) * bk))));
}
// one band of one channel: c[0 .. N) (N = 2l + 1 halves, contiguous) replaced by D c
template <int N>
__host__ __device__ __forceinline__ void gsr_xf_band(const float* __restrict__ D, uint16_t* c)
{
    float v[N];
    uint16_t out[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = gsr_xf_h2f(c[k]);
#pragma unroll
    for (int m = 0; m < N; ++m) {
        float acc = D[m * N] * v[0];
#pragma unroll
        for (int k = 1; k < N; ++k) acc = __builtin_fmaf(D[m * N + k], v[k], acc);
        out[m] = gsr_xf_f2h(acc);
    }
#pragma unroll
    for (int m = 0; m < N; ++m) c[m] = out[m];
}
// the two halves of a channel's 16-half row, as the kernel's lanes split them: part 0 = bands 1 and 2 (slots 0..7), part 1 = band 3
// (slots 8..14; slot 15 stays)
__host__ __device__ __forceinline__ void gsr_xf_sh_part(const GsrXformRule& r, int part, uint16_t* row16)
{
    if (part == 0) {
        gsr_xf_band<3>(r.D1, row16);
        gsr_xf_band<5>(r.D2, row16 + 3);
    } else {
        gsr_xf_band<7>(r.D3, row16 + 8);
    }
}

// K0t: the rule over the resident planes, in k_update's / k_unpack's work shape (k_resident.h): 512 threads cover 64 consecutive UPLOAD
// indices i, eight lanes per splat, all eight in one wave; storage slot j = inv[i] (inv: the inverse of the storage order in force;
// NULL: j = i).  A wave covers eight splats, whose mask bits lie in ONE word: it reads that word once, and for a group of eight with no
// bit set only lane 0's copy below runs.
//   q = 0      loads geoA[j]; selected: P' with 4-byte stores into geoA[j].xyz and, with SH, into piece 0 of colrow[j] (.w, the opacity,
//              stays).  EVERY splat, selected or not: its position goes to Pup[3 i ..], the cloud's positions in upload order, which
//              the ordering of an upload reads afterwards (k_move_positions' job, folded in)
//   q = 7      selected: gsr_shape_split(geoB[j]), the scale and orient rules, gsr_shape_join -- the extent half is derived by the
//              one function every kernel derives it by
//   q = 1..6   SH and selected: piece q of colrow[j] (colour chunk q - 1) into the splat's LDS row x[16] y[16] z[16] Cd[3] by
//              gsr_colour_half_slot (k_unpack's inverse transpose); behind gsr_wave_lds_sync() lane q owns channel (q - 1) >> 1, part
//              (q - 1) & 1 of the row -- eight halves nobody else reads or writes now -- and replaces them by gsr_xf_sh_part; behind
//              a second sync it takes gsr_colour_chunk<true>(row, q - 1) and stores it to col[q - 1][j] (chunks strided by the
//              capacity) and to colrow[j][q]
// The syncs sit in code only whole splats skip (wave barriers, not workgroup barriers), nothing is atomic, and a slot is written by
// the lanes of its own splat only: the result does not depend on the order the waves run in.  Without SH the kernel has no LDS.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_transform(uint32_t n, uint32_t cap, const uint32_t* __restrict__ mask /* NULL: every splat */, const GsrXformRule* __restrict__ rule,
            const uint32_t* __restrict__ inv, float4* __restrict__ geoA, uint4* __restrict__ geoB, uint4* __restrict__ col,
            uint4* __restrict__ colrow, float* __restrict__ Pup)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = 64 upload indices, eight lanes per splat");
    __shared__ __attribute__((aligned(16))) uint16_t s_h[SH ? GSR_CLUSTER : 1][GSR_ROW_HALVES];
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t i = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    if (i >= n) return;                // (whole splats leave: the lanes that meet at the wave barriers below are those that stay)
    const uint32_t i0 = i & ~7u;       // the wave's first splat: bits [i0 & 31, (i0 & 31) + 8) of word i0 >> 5
    const uint32_t group = mask ? ((uint32_t)__builtin_amdgcn_readfirstlane((int)mask[i0 >> 5]) >> (i0 & 31u)) & 0xffu : 0xffu;
    const bool selected = (group >> (i & 7u)) & 1u;
    const uint32_t j = inv ? inv[i] : i;
    if (q == 0) {
        const float4 a = geoA[j];
        float px = a.x, py = a.y, pz = a.z;
        if (selected) {
            px = gsr_xf_position(*rule, 0, a.x, a.y, a.z);
            py = gsr_xf_position(*rule, 1, a.x, a.y, a.z);
            pz = gsr_xf_position(*rule, 2, a.x, a.y, a.z);
            float* g = reinterpret_cast<float*>(geoA + j);
            g[0] = px; g[1] = py; g[2] = pz;
            if (SH) {
                float* r = reinterpret_cast<float*>(colrow + (size_t)j * 8);
                r[0] = px; r[1] = py; r[2] = pz;
            }
        }
        float* o = Pup + 3 * (size_t)i;
        o[0] = px; o[1] = py; o[2] = pz;
    }
    if (group == 0u) return;           // (wave-uniform: nothing of these eight splats changes)
    if (q == 7 && selected) {
        GsrShape h = gsr_shape_split(geoB[j]);
        h.s0 = gsr_xf_scale(*rule, h.s0); h.s1 = gsr_xf_scale(*rule, h.s1); h.s2 = gsr_xf_scale(*rule, h.s2);
        gsr_xf_orient(*rule, h.o0, h.o1, h.o2, h.o3);
        geoB[j] = gsr_shape_join(h);
    }
    if constexpr (SH) {
        const bool colour = selected && q >= 1 && q <= 6;
        uint16_t* const row = s_h[sp];
        if (colour) {
            const uint4 piece = colrow[(size_t)j * 8 + q];
            const uint32_t w[4] = {piece.x, piece.y, piece.z, piece.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) row[gsr_colour_half_slot(q - 1, k)] = (k & 1) ? gsr_hi16(w[k >> 1]) : gsr_lo16(w[k >> 1]);
        }
        gsr_wave_lds_sync();
        if (colour) gsr_xf_sh_part(*rule, (q - 1) & 1, row + 16 * ((q - 1) >> 1));
        gsr_wave_lds_sync();
        if (colour) {
            const uint4 v = gsr_colour_chunk<true>(row, q - 1);
            col[(size_t)(q - 1) * cap + j] = v;
            colrow[(size_t)j * 8 + q] = v;
        }
    }
}
