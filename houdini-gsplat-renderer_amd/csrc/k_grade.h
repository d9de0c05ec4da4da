// k_grade.h -- selected resident splats graded in place: an affine colour map and an opacity map (gsr_grade).
//
// The vertex stage forms max(Cd + sum_k Y_k(d) sh_k, 0) per channel (gsr_splat_colour, k_preprocess.h): linear in (Cd, sh_1 .. sh_15)
// in front of the clamp.  So the affine colour map c' = M c + b is BAKED exactly, from every view direction, by Cd' = M Cd + b and
// sh_k' = M sh_k for every coefficient k: the map mixes only the three channels of ONE coefficient, and the resident order of the 48
// colour halves (half h = 3 * coefficient + channel, k_resident.h) keeps those three side by side.  gsr_grade_prepare derives the rule
// below from what a user turns (exposure, gain, saturation, contrast, offset, the opacity's gain and offset) in double, once; the
// per-splat arithmetic is written once, as __host__ __device__ functions, and is evaluated by the kernel and by gsr_grade_eval (host)
// alike.  Every multiply-add is an explicit fmaf and no product feeds an add anywhere else (the translation units are compiled with
// -ffp-contract=off), conversions between half and float are gsr_xf_h2f / gsr_xf_f2h (k_transform.h: the IEEE ones): x86 and gfx950
// agree in every bit that is not a NaN's sign or payload.  No frame kernel changes, and a context that never grades launches nothing of
// this file.
//
// THE RULE -- this comment is the normative statement of each chain.  For a splat whose mask bit is set, (R, G, B) = h2f of the three
// halves of ONE coefficient as they are resident, r = 0, 1, 2 the channel that comes out, M in rows:
//   GSR_GRADE_COLOUR set:
//     Cd               Cd'_r = f2h(fmaf(M[3r], R, fmaf(M[3r+1], G, fmaf(M[3r+2], B, b[r]))))
//     SH 1..15         sh'_r = f2h(fmaf(M[3r], R, fmaf(M[3r+1], G, M[3r+2] * B)))                       (the product first, no b)
//                      slot 15 of an shx / shy / shz row (host arrays; the resident layout does not hold it) stays as it is; a cloud
//                      without SH has only the Cd step, and the zero halves beside Cd in chunk 0 stay +0
//   GSR_GRADE_ALPHA set:
//     alpha            v = fmaf(ag, alpha, ab);  alpha' = fminf(fmaxf(v, 0), 1), the two written as comparisons -- v > 0 ? v : +0, then
//                      v < 1 ? v : 1 -- so that a NaN becomes +0 and a zero comes out +0 on every machine.  alpha is the TRUE alpha:
//                      with a visibility in force the one kept aside, not the +0 a hidden splat holds
// A step whose flag is clear does not run AT ALL: a rule without flags is a no-op.  A splat whose bit is clear keeps every bit.
// Non-finite halves follow the arithmetic; a half that comes out NaN is NaN on both sides, sign and payload unspecified.
// THE IDENTITY IS NOT A NO-OP of the colour step: under M = I, b = 0 a -0 half becomes +0 (fmaf(1, -0, +0) = +0 under the Cd chain,
// and the zero products of the other two channels are +0 in both chains), and an infinite half turns its two neighbours NaN
// (0 * inf).  That is why gsr_grade_prepare clears GSR_GRADE_COLOUR for the identity instead of running it.
#pragma once
#include "k_resident.h"
#include "k_transform.h"

#define GSR_GRADEF_COLOUR 1u           // = GSR_GRADE_COLOUR
#define GSR_GRADEF_ALPHA 2u            // = GSR_GRADE_ALPHA

// what gsr_grade_prepare derives (= gsr_grade_rule of the public header): 15 dwords, by value in the kernel's argument segment --
// uniform, in scalar registers beside six pointers (k_select.h notes where that limit lies: its 41 dwords fit)
struct GsrGradeRule {
    float M[9];                        // rows
    float b[3];
    float ag, ab;
    uint32_t flags;                    // GSR_GRADEF_*
};
static_assert(sizeof(GsrGradeRule) == 15 * 4, "the rule is a run of 15 dwords");

// channel r of one graded coefficient from its three halves; with_b: the coefficient is Cd
__host__ __device__ __forceinline__ uint16_t gsr_grade_half(const GsrGradeRule& g, int r, bool with_b, uint16_t hr, uint16_t hg, uint16_t hb)
{
    const float* m = g.M + 3 * r;
    const float R = gsr_xf_h2f(hr), G = gsr_xf_h2f(hg), B = gsr_xf_h2f(hb);
    const float tail = with_b ? __builtin_fmaf(m[2], B, g.b[r]) : m[2] * B;
    float v = __builtin_fmaf(m[0], R, __builtin_fmaf(m[1], G, tail));
#if defined(__HIP_DEVICE_COMPILE__)
    // The chain ends in a float32, and THAT is rounded to a half.  Left alone, the compiler folds the last fmaf and the conversion of
    // some outputs into v_fma_mixlo_f16, and those halves came out one step off the host's in a few per cent of the cases (contrast
    // 1.3: 7 of 357 splats' first halves): the empty statement keeps the float32 a value of its own, so the conversion is
    // v_cvt_f16_f32 / v_cvt_pk_f16_f32 of the rounded sum on every path.
    asm("" : "+v"(v));
#endif
    return gsr_xf_f2h(v);
}
__host__ __device__ __forceinline__ float gsr_grade_alpha(const GsrGradeRule& g, float alpha)
{
    float v = __builtin_fmaf(g.ag, alpha, g.ab);
    v = v > 0.0f ? v : 0.0f;           // fmaxf(v, 0): NaN -> +0, -0 -> +0
    return v < 1.0f ? v : 1.0f;        // fminf(v, 1)
}

// One 16-byte colour chunk c with the halves around it: e[0], e[1] = halves 6, 7 of the chunk before, e[2..9] = its own eight,
// e[10], e[11] = halves 0, 1 of the chunk behind.  PH = (8 c) mod 3 is the channel of the chunk's first half, so own half k has the
// channel r = (PH + k) mod 3 and its coefficient begins at e[k + 2 - r]: a chunk needs at most two halves from either side, and the
// pattern repeats every three chunks.  cd: the chunk is chunk 0, whose first coefficient is Cd.  Every index is a constant behind the
// unrolling: the halves stay in registers.
template <int PH>
__device__ __forceinline__ void gsr_grade_chunk(const GsrGradeRule& g, bool cd, const uint16_t (&e)[12], uint16_t (&out)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int r = (PH + k) % 3, at = k + 2 - r;
        out[k] = gsr_grade_half(g, r, PH == 0 && k < 3 && cd, e[at], e[at + 1], e[at + 2]);
    }
}

// K0g: the rule over the resident planes, in k_update's / k_transform's work shape (k_resident.h): 512 threads cover 64 consecutive
// UPLOAD indices i, eight lanes per splat, all eight in one wave; storage slot j = inv[i] (inv: the inverse of the storage order in
// force; NULL: j = i).  A wave covers eight splats, whose mask bits lie in ONE word: it reads that word once (readfirstlane), and a
// group of eight with no bit set does nothing.
//   q = 0      GSR_GRADEF_ALPHA, selected: the true alpha -- alpha0[i] with a visibility in force (alpha0 != NULL), else geoA[j].w --
//              through gsr_grade_alpha into alpha0[i] (if there), geoA[j].w and, with SH, piece 0's .w of colrow[j] (4-byte stores; the
//              position stays).  With a visibility the host applies its rule again behind the kernel: a hidden splat ends at +0.0f
//   q = 1..6   GSR_GRADEF_COLOUR, SH, selected: piece q of colrow[j] = colour chunk q - 1.  NO transpose through LDS: a coefficient's
//              three halves are adjacent in the resident order, so the lane takes dword 3 of the lane before and dword 0 of the lane
//              behind (two cross-lane moves of one dword; lanes 0 and 7 bring zeros nobody reads: chunk 0 begins and chunk 5 ends with
//              a whole coefficient), grades its eight halves by gsr_grade_chunk and stores them to col[q - 1][j] (chunks strided by
//              the capacity) and to colrow[j][q].  A coefficient that straddles two chunks is evaluated by both lanes, from the same
//              three input halves
//   q = 1      GSR_GRADEF_COLOUR, no SH, selected: halves 0..2 of col[j] (chunk 0) rewritten, 8 bytes; its other halves stay +0
// No LDS, no barrier, no scratch, nothing atomic; a slot is read and written by the lanes of its own splat only, every load of a
// splat's pieces in front of the cross-lane moves and every store behind them.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_grade(uint32_t n, uint32_t cap, const uint32_t* __restrict__ mask /* NULL: every splat */, const GsrGradeRule g,
        const uint32_t* __restrict__ inv, float4* __restrict__ geoA, uint4* __restrict__ col, uint4* __restrict__ colrow,
        float* __restrict__ alpha0 /* NULL: no visibility in force */)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = 64 upload indices, eight lanes per splat");
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t i = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    if (i >= n) return;                // (whole splats leave)
    const uint32_t i0 = i & ~7u;       // the wave's first splat: bits [i0 & 31, (i0 & 31) + 8) of word i0 >> 5
    const uint32_t group = mask ? ((uint32_t)__builtin_amdgcn_readfirstlane((int)mask[i0 >> 5]) >> (i0 & 31u)) & 0xffu : 0xffu;
    if (group == 0u) return;           // (wave-uniform: nothing of these eight splats changes)
    const bool selected = (group >> (i & 7u)) & 1u;
    const uint32_t j = selected ? (inv ? inv[i] : i) : 0u;
    if (q == 0 && selected && (g.flags & GSR_GRADEF_ALPHA)) {
        float* const a = reinterpret_cast<float*>(geoA + j) + 3;
        const float v = gsr_grade_alpha(g, alpha0 ? alpha0[i] : *a);
        if (alpha0) alpha0[i] = v;
        *a = v;
        if (SH) reinterpret_cast<float*>(colrow + (size_t)j * 8)[3] = v;
    }
    if (!(g.flags & GSR_GRADEF_COLOUR)) return;        // (uniform)
    if constexpr (SH) {
        const bool colour = selected && q >= 1 && q <= 6;
        uint4 p = make_uint4(0u, 0u, 0u, 0u);
        if (colour) p = colrow[(size_t)j * 8 + q];
        const uint32_t before = (uint32_t)__shfl_up((int)p.w, 1, 64), behind = (uint32_t)__shfl_down((int)p.x, 1, 64);
        if (colour) {
            const uint16_t e[12] = {gsr_lo16(before), gsr_hi16(before), gsr_lo16(p.x), gsr_hi16(p.x), gsr_lo16(p.y), gsr_hi16(p.y),
                                    gsr_lo16(p.z), gsr_hi16(p.z), gsr_lo16(p.w), gsr_hi16(p.w), gsr_lo16(behind), gsr_hi16(behind)};
            uint16_t o[8];
            const int c = q - 1, ph = (8 * c) % 3;
            if (ph == 0) gsr_grade_chunk<0>(g, c == 0, e, o);
            else if (ph == 1) gsr_grade_chunk<1>(g, false, e, o);
            else gsr_grade_chunk<2>(g, false, e, o);
            const uint4 v = make_uint4(gsr_pk(o[0], o[1]), gsr_pk(o[2], o[3]), gsr_pk(o[4], o[5]), gsr_pk(o[6], o[7]));
            col[(size_t)c * cap + j] = v;
            colrow[(size_t)j * 8 + q] = v;
        }
    } else if (q == 1 && selected) {
        uint2* const at = reinterpret_cast<uint2*>(col + j);
        uint2 w = *at;
        const uint16_t hr = gsr_lo16(w.x), hg = gsr_hi16(w.x), hb = gsr_lo16(w.y);
        w.x = gsr_pk(gsr_grade_half(g, 0, true, hr, hg, hb), gsr_grade_half(g, 1, true, hr, hg, hb));
        w.y = (w.y & 0xffff0000u) | gsr_grade_half(g, 2, true, hr, hg, hb);
        *at = w;
    }
}
