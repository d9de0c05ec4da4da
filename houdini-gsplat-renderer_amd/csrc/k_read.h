// k_read.h -- K0r: the resident cloud read back in UPLOAD order (gsr_read, gsr_read_device): k_pack run backwards, in
// k_update's shape.  Rows [0, cnt) of the destination arrays get the attributes of the splats [first, first + cnt) of the upload:
//   row t  <-  storage slot j = inv[first + t]     (inv: upload index -> storage slot, the inverse of perm; NULL: upload order)
// With a row list (rows: device memory, cnt upload indices; NULL: none -- gsr_read_masked's, written by k_copy_compact) row t is the
// splat rows[t] in the place of first + t, and everything below reads "first + t" as "rows[t]".
// One workgroup of GSR_PACK_THREADS = 64 rows, k_resident.h's lane roles.
// LOADS (a lane whose piece feeds no array that is wanted loads nothing; the wanted set is uniform: it sits in the argument segment):
//   SH and a colour array wanted:  lane q = 0..6 loads piece q of the splat's 128-byte colrow line (ONE request per splat: piece 0 is
//                                  geoA[j] bit for bit, pieces 1..6 the colour chunks), lane 7 geoB[j]
//   otherwise:                     lane 0 geoA[j], lane 1 col[j] (chunk 0: Cd), lane 7 geoB[j] -- a P-only read touches 16 bytes per splat
//   a visibility in force:         lane 0 takes the alpha from alpha0[first + t] (the TRUE alphas, upload order: a coalesced read), not
//                                  from the resident .w, which is +0.0f for a hidden splat
// TRANSPOSE (SH arrays wanted): lanes 1..6 put the eight halves of chunk q - 1 into the splat's LDS row by gsr_colour_half_slot, the
// rule gsr_colour_chunk reads it by, and the row is read back as k_pack wrote it.  Whole splats behind cnt leave in front of the sync.
// Index 15 of the x / y / z rows (slot 15 of a 16-slot sh row) is not resident -- k_pack never reads it -- and comes back as a zero
// half (+0.0f).
// STORES (plain vector stores; only rows t < cnt are touched):
//   halves (F32 = false; the destinations are the verb's own 256-byte aligned device rows in gsr_upload_append's layout):
//     lane 0 P (3 x 4 B) + alpha (4 B); lane 1 Cd (3 x 2 B: halves 0..2 of chunk 0); lanes 1..6 16 bytes of the x / y / z rows;
//     lane 7 scale (3 x 2 B) + orient (8 B)
//   float32 (F32 = true; the caller's arrays, gsr_device_attrs' layout; every half as the float32 of exactly that value, gsr_h2f):
//     every value is ONE 4-byte store inside its array (rows are not 16-byte aligned: 15 vec3 are 180 bytes); lanes 1..6 store floats
//     [8 (q - 1), 8 (q - 1) + 8) of the splat's 3 * vpp floats (float f <- LDS half gsr_sh_float_slot(f)); slots >= vpp are not written out
// Per splat with everything: 128 + 16 bytes read, 122 (halves) or 64 + 12 vpp (float32) written.  Nothing resident is written.
#pragma once
#include "k_resident.h"

template <bool F32> struct GsrReadDst;
template <> struct GsrReadDst<false> {      // device rows in gsr_upload_append's layout (NULL: not wanted)
    float *P, *alpha;
    uint16_t *Cd, *scale, *orient, *shx, *shy, *shz;
    __device__ __forceinline__ bool wants_sh() const { return shx != nullptr; }      // (all three or none: the host checks)
};
template <> struct GsrReadDst<true> {       // the caller's float32 arrays in gsr_device_attrs' layout (NULL: not wanted)
    float *P, *alpha, *Cd, *scale, *orient, *sh;
    int32_t vpp;                            // vec3 per point of sh: 1..16
    __device__ __forceinline__ bool wants_sh() const { return sh != nullptr; }
};

template <bool SH, bool F32>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_unpack(uint32_t first, uint32_t cnt, GsrReadDst<F32> dst, const uint32_t* __restrict__ inv,
         const float4* __restrict__ geoA, const uint4* __restrict__ geoB, const uint4* __restrict__ col, const uint4* __restrict__ colrow,
         const float* __restrict__ alpha0, const uint32_t* __restrict__ rows)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = 64 rows, eight lanes per splat");
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][GSR_ROW_HALVES];
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t t = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    if (t >= cnt) return;              // (whole splats leave: the lanes that meet at the wave barrier below are those that stay)
    const uint32_t u = rows ? rows[t] : first + t;     // the row's upload index
    const uint32_t j = inv ? inv[u] : u;
    const bool sh = SH && dst.wants_sh();
    const bool colour = dst.Cd || sh, shape = dst.scale || dst.orient;
    const bool geo = dst.P || (dst.alpha && !alpha0);          // the resident P + opacity word is needed
    uint4 piece = make_uint4(0u, 0u, 0u, 0u);
    if (SH && colour) {
        if (q == 7) { if (shape) piece = geoB[j]; }
        else if (q == 0 ? geo : (q == 1 || sh)) piece = colrow[(size_t)j * 8 + q];
    } else if (q == 0) {
        if (geo) piece = gsr_as_uint4(geoA[j]);
    } else if (q == 1) {
        if (colour) piece = col[j];
    } else if (q == 7) {
        if (shape) piece = geoB[j];
    }
    if (q == 0) {
        if (dst.P) {
            float* p = dst.P + 3 * (size_t)t;
            p[0] = __uint_as_float(piece.x); p[1] = __uint_as_float(piece.y); p[2] = __uint_as_float(piece.z);
        }
        if (dst.alpha) dst.alpha[t] = alpha0 ? alpha0[u] : __uint_as_float(piece.w);
        if (sh) { s_h[sp][15] = 0; s_h[sp][31] = 0; s_h[sp][47] = 0; }       // (the index no chunk holds)
    } else if (q == 7) {
        const GsrShape h = gsr_shape_split(piece);
        if constexpr (F32) {
            if (dst.scale) { float* s = dst.scale + 3 * (size_t)t; s[0] = gsr_h2f(h.s0); s[1] = gsr_h2f(h.s1); s[2] = gsr_h2f(h.s2); }
            if (dst.orient) { float* o = dst.orient + 4 * (size_t)t; o[0] = gsr_h2f(h.o0); o[1] = gsr_h2f(h.o1); o[2] = gsr_h2f(h.o2); o[3] = gsr_h2f(h.o3); }
        } else {
            if (dst.scale) { uint16_t* s = dst.scale + 3 * (size_t)t; s[0] = h.s0; s[1] = h.s1; s[2] = h.s2; }
            // (orient rows are 8 bytes in a 256-byte aligned section; the extent half, the high half of .w, is derived and stays behind)
            if (dst.orient) *reinterpret_cast<uint2*>(dst.orient + 4 * (size_t)t) = make_uint2((piece.y >> 16) | (piece.z << 16), (piece.z >> 16) | (piece.w << 16));
        }
    } else {
        if (q == 1 && dst.Cd) {        // halves 0..2 of chunk 0
            if constexpr (F32) { float* c = dst.Cd + 3 * (size_t)t; c[0] = gsr_h2f(gsr_lo16(piece.x)); c[1] = gsr_h2f(gsr_hi16(piece.x)); c[2] = gsr_h2f(gsr_lo16(piece.y)); }
            else { uint16_t* c = dst.Cd + 3 * (size_t)t; c[0] = gsr_lo16(piece.x); c[1] = gsr_hi16(piece.x); c[2] = gsr_lo16(piece.y); }
        }
        if (sh) {
            const uint32_t w[4] = {piece.x, piece.y, piece.z, piece.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int at = gsr_colour_half_slot(q - 1, k);
                if (at < 48) s_h[sp][at] = (k & 1) ? gsr_hi16(w[k >> 1]) : gsr_lo16(w[k >> 1]);      // (the Cd halves went out above)
            }
        }
    }
    if (!sh) return;
    gsr_wave_lds_sync();
    if (q < 1 || q > 6) return;
    if constexpr (F32) {
        const int nf = 3 * dst.vpp;                    // floats of a splat's row (<= 48)
        float* row = dst.sh + (size_t)t * (size_t)nf;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int f = 8 * (q - 1) + k;
            if (f < nf) row[f] = gsr_h2f(s_h[sp][gsr_sh_float_slot(f)]);
        }
    } else {
        // lanes 1..6: x[0..7] x[8..15] y[0..7] y[8..15] z[0..7] z[8..15] (rows of 16 halves = 32 bytes, 16-byte stores)
        const int ch = (q - 1) >> 1, part = (q - 1) & 1;
        uint16_t* row = (ch == 0 ? dst.shx : (ch == 1 ? dst.shy : dst.shz)) + 16 * (size_t)t + 8 * part;
        *reinterpret_cast<uint4*>(row) = *reinterpret_cast<const uint4*>(&s_h[sp][16 * ch + 8 * part]);
    }
}
