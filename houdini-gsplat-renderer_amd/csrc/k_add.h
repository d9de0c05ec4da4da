// k_add.h -- splats added to a resident cloud on the GPU (gsr_add): gsr_remove the other way round.
//
// An add is an upload whose source is two-sided: the resident splats' rows exist only as packed planes (the half arrays of their
// upload are long gone from the arena), the new splats' rows only as staged arrays.  Everything around the pack runs as it is:
// k_move_positions with no new row writes every resident position in upload order, the new positions are copied behind them,
// k_bbox_partials / k_morton_codes / the radix sort order the n_old + m positions as an upload orders them.  What this file adds is the
// pack behind that, and the visibility mask's extension.  A context that never calls gsr_add launches nothing of this file.
#pragma once
#include "gsr_device.h"
#include "k_preprocess.h"

// k_add_pack: the n = n_old + m splats of the new order into the SPARE planes (the host swaps the two sets afterwards).  One
// workgroup = one destination cluster of 64 slots, eight lanes per splat -- k_pack's shape, and k_repack's:
//   slot j' <- the splat i = perm_new[j'] (NULL: i = j')
//   i <  n_old  (resident): lane q LOADS its 16-byte pieces from the old planes at slot j = inv_old[i] (NULL: j = i), as k_repack does:
//               q = 0 geoA[j]; q = 1..6 col[q - 1][j] (chunks strided by the SOURCE capacity; without SH only chunk 0); q = 7 geoB[j];
//               every q colrow[j][q] (SH only)
//   i >= n_old  (new): lane q FORMS its pieces from row i - n_old of the staged arrays, exactly as k_pack does: q = 0 P + opacity (and
//               the Cd halves into LDS), q = 1..6 the SH rows through LDS and gsr_colour_chunk, q = 7 scale + orient with gsr_extent_half
// The branch is uniform over a splat's eight lanes; the wave-level fence and barrier between the LDS writes and reads are reached by
// every lane.  Then ONE store per plane for old and new lanes alike -- geoA', geoB', col'[q - 1] (strided by the DESTINATION capacity)
// and the colour row -- so a wave that mixes old and new splats still writes eight whole 128-byte colrow lines and 128 contiguous bytes
// of geoA', geoB' and each chunk in one store instruction each.  The operands of gsr_cluster_fold are taken from the pieces about to
// be stored: the position of lane 0 and the extent half of lane 7, which is what k_pack feeds it for a new splat and k_repack for a
// resident one -- the bounds are bit for bit those of a fresh upload.  Slots behind n in the last cluster are not written.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_add_pack(uint32_t n, uint32_t n_old, uint32_t cap_src, uint32_t cap_dst, GsrPackSrc src, const uint32_t* __restrict__ perm_new,
           const uint32_t* __restrict__ inv_old,
           const float4* __restrict__ geoA, const uint4* __restrict__ geoB, const uint4* __restrict__ col, const uint4* __restrict__ colrow,
           float4* __restrict__ geoA2, uint4* __restrict__ geoB2, uint4* __restrict__ col2, uint4* __restrict__ colrow2,
           float4* __restrict__ clusA2, float4* __restrict__ clusB2)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = one cluster");
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][56];   // per NEW splat: x[16] y[16] z[16] Cd[3] (+ pad), as in k_pack
    __shared__ float s_red[8][8];                                           // per wave: lo.xyz hi.xyz mf bad
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t jn = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    const bool live = jn < n;
    const uint32_t i = live ? (perm_new ? perm_new[jn] : jn) : 0u;
    const bool fresh = live && i >= n_old;             // (the same for a splat's eight lanes)
    const bool plane = q == 0 || q == 7 || SH || q == 1;   // this lane has a piece of geoA / geoB / a colour chunk
    auto pk = [](uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); };
    uint4 piece = make_uint4(0u, 0u, 0u, 0u);          // q = 0: geoA; q = 1..6: chunk q - 1; q = 7: geoB
    uint4 rowpiece = make_uint4(0u, 0u, 0u, 0u);       // this lane's eighth of the splat's 128-byte row (lane 7: padding)
    if (live && !fresh) {
        const uint32_t j = inv_old ? inv_old[i] : i;
        if (SH) rowpiece = colrow[(size_t)j * 8 + q];
        if (q == 0) {
            const float4 a = geoA[j];
            piece = make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w));
        } else if (q == 7) {
            piece = geoB[j];
        } else if (SH || q == 1) {
            piece = col[(size_t)(q - 1) * cap_src + j];
        }
    } else if (fresh) {
        const size_t t = (size_t)(i - n_old);
        if (q == 0) {
            const float px = src.P[3 * t], py = src.P[3 * t + 1], pz = src.P[3 * t + 2], op = src.alpha[t];
            piece = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), __float_as_uint(op));
            rowpiece = piece;
            s_h[sp][48] = src.Cd[3 * t]; s_h[sp][49] = src.Cd[3 * t + 1]; s_h[sp][50] = src.Cd[3 * t + 2];
        } else if (q == 7) {
            const uint16_t* s = src.scale + 3 * t;
            const uint16_t* o = src.orient + 4 * t;
            const uint16_t s0 = s[0], s1 = s[1], s2 = s[2], o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3];
            piece = make_uint4(pk(s0, s1), pk(s2, o0), pk(o1, o2), pk(o3, gsr_extent_half(s0, s1, s2, o0, o1, o2, o3)));
        } else if (SH) {
            // lanes 1..6: x[0..7] x[8..15] y[0..7] y[8..15] z[0..7] z[8..15] (rows of 16 halves = 32 bytes, 16-byte loads)
            const int ch = (q - 1) >> 1, part = (q - 1) & 1;
            const uint16_t* row = (ch == 0 ? src.shx : (ch == 1 ? src.shy : src.shz)) + 16 * t + 8 * part;
            *reinterpret_cast<uint4*>(&s_h[sp][16 * ch + 8 * part]) = *reinterpret_cast<const uint4*>(row);
        }
    }
    // (a splat's eight lanes sit in one wave: its LDS row is written and read by that wave only)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (fresh && q >= 1 && (SH ? q <= 6 : q == 1)) {
        piece = gsr_colour_chunk<SH>(s_h[sp], q - 1);
        rowpiece = piece;
    }
    // the common stores, and what the cluster's bounds take from them
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, mf = 0.0f;
    bool bad = false;
    if (live) {
        if (q == 0) {
            const float px = __uint_as_float(piece.x), py = __uint_as_float(piece.y), pz = __uint_as_float(piece.z);
            geoA2[jn] = make_float4(px, py, pz, __uint_as_float(piece.w));
            bad = !(__builtin_fabsf(px) < 3.0e38f) || !(__builtin_fabsf(py) < 3.0e38f) || !(__builtin_fabsf(pz) < 3.0e38f);
            lo[0] = hi[0] = px; lo[1] = hi[1] = py; lo[2] = hi[2] = pz;
        } else if (q == 7) {
            geoB2[jn] = piece;
            mf = gsr_h2f((uint16_t)(piece.w >> 16));
            bad = !(mf < 6.0e4f);
        } else if (plane) {
            col2[(size_t)(q - 1) * cap_dst + jn] = piece;
        }
        if (SH) colrow2[(size_t)jn * 8 + q] = rowpiece;
    }
    gsr_cluster_fold(lo, hi, mf, bad, s_red, clusA2, clusB2);
}

// A visibility mask in force, carried into the larger cloud: the words of the n_old resident splats with the bits at and behind n_old
// cleared (a caller's last word may hold anything there), and clear words behind them.  One lane per word of the new mask.
__global__ void __launch_bounds__(256)
k_add_mask_extend(uint32_t n_old, uint32_t words_new, const uint32_t* __restrict__ mask_old, uint32_t* __restrict__ mask_new)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= words_new) return;
    const uint32_t full = n_old >> 5, rest = n_old & 31u;
    uint32_t v = 0u;
    if (w < full) v = mask_old[w];
    else if (w == full && rest) v = mask_old[w] & ((1u << rest) - 1u);
    mask_new[w] = v;
}
