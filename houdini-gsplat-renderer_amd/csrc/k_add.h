// k_add.h -- splats added to a resident cloud on the GPU (gsr_add): gsr_remove the other way round.
//
// An add is an upload whose source is two-sided: the resident splats' rows exist only as packed planes (the half arrays of their
// upload are long gone from the arena), the new splats' rows only as staged arrays.  Everything around the pack runs as it is:
// k_move_positions with no new row writes every resident position in upload order, the new positions are copied behind them,
// k_bbox_partials / k_morton_codes / the radix sort order the n_old + m positions as an upload orders them.  What this file adds is the
// pack behind that, and the visibility mask's extension.  A context that never calls gsr_add launches nothing of this file.
#pragma once
#include "gsr_device.h"
#include "k_resident.h"

// k_add_pack: the n = n_old + m splats of the new order into the SPARE planes (the host swaps the two sets afterwards).  One
// workgroup = one destination cluster, k_resident.h's lane roles:
//   slot j' <- the splat i = perm_new[j'] (NULL: i = j')
//   i <  n_old  (resident): its pieces are LOADED from the old planes at slot j = inv_old[i] (NULL: j = i), the loads of k_repack
//               (chunks strided by the SOURCE capacity)
//   i >= n_old  (new): its pieces are FORMED from row i - n_old of the staged arrays, as k_pack forms them
// The branch is uniform over a splat's eight lanes, and every lane reaches the sync.  Then ONE store per plane for old and new lanes
// alike (chunks strided by the DESTINATION capacity), so a wave that mixes old and new splats still writes eight whole 128-byte colrow
// lines and 128 contiguous bytes of geoA', geoB' and each chunk in one store instruction each.  The bounds take the pieces about to
// be stored.  Slots behind n in the last cluster are not written.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_add_pack(uint32_t n, uint32_t n_old, uint32_t cap_src, uint32_t cap_dst, GsrPackSrc src, const uint32_t* __restrict__ perm_new,
           const uint32_t* __restrict__ inv_old,
           const float4* __restrict__ geoA, const uint4* __restrict__ geoB, const uint4* __restrict__ col, const uint4* __restrict__ colrow,
           float4* __restrict__ geoA2, uint4* __restrict__ geoB2, uint4* __restrict__ col2, uint4* __restrict__ colrow2,
           float4* __restrict__ clusA2, float4* __restrict__ clusB2)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = one cluster");
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][GSR_ROW_HALVES];   // (used by the NEW splats only)
    __shared__ float s_red[8][8];                                           // per wave: lo.xyz hi.xyz mf bad
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t jn = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    const bool live = jn < n;
    const uint32_t i = live ? (perm_new ? perm_new[jn] : jn) : 0u;
    const bool fresh = live && i >= n_old;             // (the same for a splat's eight lanes)
    uint4 piece = make_uint4(0u, 0u, 0u, 0u), rowpiece = piece;
    if (fresh) {
        piece = gsr_stage_new_splat<SH>(q, (size_t)(i - n_old), src, s_h[sp]);
        if (q == 0) rowpiece = piece;
    } else if (live) {
        const uint32_t j = inv_old ? inv_old[i] : i;
        if (SH) rowpiece = colrow[(size_t)j * 8 + q];
        if (q == 0) piece = gsr_as_uint4(geoA[j]);
        else if (q == 7) piece = geoB[j];
        else if (gsr_colour_lane<SH>(q)) piece = col[(size_t)(q - 1) * cap_src + j];
    }
    // The pieces land HERE (s_waitcnt vmcnt(0); expcnt and lgkmcnt stay open): they are loaded in one set of q branches and stored in
    // another, behind the sync.  Left to the compiler, the wait sits in front of each store, where it also waits for the store of the
    // branch before: three store round trips in a row, 0.08 ms of 0.75 at 6 M splats (LAB_NOTES.md, "Resident-layout kernels in one header").
    __builtin_amdgcn_s_waitcnt(0x0f70);
    gsr_wave_lds_sync();
    if (fresh && gsr_colour_lane<SH>(q)) rowpiece = piece = gsr_colour_chunk<SH>(s_h[sp], q - 1);
    GsrClusterIn in;
    if (live) {
        gsr_store_geo(q, jn, piece, geoA2, geoB2, in);
        if (gsr_colour_lane<SH>(q)) col2[(size_t)(q - 1) * cap_dst + jn] = piece;
        if (SH) colrow2[(size_t)jn * 8 + q] = rowpiece;
    }
    gsr_cluster_fold(in, s_red, clusA2, clusB2);
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
