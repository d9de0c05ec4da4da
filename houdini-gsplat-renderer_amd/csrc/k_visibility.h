// k_visibility.h -- resident splats hidden by crop volumes or a mask (gsr_set_visibility).
//
// The only opacity the frame kernels read is geoA[j].w (with SH: its copy in colrow[j][0].w), K1 drops a splat whose opacity is below
// 1/255 before its covariance chain, and the fragment test discards on the same value: a splat whose RESIDENT opacity is +0.0f
// contributes nothing, exactly, in every regime.  So hiding is a resident edit: the true alphas are kept aside (alpha0, upload
// order), and one streaming pass writes, per splat, either its own alpha or +0.0f -- where that differs from what is there.
// No frame kernel changes, and a context that never sets a visibility never launches anything of this file.
#pragma once
#include "gsr_device.h"

// alpha0[i] = the opacity of the splat with upload index i, i in [first, first + cnt): read where the splat sits (inv: upload index ->
// storage slot; NULL: upload order).  Runs while geoA holds the TRUE alphas of the range: over the whole cloud when a visibility
// is first set and after an upload, over the edited rows behind k_update* -- so it does not care whether the alphas came from host
// halves, raw floats or device memory.  4 bytes gathered (from a 16-byte vector) and 4 bytes written, coalesced, per splat.
__global__ void __launch_bounds__(256)
k_alpha_capture(uint32_t first, uint32_t cnt, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA, float* __restrict__ alpha0)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= cnt) return;
    const uint32_t i = first + t;
    const uint32_t j = inv ? inv[i] : i;
    alpha0[i] = reinterpret_cast<const float*>(geoA + j)[3];
}

// One thread per storage slot j.  A stream over geoA (one coalesced 16-byte load per lane) with two 4-byte gathers by upload index
// i = perm[j] -- alpha0[i] and the mask word of i, both small against the stream (a Morton-ordered store keeps neighbours in upload
// order near each other only by accident: at 6 M splats the 24 MB of alpha0 outgrow an XCD's L2 and are served by the Infinity Cache;
// k_alpha_capture, the same gather the other way round, takes 0.115 ms there).  The rule
// arrives by value in the argument segment: it is uniform, sits in scalar registers, and the loop over its volumes has a uniform
// trip count.  want = visible ? alpha0[i] : +0.0f is stored ONLY where its bits differ from what is there: a dragged handle changes
// a thin shell of splats per step, and unconditional 4-byte stores at a 16-byte (and, in colrow, a 128-byte) stride would turn most
// of the pass into partial-line writes.  The two counts -- hidden splats, and splats whose resident bits changed -- are taken per wave by
// ballot and popcount and leave it as ONE 64-bit vector atomic from its first lane (hidden in the low word, changed in the high one;
// none where both are zero), into the workgroup's slot of GSR_VIS_COUNTER_SLOTS counters that lie 64 bytes apart; the host adds the
// slots up.  (With a single counter the 94 k waves of a 6 M cloud queue up behind one address: the pass took 0.71 ms with nothing to
// store and 1.39 ms when every wave also reported a change -- all of it the atomics; LAB_NOTES.md, "Visibility".)  No LDS, no barrier.
#define GSR_VIS_COUNTER_SLOTS  512
#define GSR_VIS_COUNTER_STRIDE 8       // in 64-bit words
__global__ void __launch_bounds__(256)
k_visibility(uint32_t n, const uint32_t* __restrict__ perm, float4* __restrict__ geoA, uint4* __restrict__ colrow /* NULL: no SH */,
             const float* __restrict__ alpha0, const uint32_t* __restrict__ mask /* NULL: none */, GsrVisRule vis,
             unsigned long long* __restrict__ counters)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const bool live = j < n;
    bool hidden = false, changed = false;
    if (live) {
        const float4 a = geoA[j];
        const uint32_t i = perm ? perm[j] : j;
        const uint32_t word = mask ? mask[i >> 5] : 0u;
        hidden = !gsr_splat_visible(vis, a.x, a.y, a.z, word, i);
        const uint32_t want = hidden ? 0u : __float_as_uint(alpha0[i]);
        changed = want != __float_as_uint(a.w);
        if (changed) {
            reinterpret_cast<uint32_t*>(geoA + j)[3] = want;
            if (colrow) reinterpret_cast<uint32_t*>(colrow + (size_t)j * 8)[3] = want;
        }
    }
    const unsigned long long counts = (unsigned long long)__popcll(__ballot(hidden)) | ((unsigned long long)__popcll(__ballot(changed)) << 32);
    if ((threadIdx.x & 63u) == 0u && counts)
        atomicAdd(counters + (size_t)(blockIdx.x & (GSR_VIS_COUNTER_SLOTS - 1u)) * GSR_VIS_COUNTER_STRIDE, counts);
}
