// k_copy.h -- selected resident splats copied on the GPU (gsr_read_masked, gsr_read_masked_device, gsr_duplicate):
// k_remove.h's stream compaction with the SELECTED splats in the survivors' place.
//
// A masked read is that compaction in front of k_unpack, which takes the compacted upload indices as its row list.  A duplicate is a
// move whose source is a multiset: the n resident splats and, behind them, the copies, in the ascending upload order of their
// originals; the ordering of an upload runs over the n + m positions and k_repack (as it is) carries the planes, taking "the old slot
// of upload index i'" from a slot list in which a copy names the slot of its original.  A context that never calls one of the three
// verbs launches nothing of this file.
//
// The work shape is k_remove.h's: one workgroup of GSR_REMOVE_THREADS = 256 lanes (four waves) spans GSR_REMOVE_BLOCK = 4096
// consecutive upload indices in 16 rounds; round r, wave w is the block's wave-slot s = 4 r + w and holds the 64 splats
// [64 s, 64 s + 64) of the block, one per lane.  The bitmap is the SELECTION's: one 64-bit word per wave-slot, bit l = the splat of
// lane l is selected.  Every word of every block is written (a wave-slot behind n writes 0), so a bit behind n is clear and nothing
// behind the mark looks at the caller's mask again.  k_remove_scan, as it is, turns the block counts into block offsets and the total.
#pragma once
#include "gsr_device.h"
#include "k_remove.h"

// 1. MARK.  selected(i) = i < n and the caller's bit (mask: ceil(n / 32) words; NULL: every splat).  A wave's 64 verdicts are one
// ballot; lane 0 stores it as one 8-byte vector store (no atomic).  A wave keeps the popcounts of its 16 ballots in a scalar; the four
// of them meet in a four-word LDS table and thread 0 leaves the block's count of SET bits.
__global__ void __launch_bounds__(GSR_REMOVE_THREADS)
k_copy_mark(uint32_t n, const uint32_t* __restrict__ mask, unsigned long long* __restrict__ sel, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_cnt[GSR_REMOVE_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t set = 0u;                                 // (wave-uniform)
#pragma unroll 1
    for (uint32_t r = 0; r < GSR_REMOVE_BLOCK / GSR_REMOVE_THREADS; ++r) {
        const uint32_t s = r * (GSR_REMOVE_THREADS / 64u) + wave;
        const uint32_t i = blockIdx.x * (uint32_t)GSR_REMOVE_BLOCK + s * 64u + lane;
        const bool take = i < n && (mask ? ((mask[i >> 5] >> (i & 31u)) & 1u) != 0u : true);
        const unsigned long long word = __ballot(take);
        set += (uint32_t)__popcll(word);
        if (lane == 0u) sel[(size_t)blockIdx.x * GSR_REMOVE_SLOTS + s] = word;
    }
    if (lane == 0u) s_cnt[wave] = set;
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// 2. COMPACT.  One lane per upload index, in k_copy_mark's shape.  The block's 64 bitmap words are popcounted and scanned by its first
// wave into a 64-word LDS table; selected splat i then has the rank
//     r = offsets[block] + table[wave-slot] + mbcnt(word)        (the set bits of its wave's word below its own lane)
// and writes rows[r] = i: the row list k_unpack reads.  Plain vector stores, no atomic: every rank is written by one lane.
// DUP (gsr_duplicate): the lane of EVERY resident splat i < n also leaves what the ordering and k_repack read of the n + m splats of
// the larger cloud -- the position bits geoA[j].xyz (j = inv[i], its slot; inv NULL: upload order) at Pup[i] and the slot j at
// src_slot[i]; a selected one leaves the same two again at n + r, the upload index of its copy, and, under a visibility (alpha0: the
// true alphas in upload order; NULL: none in force), alpha0[i] at alpha0_new[n + r].  alpha0_new may be alpha0 itself: index n + r is
// behind every index that is read.
template <bool DUP>
__global__ void __launch_bounds__(GSR_REMOVE_THREADS)
k_copy_compact(uint32_t n, const unsigned long long* __restrict__ sel, const uint32_t* __restrict__ offsets, uint32_t* __restrict__ rows,
               const uint32_t* __restrict__ inv, const float4* __restrict__ geoA, float* __restrict__ Pup, uint32_t* __restrict__ src_slot,
               const float* alpha0, float* alpha0_new)
{
    __shared__ uint32_t s_pre[GSR_REMOVE_SLOTS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long* const words = sel + (size_t)blockIdx.x * GSR_REMOVE_SLOTS;
    if (wave == 0u) {
        const uint32_t v = (uint32_t)__popcll(words[lane]);
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        s_pre[lane] = incl - v;
    }
    __syncthreads();
    const uint32_t first = offsets[blockIdx.x];
#pragma unroll 1
    for (uint32_t r = 0; r < GSR_REMOVE_BLOCK / GSR_REMOVE_THREADS; ++r) {
        const uint32_t s = r * (GSR_REMOVE_THREADS / 64u) + wave;
        const unsigned long long word = words[s];      // (one address per wave)
        const uint32_t i = blockIdx.x * (uint32_t)GSR_REMOVE_BLOCK + s * 64u + lane;
        const bool take = ((word >> lane) & 1ull) != 0ull;
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(word >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)word, 0u));
        const uint32_t rank = first + s_pre[s] + below;
        if (take) rows[rank] = i;
        if (!DUP || i >= n) continue;
        const uint32_t j = inv ? inv[i] : i;
        const float4 a = geoA[j];
        float* const o = Pup + 3 * (size_t)i;
        o[0] = a.x; o[1] = a.y; o[2] = a.z;
        src_slot[i] = j;
        if (take) {
            const size_t to = (size_t)n + rank;
            float* const oc = Pup + 3 * to;
            oc[0] = a.x; oc[1] = a.y; oc[2] = a.z;
            src_slot[to] = j;
            if (alpha0) alpha0_new[to] = alpha0[i];
        }
    }
}

// gsr_copy_map's rule is the same arithmetic on the host (gsr_resident_edit.h): rows[r] = the r-th set bit, ascending.
