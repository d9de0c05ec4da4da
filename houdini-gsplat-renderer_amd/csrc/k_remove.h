// k_remove.h -- resident splats removed on the GPU (gsr_remove): the stream compaction in front of k_repack.
//
// A removal is a move whose source is a subset: the survivors' positions go through the ordering of an upload, and k_repack (as it
// is) carries their planes into the spare set, taking "the old slot of upload index i'" from src_slot where a move hands it the
// inverse of the old storage order.  What this file adds is everything in upload order in front of that: which splats stay (mark),
// where each workgroup's survivors begin (scan), and the survivors' positions, old slots, true alphas and visibility-mask bits at their
// new upload indices (compact).  A context that never calls gsr_remove launches nothing of this file.
//
// One workgroup of GSR_REMOVE_THREADS = 256 lanes (four waves) spans GSR_REMOVE_BLOCK = 4096 consecutive upload indices in
// 16 rounds; round r, wave w is the block's wave-slot s = 4 r + w and holds the 64 splats [64 s, 64 s + 64) of the block, one per
// lane.  The bitmap is the SURVIVORS': one 64-bit word per wave-slot, bit l = the splat of lane l stays.  Every word of every block is
// written (a wave-slot behind n writes 0), so a bit behind n is clear and nothing behind the mark looks at n again.
#pragma once
#include "gsr_device.h"

#define GSR_REMOVE_THREADS 256
#define GSR_REMOVE_SLOTS   (GSR_REMOVE_BLOCK / 64)      // wave-slots (bitmap words of 64 bits) per block
static_assert(GSR_REMOVE_BLOCK % (GSR_REMOVE_THREADS) == 0 && GSR_REMOVE_SLOTS == 64, "the compaction scans a block's 64 words in one wave");

// 1. MARK.  gone(i) = the caller's bit (mask: ceil(n / 32) words, NULL: none) or, with HIDDEN, what the visibility in force hides:
// gsr_splat_visible on the raw position bits geoA[inv[i]] holds (inv: upload index -> storage slot; NULL: upload order) and the word
// of the visibility mask in force (NULL: none).  A wave's 64 verdicts are one ballot; lane 0 stores it as one 8-byte vector store (two
// whole 32-bit words of the bitmap; no atomic).  A wave keeps the popcounts of its 16 ballots in a scalar; the four of them meet in a
// four-word LDS table and thread 0 leaves the block's survivor count.
template <bool HIDDEN>
__global__ void __launch_bounds__(GSR_REMOVE_THREADS)
k_remove_mark(uint32_t n, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA,
              const uint32_t* __restrict__ vis_mask, GsrVisRule vis, unsigned long long* __restrict__ keep, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_cnt[GSR_REMOVE_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t kept = 0u;                                // (wave-uniform)
#pragma unroll 1
    for (uint32_t r = 0; r < GSR_REMOVE_BLOCK / GSR_REMOVE_THREADS; ++r) {
        const uint32_t s = r * (GSR_REMOVE_THREADS / 64u) + wave;
        const uint32_t i = blockIdx.x * (uint32_t)GSR_REMOVE_BLOCK + s * 64u + lane;
        bool stay = false;
        if (i < n) {
            stay = mask ? ((mask[i >> 5] >> (i & 31u)) & 1u) == 0u : true;
            if (HIDDEN && stay) {
                const float4 a = geoA[inv ? inv[i] : i];
                stay = gsr_splat_visible(vis, a.x, a.y, a.z, vis_mask ? vis_mask[i >> 5] : 0u, i);
            }
        }
        const unsigned long long word = __ballot(stay);
        kept += (uint32_t)__popcll(word);
        if (lane == 0u) keep[(size_t)blockIdx.x * GSR_REMOVE_SLOTS + s] = word;
    }
    if (lane == 0u) s_cnt[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// 2. SCAN.  offsets[b] = the survivors of the blocks before b; offsets[nblocks] = all of them (the host fetches that word).  ONE
// workgroup of 1024 lanes walks the counts 1024 at a time: an inclusive scan inside each wave by shuffles, the 16 wave totals through a
// 17-word LDS table (scanned by the first wave), the running total carried in a register.  (6 M splats: 1465 counts, two rounds.)
#define GSR_REMOVE_SCAN_THREADS 1024
__global__ void __launch_bounds__(GSR_REMOVE_SCAN_THREADS)
k_remove_scan(uint32_t nblocks, const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets)
{
    __shared__ uint32_t s_wave[GSR_REMOVE_SCAN_THREADS / 64 + 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t running = 0u;
    for (uint32_t base = 0; base < nblocks; base += GSR_REMOVE_SCAN_THREADS) {      // (uniform trip count: the barriers are met by all)
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nblocks ? counts[b] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        if (wave == 0u) {                              // the 16 wave totals -> what lies before each wave, and behind them the round's total
            const uint32_t t = lane < GSR_REMOVE_SCAN_THREADS / 64u ? s_wave[lane] : 0u;
            uint32_t ti = t;
#pragma unroll
            for (int d = 1; d < GSR_REMOVE_SCAN_THREADS / 64; d <<= 1) {
                const uint32_t up = __shfl_up(ti, d, 64);
                if (lane >= (uint32_t)d) ti += up;
            }
            if (lane < GSR_REMOVE_SCAN_THREADS / 64u) s_wave[lane] = ti - t;
            if (lane == GSR_REMOVE_SCAN_THREADS / 64u - 1u) s_wave[GSR_REMOVE_SCAN_THREADS / 64] = ti;
        }
        __syncthreads();
        if (b < nblocks) offsets[b] = running + s_wave[wave] + incl - v;
        running += s_wave[GSR_REMOVE_SCAN_THREADS / 64];
        __syncthreads();                               // (the table is rewritten by the next round)
    }
    if (threadIdx.x == 0u) offsets[nblocks] = running;
}

// 3. COMPACT.  One lane per old upload index, in k_remove_mark's shape.  The block's 64 bitmap words are popcounted and scanned by its
// first wave into a 64-word LDS table; survivor i then has the new upload index
//     i' = offsets[block] + table[wave-slot] + mbcnt(word)       (the set bits of its wave's word below its own lane)
// and writes, at i': the raw position bits of geoA[j].xyz (j = its old slot) to Pup, the array the ordering reads; src_slot[i'] = j,
// what k_repack takes in the place of the old order's inverse; and with VIS (a visibility in force) its true alpha into the SECOND
// alpha0 array -- never in place: writer i' and reader i are lanes of different workgroups -- and, if the visibility has a mask and its
// bit there is set, that bit into the new mask: a zeroed buffer and a vector atomic OR without return.
template <bool VIS>
__global__ void __launch_bounds__(GSR_REMOVE_THREADS)
k_remove_compact(const unsigned long long* __restrict__ keep, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ inv,
                 const float4* __restrict__ geoA, float* __restrict__ Pup, uint32_t* __restrict__ src_slot,
                 const float* __restrict__ alpha0, float* __restrict__ alpha0_new, const uint32_t* __restrict__ vis_mask,
                 uint32_t* __restrict__ vis_mask_new)
{
    __shared__ uint32_t s_pre[GSR_REMOVE_SLOTS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long* const words = keep + (size_t)blockIdx.x * GSR_REMOVE_SLOTS;
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
        if (!((word >> lane) & 1ull)) continue;
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(word >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)word, 0u));
        const uint32_t i = blockIdx.x * (uint32_t)GSR_REMOVE_BLOCK + s * 64u + lane;
        const uint32_t to = first + s_pre[s] + below;
        const uint32_t j = inv ? inv[i] : i;
        const float4 a = geoA[j];
        float* const o = Pup + 3 * (size_t)to;
        o[0] = a.x; o[1] = a.y; o[2] = a.z;
        src_slot[to] = j;
        if (VIS) {
            alpha0_new[to] = alpha0[i];
            if (vis_mask && ((vis_mask[i >> 5] >> (i & 31u)) & 1u)) atomicOr(vis_mask_new + (to >> 5), 1u << (to & 31u));
        }
    }
}

// gsr_remove_map's rule is the same arithmetic on the host (gsr_api.hip): new_index[i] = the survivors before i.
