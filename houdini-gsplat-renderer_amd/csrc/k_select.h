// k_select.h -- resident splats selected by screen region (gsr_select): a rectangle, a painted image, a depth test.
//
// A splat is selected by where its CENTRE projects.  The arithmetic is gsr_k1_front's (k_preprocess.h) restated: the origin round
// trip, the two affine chains, the clip and opacity tests, the window centre and the window depth, in that order and with the same
// roundings, so a rectangle hits exactly the centres the frame's records carry.  It is restated and not shared because K1's code
// object is pinned as it is; tests/test_select.py holds the restatement to the oracle's records bit for bit.  Every multiply-add is an
// explicit fmaf and no product feeds an add anywhere else (the translation units are compiled with -ffp-contract=off), the
// divisions are IEEE divisions: x86 and gfx950 agree in every bit, and gsr_select_eval (host) and k_select go through the one function.
// No frame kernel changes, and a context that never selects launches nothing of this file but k_mask_count (the bit count of a mask,
// at the end: gsr_transform and gsr_grade).
#pragma once
#include "gsr_device.h"

// The constants of one selection, by value in the kernel's argument segment: 41 dwords, uniform, in scalar registers.  (Not GsrFrame:
// its hundred scalars do not fit beside a kernel's pointers; gsr_device.h, gsr_frame_fetch.)
#define GSR_SELF_ANY_OPACITY 1         // = GSR_SELECT_ANY_OPACITY: the opacity test is dropped (a hidden splat's +0.0f can be hit)
struct GsrSelectRule {
    float ov[12];                      // rows 0..2 of glH_ObjViewMatrix: ov[r*4+c]
    float pr[16];                      // glH_ProjectMatrix rows
    float origin[3];
    float W, H;                        // (float)width, (float)height
    float x0, y0, x1, y1;              // the rect: GL window coordinates, half-open
    float depth_bias;
    int32_t flags;                     // GSR_SELF_*
    int32_t width, height;
};
static_assert(sizeof(GsrSelectRule) == 41 * 4, "the rule is a run of 41 dwords");

__host__ __device__ __forceinline__ float gsr_sel_aff4(const float* m, float x, float y, float z)
{
    return __builtin_fmaf(m[0], x, __builtin_fmaf(m[1], y, __builtin_fmaf(m[2], z, m[3])));
}

// THE rule, in one place.  (px, py, pz): the raw position bits, what geoA holds; a: the RESIDENT opacity (+0.0f for a splat a
// visibility hides).  image: one bit per pixel, bit p & 31 of word p >> 5 (NULL: no image clause); depth: float[height * width] window
// depths (NULL: no depth clause); both are only dereferenced at a pixel the centre lies in.  centre (or NULL): cx, cy, zw of a
// SELECTABLE splat -- one that passes the clip and opacity tests, whatever the region says -- else three NaNs.
// The comparisons are written so that a NaN anywhere means "no hit".
__host__ __device__ __forceinline__ bool gsr_select_hit(const GsrSelectRule& r, float px, float py, float pz, float a,
                                                        const uint32_t* __restrict__ image, const float* __restrict__ depth, float* centre)
{
    // fl32(P - origin) + origin
    const float x = (px - r.origin[0]) + r.origin[0];
    const float y = (py - r.origin[1]) + r.origin[1];
    const float z = (pz - r.origin[2]) + r.origin[2];
    const float tvx = gsr_sel_aff4(&r.ov[0], x, y, z);
    const float tvy = gsr_sel_aff4(&r.ov[4], x, y, z);
    const float tvz = gsr_sel_aff4(&r.ov[8], x, y, z);
    const float ftvy = -tvy;
    const float clx = gsr_sel_aff4(&r.pr[0], tvx, ftvy, tvz);
    const float cly = gsr_sel_aff4(&r.pr[4], tvx, ftvy, tvz);
    const float clz = gsr_sel_aff4(&r.pr[8], tvx, ftvy, tvz);
    const float clw = gsr_sel_aff4(&r.pr[12], tvx, ftvy, tvz);
    const bool selectable = (clw > 0.0f) && !(clz < -clw || clz > clw) && ((r.flags & GSR_SELF_ANY_OPACITY) || a >= (1.0f / 255.0f));
    if (!selectable) {
        if (centre) { centre[0] = centre[1] = centre[2] = __builtin_nanf(""); }
        return false;
    }
    const float cx = __builtin_fmaf(clx / clw, 0.5f, 0.5f) * r.W;
    const float cy = __builtin_fmaf((-cly) / clw, 0.5f, 0.5f) * r.H;
    const float zw = __builtin_fmaf(clz / clw, 0.5f, 0.5f);
    if (centre) { centre[0] = cx; centre[1] = cy; centre[2] = zw; }
    // the rect, always (a NaN centre fails every comparison); a NaN window depth is no hit either, with or without a depth clause
    if (!(r.x0 <= cx && cx < r.x1 && r.y0 <= cy && cy < r.y1) || !(zw == zw)) return false;
    if (!image && !depth) return true;
    // the pixel: defined only inside the image -- no index is ever formed from a centre outside it
    if (!(cx >= 0.0f && cx < r.W && cy >= 0.0f && cy < r.H)) return false;
    const int qx = (int)cx, qy = (int)cy;
    const size_t p = (size_t)qy * (size_t)r.width + (size_t)qx;
    if (image && !((image[p >> 5] >> (p & 31u)) & 1u)) return false;
    if (depth && !(zw <= depth[p] + r.depth_bias)) return false;       // (one f32 add, one compare)
    return true;
}

// how a wave's 32 verdicts meet the 32 bits the mask held (GSR_SELECT_*)
#define GSR_SELOP_REPLACE   0
#define GSR_SELOP_ADD       1
#define GSR_SELOP_SUBTRACT  2
#define GSR_SELOP_INTERSECT 3
#define GSR_SELOP_TOGGLE    4
__host__ __device__ __forceinline__ uint32_t gsr_select_apply(int op, uint32_t prior, uint32_t hit)
{
    return op == GSR_SELOP_ADD ? (prior | hit) : op == GSR_SELOP_SUBTRACT ? (prior & ~hit) : op == GSR_SELOP_INTERSECT ? (prior & hit) :
           op == GSR_SELOP_TOGGLE ? (prior ^ hit) : hit;
}

// One thread per UPLOAD index i, in k_alpha_capture's shape: one 16-byte gather geoA[inv[i]] (inv: upload index -> storage slot;
// NULL: upload order), the rule, and -- only by the lanes that are still candidates -- the 4-byte gathers of the image word and the
// depth texel.  A wave's 64 verdicts are one ballot; lanes 0 and 32 each own one 32-bit word of the mask: each loads the prior word if
// the op reads it, applies the op, clears the bits at and behind n, and stores it with a plain vector store -- iff its word index is
// below ceil(n / 32): the last wave may own only one of its two words, and not one byte behind the mask is written.  No atomic touches
// the mask, nothing is cleared beforehand, and the result does not depend on the order the waves run in.
// The two counts -- splats hit, bits set afterwards -- leave the wave as ONE 64-bit vector atomic from its first lane (hit in the low
// word, set in the high one; none where both are zero) into the workgroup's slot of GSR_SEL_COUNTER_SLOTS counters 64 bytes apart, as
// k_visibility's do (k_visibility.h records what a single counter address cost); the host adds the slots up.  No LDS, no barrier.
#define GSR_SELECT_THREADS     256
#define GSR_SEL_COUNTER_SLOTS  512
#define GSR_SEL_COUNTER_STRIDE 8       // in 64-bit words
// The epilogue of every selection kernel (k_select, k_select_attrs.h): thread i = blockIdx.x * GSR_SELECT_THREADS + threadIdx.x holds
// the verdict of upload index i (false for i >= n); every lane of the wave must call it.  The ballot, the two mask words of lanes 0
// and 32, and the wave's counts, as described above.
__device__ __forceinline__ void gsr_select_epilogue(uint32_t n, uint32_t i, bool hit, int op, uint32_t* __restrict__ mask,
                                                    unsigned long long* __restrict__ counters)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long ballot = __ballot(hit);   // (every lane of the wave is here: nobody has left)
    uint32_t set = 0u;
    if ((lane & 31u) == 0u) {
        const uint32_t w = i >> 5, words = (n >> 5) + ((n & 31u) ? 1u : 0u);
        if (w < words) {
            const uint32_t mine = lane ? (uint32_t)(ballot >> 32) : (uint32_t)ballot;
            uint32_t v = gsr_select_apply(op, op == GSR_SELOP_REPLACE ? 0u : mask[w], mine);
            const uint32_t left = n - w * 32u;         // splats from this word's first bit on (>= 1)
            if (left < 32u) v &= (1u << left) - 1u;
            mask[w] = v;
            set = (uint32_t)__popc(v);
        }
    }
    const uint32_t n_set = (uint32_t)__builtin_amdgcn_readlane((int)set, 0) + (uint32_t)__builtin_amdgcn_readlane((int)set, 32);
    const unsigned long long counts = (unsigned long long)__popcll(ballot) | ((unsigned long long)n_set << 32);
    if (lane == 0u && counts)
        atomicAdd(counters + (size_t)(blockIdx.x & (GSR_SEL_COUNTER_SLOTS - 1u)) * GSR_SEL_COUNTER_STRIDE, counts);
}

__global__ void __launch_bounds__(GSR_SELECT_THREADS)
k_select(uint32_t n, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA, GsrSelectRule rule,
         const uint32_t* __restrict__ image /* NULL: none */, const float* __restrict__ depth /* NULL: none */, int op,
         uint32_t* __restrict__ mask, unsigned long long* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * (uint32_t)GSR_SELECT_THREADS + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const float4 a = geoA[inv ? inv[i] : i];
        hit = gsr_select_hit(rule, a.x, a.y, a.z, a.w, image, depth, nullptr);
    }
    gsr_select_epilogue(n, i, hit, op, mask, counters);
}

// How many of the first n bits of a mask are set (gsr_transform and gsr_grade count the mask a selection leaves before they write
// anything): one thread per word, bits at and behind n dropped, a wave's sum in ONE atomic on a counter word of the staging arena
// (zeroed in front).  Reads the mask, writes nothing else: a verb returns on a zero count before it has changed anything.
__global__ void __launch_bounds__(256)
k_mask_count(uint32_t n, const uint32_t* __restrict__ mask, uint32_t* __restrict__ count)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, words = (n >> 5) + ((n & 31u) ? 1u : 0u);
    uint32_t set = 0u;
    if (w < words) {
        uint32_t v = mask[w];
        const uint32_t left = n - w * 32u;             // splats from this word's first bit on (>= 1)
        if (left < 32u) v &= (1u << left) - 1u;
        set = (uint32_t)__popc(v);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) set += __shfl_xor(set, d, 64);
    if ((threadIdx.x & 63u) == 0u && set) atomicAdd(count, set);
}
