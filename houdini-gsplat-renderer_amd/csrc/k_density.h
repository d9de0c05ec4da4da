// k_density.h -- resident splats selected by how many neighbours they have (gsr_select_density): the floaters of a
// capture, a trainer's density prune.
//
// THE rule, in one place: gsr_density_axis / gsr_density_class (the cell of a splat and whether it is population), gsr_density_row
// (which key range a neighbouring row of cells is) and gsr_density_hit (the verdict over a count) are __host__ __device__, as
// gsr_select_hit and gsr_attr_hit are; the kernels and gsr_select_density_eval (host) all go through them.  The only float
// arithmetic is one f32 subtraction and one f32 multiplication per axis (never fused: the translation units are compiled with
// -ffp-contract=off, and no fmaf is written) and a floorf; every range test is made on the float, before any conversion.  Everything
// behind the cell is integer arithmetic: x86 and gfx950 agree in every bit.  No frame kernel changes, and a context that never selects
// by density launches nothing of this file.
#pragma once
#include "k_select.h"

// the flags of gsplat_hip.h (GSR_DENSITY_*; gsr_resident_select.h holds the two sets equal)
#define GSR_DENF_SKIP_HIDDEN 1
#define GSR_DENF_HIT_OUTSIDE 2
#define GSR_DEN_CELLS   1024           // cells per axis: a key is ix | iy << 10 | iz << 20, x fastest (NOT Morton: a row of cells is one key range)
#define GSR_DEN_NOKEY   (1u << 30)     // what k_density_keys writes for a splat that is not population: sorts behind every key
#define GSR_DEN_NONE    GSR_DEN_NOKEY          // gsr_density_class: neither population nor outside
#define GSR_DEN_OUTSIDE (GSR_DEN_NOKEY | 1u)   // gsr_density_class: passes the alpha and visibility tests, not in the grid
#define GSR_DEN_CNT_OUTSIDE 0x80000000u        // the bit of a count word that says "outside" (a count is at most n < 2^31)
#define GSR_DEN_BINS    64             // count_hist: bin b < 63 holds N == b + 1, bin 63 holds N >= 64

// the rule as the kernels take it (by value in the argument segment: uniform).  inv_cell = 1.0f / cell, one IEEE division on the host:
// no kernel divides.
struct GsrDensityRule {
    float inv_cell;
    float origin[3];
    int32_t reach, flags, op;
    uint32_t count_lo, count_hi;
    float alpha_min;
};

// the words of the result block the kernels count into (uint32 each; [0] and [1] leave a workgroup as ONE 64-bit atomic)
#define GSR_DEN_R_POP     0
#define GSR_DEN_R_OUTSIDE 1
#define GSR_DEN_R_CELLS   2
#define GSR_DEN_R_HIST    4
#define GSR_DEN_R_WORDS   (GSR_DEN_R_HIST + GSR_DEN_BINS)

// One axis of the cell rule: t = (p - o) * inv in two roundings, f = floorf(t); in the grid iff 0 <= f < 1024, tested on the FLOAT --
// a NaN, an infinity or a huge t fails the comparison and never reaches the conversion.  (-0.0f is cell 0.)
__host__ __device__ __forceinline__ bool gsr_density_axis(float p, float o, float inv, uint32_t* cell)
{
    const float d = p - o;
    const float t = d * inv;
    const float f = __builtin_floorf(t);
    if (!(0.0f <= f && f < (float)GSR_DEN_CELLS)) return false;
    *cell = (uint32_t)(int)f;
    return true;
}

// What a splat is to the rule: its key (< 2^30) if it is population, GSR_DEN_OUTSIDE if it passes the alpha and visibility tests but
// lies outside the grid, GSR_DEN_NONE otherwise.  (px, py, pz): the raw position bits, what geoA holds; a: its TRUE alpha (a NaN is
// never population); hidden: the visibility in force hides it (false without one).
__host__ __device__ __forceinline__ uint32_t gsr_density_class(const GsrDensityRule& r, float px, float py, float pz, float a, bool hidden)
{
    if (!(a >= r.alpha_min)) return GSR_DEN_NONE;
    if ((r.flags & GSR_DENF_SKIP_HIDDEN) && hidden) return GSR_DEN_NONE;
    uint32_t ix = 0u, iy = 0u, iz = 0u;
    const bool inx = gsr_density_axis(px, r.origin[0], r.inv_cell, &ix);
    const bool iny = gsr_density_axis(py, r.origin[1], r.inv_cell, &iy);
    const bool inz = gsr_density_axis(pz, r.origin[2], r.inv_cell, &iz);
    return inx && iny && inz ? (ix | iy << 10 | iz << 20) : GSR_DEN_OUTSIDE;
}

// The row of cells (iy + dy, iz + dz) around the cell of `key`, clamped in x to the grid: keys *lo .. *hi inclusive.  false: the row
// does not exist (outside 0..1023 in y or z).  Without the clamp ix = 1023, +1 would alias into (0, iy + 1).
__host__ __device__ __forceinline__ bool gsr_density_row(uint32_t key, int reach, int dy, int dz, uint32_t* lo, uint32_t* hi)
{
    const int ix = (int)(key & 1023u), y = (int)((key >> 10) & 1023u) + dy, z = (int)(key >> 20) + dz;
    if (y < 0 || y >= GSR_DEN_CELLS || z < 0 || z >= GSR_DEN_CELLS) return false;
    const int x0 = ix - reach < 0 ? 0 : ix - reach, x1 = ix + reach >= GSR_DEN_CELLS ? GSR_DEN_CELLS - 1 : ix + reach;
    const uint32_t base = (uint32_t)y << 10 | (uint32_t)z << 20;
    *lo = base | (uint32_t)x0;
    *hi = base | (uint32_t)x1;
    return true;
}

// The verdict over a count word: an outside splat by the flag; a population splat (N >= 1: it counts itself) by the range, compared as
// unsigned integers; everything else (N == 0) never.
__host__ __device__ __forceinline__ bool gsr_density_hit(const GsrDensityRule& r, uint32_t word)
{
    if (word & GSR_DEN_CNT_OUTSIDE) return (r.flags & GSR_DENF_HIT_OUTSIDE) != 0;
    return word != 0u && r.count_lo <= word && word <= r.count_hi;
}

// the bin of count_hist a count N >= 1 falls into
__host__ __device__ __forceinline__ uint32_t gsr_density_bin(uint32_t N) { return (N < (uint32_t)GSR_DEN_BINS ? N : (uint32_t)GSR_DEN_BINS) - 1u; }

#define GSR_DENSITY_THREADS GSR_SELECT_THREADS

// The grid of k_density_keys and k_density_count is capped: workgroup b takes the 256-index chunks b, b + grid, .. and sends its counts
// once, at its end.  With one workgroup per chunk the 23 k workgroups of a 6 M cloud queue as many atomics on ONE address (k_visibility.h
// records what that costs; here it was two thirds of k_density_keys' time).
#define GSR_DENSITY_BLOCKS 2048
#define GSR_DEN_ROWS (2 * 2 + 1)       // the rows of one z plane at the largest reach

// One thread per UPLOAD index i, k_select's gather: geoA[inv ? inv[i] : i], and alpha0[i] / the visibility's mask word when a
// visibility is in force.  Writes key[i] (GSR_DEN_NOKEY for what is not population), val[i] = i, and cnt[i] = 0 or GSR_DEN_CNT_OUTSIDE
// -- every word of cnt, so nothing is cleared in front and k_density_hit knows an outside splat without a second gather.  The two
// counts are ballots summed over a wave's chunks; they leave a workgroup as ONE 64-bit integer atomic (population in the low word,
// outside in the high one: neither can carry, each is at most n < 2^31).
__global__ void __launch_bounds__(GSR_DENSITY_THREADS)
k_density_keys(uint32_t n, uint32_t nchunks, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA, const float* __restrict__ alpha0 /* NULL: geoA's */,
               const uint32_t* __restrict__ vis_mask /* NULL: none */, int hide, GsrDensityRule rule, GsrVisRule vis,
               uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ cnt, uint32_t* __restrict__ res)
{
    __shared__ unsigned long long s_counts;
    if (threadIdx.x == 0u) s_counts = 0ull;
    __syncthreads();
    unsigned long long counts = 0ull;                  // (wave-uniform)
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint32_t i = chunk * (uint32_t)GSR_DENSITY_THREADS + threadIdx.x;
        uint32_t cls = GSR_DEN_NONE;
        if (i < n) {
            const float4 a = geoA[inv ? inv[i] : i];
            const float alpha = alpha0 ? alpha0[i] : a.w;
            const bool hidden = hide && !gsr_splat_visible(vis, a.x, a.y, a.z, vis_mask ? vis_mask[i >> 5] : 0u, i);
            cls = gsr_density_class(rule, a.x, a.y, a.z, alpha, hidden);
            key[i] = cls < GSR_DEN_NOKEY ? cls : GSR_DEN_NOKEY;
            val[i] = i;
            cnt[i] = cls == GSR_DEN_OUTSIDE ? GSR_DEN_CNT_OUTSIDE : 0u;
        }
        const unsigned long long pop = __ballot(cls < GSR_DEN_NOKEY), out = __ballot(cls == GSR_DEN_OUTSIDE);
        counts += (unsigned long long)__popcll(pop) | ((unsigned long long)__popcll(out) << 32);
    }
    if ((threadIdx.x & 63u) == 0u && counts) atomicAdd(&s_counts, counts);
    __syncthreads();
    if (threadIdx.x == 0u && s_counts) atomicAdd(reinterpret_cast<unsigned long long*>(res + GSR_DEN_R_POP), s_counts);
}

// One thread per SORTED entry j < n_pop (the device word k_density_keys counted; the sentinels sort behind it): N = the sum, over the
// (2 reach + 1)^2 rows that exist, of upper_bound - lower_bound of the row's clamped key range in keys[0, n_pop).
// A binary search is a chain of dependent loads, and a wave that runs 2 (2 reach + 1)^2 of them one after the other waits for
// 18 x 23 (reach 1, 6 M keys) round trips to the cache.  So the searches of one z plane -- up to five rows, two bounds each -- advance
// in LOCK STEP: the branchless form (pos += s iff keys[pos + s - 1] < k, s = the powers of two from the largest <= n_pop down) takes the
// same number of steps for every search, each step issues all its loads before it looks at one, and the chain is 23 per plane.  A row
// that does not exist, or lies beyond the reach (uniform), searches for key 0 twice: both bounds stay 0.  Every index is clamped into
// [0, n_pop), so no load depends on a comparison.  Neighbouring threads hold equal or adjacent keys: the loads of a wave fall into the
// same cache lines.  cnt[val[j]] = N is one scattered dword; count_hist is privatised in LDS over the workgroup's chunks, occupied cells
// (key[j] != key[j - 1]) are ballots; both leave once per workgroup; integer atomics only.  No scratch: every array below is indexed by
// unrolled constants.
__global__ void __launch_bounds__(GSR_DENSITY_THREADS)
k_density_count(uint32_t n, uint32_t nchunks, int reach, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                uint32_t* __restrict__ cnt, uint32_t* __restrict__ res)
{
    __shared__ uint32_t s_hist[GSR_DEN_BINS];
    __shared__ uint32_t s_cells;
    if (threadIdx.x < (uint32_t)GSR_DEN_BINS) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == (uint32_t)GSR_DEN_BINS) s_cells = 0u;
    __syncthreads();
    const uint32_t counted = res[GSR_DEN_R_POP], n_pop = counted < n ? counted : n;
    const uint32_t top = n_pop ? 1u << (31 - __clz((int)n_pop)) : 0u;      // the largest power of two <= n_pop
    uint32_t cells = 0u;                               // (wave-uniform)
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_DENSITY_THREADS >= n_pop) break;          // (uniform: only sentinels from here on)
        const uint32_t j = chunk * (uint32_t)GSR_DENSITY_THREADS + threadIdx.x;
        bool first = false;
        if (j < n_pop) {
            const uint32_t key = keys[j];
            first = j == 0u || keys[j - 1u] != key;
            uint32_t N = 0u;
            for (int dz = -reach; dz <= reach; ++dz) {
                uint32_t klo[GSR_DEN_ROWS], kend[GSR_DEN_ROWS], plo[GSR_DEN_ROWS], pend[GSR_DEN_ROWS];
#pragma unroll
                for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                    const int dy = r - 2;
                    uint32_t a = 0u, b = 0u;
                    const bool on = dy >= -reach && dy <= reach && gsr_density_row(key, reach, dy, dz, &a, &b);
                    klo[r] = on ? a : 0u;
                    kend[r] = on ? b + 1u : 0u;        // (b + 1 <= 2^30: no wrap)
                    plo[r] = pend[r] = 0u;
                }
                for (uint32_t s = top; s; s >>= 1) {
                    uint32_t va[GSR_DEN_ROWS], vb[GSR_DEN_ROWS];
#pragma unroll
                    for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                        va[r] = vb[r] = 0u;
                        if (r - 2 >= -reach && r - 2 <= reach) {            // (uniform)
                            const uint32_t ta = plo[r] + s, tb = pend[r] + s;   // (>= 1; below 2^32: a position is below 2^31, s at most 2^30)
                            va[r] = keys[(ta < n_pop ? ta : n_pop) - 1u];
                            vb[r] = keys[(tb < n_pop ? tb : n_pop) - 1u];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                        const uint32_t ta = plo[r] + s, tb = pend[r] + s;
                        if (ta <= n_pop && va[r] < klo[r]) plo[r] = ta;
                        if (tb <= n_pop && vb[r] < kend[r]) pend[r] = tb;
                    }
                }
#pragma unroll
                for (int r = 0; r < GSR_DEN_ROWS; ++r) N += pend[r] - plo[r];
            }
            const uint32_t v = vals[j];
            if (v < n) cnt[v] = N;
            if (N) atomicAdd(&s_hist[gsr_density_bin(N)], 1u);
        }
        cells += (uint32_t)__popcll(__ballot(first));
    }
    if ((threadIdx.x & 63u) == 0u && cells) atomicAdd(&s_cells, cells);
    __syncthreads();
    if (threadIdx.x < (uint32_t)GSR_DEN_BINS && s_hist[threadIdx.x]) atomicAdd(res + GSR_DEN_R_HIST + threadIdx.x, s_hist[threadIdx.x]);
    if (threadIdx.x == (uint32_t)GSR_DEN_BINS && s_cells) atomicAdd(res + GSR_DEN_R_CELLS, s_cells);
}

// One thread per UPLOAD index i: the count word of i, the verdict, N into counts_out (the outside bit stripped; NULL: skipped), and
// k_select's epilogue unchanged.
__global__ void __launch_bounds__(GSR_DENSITY_THREADS)
k_density_hit(uint32_t n, GsrDensityRule rule, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ counts_out /* NULL: none */,
              uint32_t* __restrict__ mask, unsigned long long* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * (uint32_t)GSR_DENSITY_THREADS + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t word = cnt[i];
        hit = gsr_density_hit(rule, word);
        if (counts_out) counts_out[i] = word & ~GSR_DEN_CNT_OUTSIDE;
    }
    gsr_select_epilogue(n, i, hit, rule.op, mask, counters);
}
