// k_measure.h -- a selection measured where it is resident (gsr_measure): counts, bounds, first and second moments about
// a reference point, histograms of up to four channels.
//
// THE rule, in one place: every function a result goes through is __host__ __device__ (the ordered key of a float, the terms of a
// splat's moments, a channel's value, the LOG2 replacement, the bin of a value); k_measure and gsr_measure_eval (host) both go through
// them.  The only arithmetic is exact (half -> float, float -> double, a product of two floats in binary64), one f32 subtraction
// per axis (p - ref), the extent's two explicit fmaf, the bin's f32 subtraction and multiply, and binary64 additions in ONE fixed
// order: the perfect binary tree over upload indices (below).  The translation units are compiled with -ffp-contract=off; x86 and
// gfx950 agree in every bit.  No floating-point atomic anywhere: what crosses workgroups is integer (counts, ordered keys, bins) or
// goes through memory to a second launch that keeps the tree's order (k_measure_fold).
// No frame kernel changes, and a context that never measures launches nothing of this file.
#pragma once
#include "k_select_attrs.h"

// gsplat_hip.h's constants (GSR_MEASURE_*, GSR_HIST_*; gsr_resident_measure.h holds the two sets equal)
#define GSR_MEASW_BOUNDS   1
#define GSR_MEASW_EXTENT   2
#define GSR_MEASW_MOMENTS  4
#define GSR_MEASW_ALL      7
#define GSR_MEASF_SKIP_HIDDEN 1
#define GSR_HISTC_X          0
#define GSR_HISTC_Y          1
#define GSR_HISTC_Z          2
#define GSR_HISTC_ALPHA      3
#define GSR_HISTC_SCALE_MAX  4
#define GSR_HISTC_SCALE_MIN  5
#define GSR_HISTC_CD_R       6
#define GSR_HISTC_CD_G       7
#define GSR_HISTC_CD_B       8
#define GSR_HISTC_COUNT      9
#define GSR_HISTF_LOG2       1
#define GSR_MEAS_HISTS       4         // specs per request
#define GSR_MEAS_BINS        256       // bins per spec; behind them: under, over, nan
#define GSR_MEAS_TABLE       (GSR_MEAS_HISTS * (GSR_MEAS_BINS + 3))

// gsr_hist_spec's and gsr_measure_request's layouts (by value in the kernel's argument segment: uniform, in scalar registers)
struct GsrHistSpec {
    int32_t channel, flags, bins;
    float lo, hi, inv_w;
};
struct GsrMeasureRule {
    int32_t what, flags;
    float ref[3];
    float extent_k;
    int32_t n_hist;
    GsrHistSpec hist[GSR_MEAS_HISTS];
    int32_t reserved_;
};
static_assert(sizeof(GsrHistSpec) == 6 * 4 && sizeof(GsrMeasureRule) == 32 * 4, "the request is a run of 32 dwords");

// ---- the ordered key: sign-magnitude bits -> an int32 whose order is the total order of the floats' bits (-0 < +0; its own inverse)
__host__ __device__ __forceinline__ int32_t gsr_meas_key(uint32_t bits)
{
    const int32_t b = (int32_t)bits;
    return b ^ ((b >> 31) & 0x7fffffff);
}
// What the reductions carry: a uint32 that only ever grows, 0 = "no value yet" (no finite or infinite float encodes to 0).  A minimum is
// the maximum of the complemented key.
__host__ __device__ __forceinline__ uint32_t gsr_meas_enc_lo(float x) { return (uint32_t)gsr_meas_key(__builtin_bit_cast(uint32_t, x)) ^ 0x7fffffffu; }
__host__ __device__ __forceinline__ uint32_t gsr_meas_enc_hi(float x) { return (uint32_t)gsr_meas_key(__builtin_bit_cast(uint32_t, x)) ^ 0x80000000u; }
__host__ __device__ __forceinline__ float gsr_meas_dec_lo(uint32_t e) { return __builtin_bit_cast(float, (uint32_t)gsr_meas_key(e ^ 0x7fffffffu)); }
__host__ __device__ __forceinline__ float gsr_meas_dec_hi(uint32_t e) { return __builtin_bit_cast(float, (uint32_t)gsr_meas_key(e ^ 0x80000000u)); }

__host__ __device__ __forceinline__ bool gsr_meas_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
__host__ __device__ __forceinline__ bool gsr_meas_half_finite(uint32_t h) { return (h & 0x7c00u) != 0x7c00u; }

// the largest / smallest |half| of the three scale halves, as gsr_attr_hit forms them (a NaN half: NaN)
__host__ __device__ __forceinline__ void gsr_meas_scales(uint32_t s0, uint32_t s1, uint32_t s2, float* smax, float* smin)
{
    const float a0 = __builtin_fabsf(gsr_attr_h2f(s0)), a1 = __builtin_fabsf(gsr_attr_h2f(s1)), a2 = __builtin_fabsf(gsr_attr_h2f(s2));
    if (!(a0 == a0 && a1 == a1 && a2 == a2)) { *smax = *smin = __builtin_nanf(""); return; }
    const float hi01 = a0 > a1 ? a0 : a1, lo01 = a0 < a1 ? a0 : a1;
    *smax = hi01 > a2 ? hi01 : a2;
    *smin = lo01 < a2 ? lo01 : a2;
}

// the nine binary64 terms of a measured splat: d = p - ref (one f32 subtraction per axis), then d and the exact products
__host__ __device__ __forceinline__ void gsr_meas_terms(const float ref[3], float px, float py, float pz, double t[9])
{
    const float dx = px - ref[0], dy = py - ref[1], dz = pz - ref[2];
    const double x = (double)dx, y = (double)dy, z = (double)dz;
    t[0] = x; t[1] = y; t[2] = z;
    t[3] = x * x; t[4] = x * y; t[5] = x * z;
    t[6] = y * y; t[7] = y * z;
    t[8] = z * z;
}

// a channel's value of one splat
__host__ __device__ __forceinline__ float gsr_meas_channel(int channel, float px, float py, float pz, float a, uint32_t s0, uint32_t s1, uint32_t s2,
                                                           uint32_t c0, uint32_t c1, uint32_t c2)
{
    float smax, smin;
    switch (channel) {
    case GSR_HISTC_X: return px;
    case GSR_HISTC_Y: return py;
    case GSR_HISTC_Z: return pz;
    case GSR_HISTC_ALPHA: return a;
    case GSR_HISTC_SCALE_MAX: gsr_meas_scales(s0, s1, s2, &smax, &smin); return smax;
    case GSR_HISTC_SCALE_MIN: gsr_meas_scales(s0, s1, s2, &smax, &smin); return smin;
    case GSR_HISTC_CD_R: return gsr_attr_h2f(c0);
    case GSR_HISTC_CD_G: return gsr_attr_h2f(c1);
    default: return gsr_attr_h2f(c2);
    }
}

// GSR_HIST_LOG2's replacement of a finite x > 0: piecewise-linear in log2 (the exponent, and the mantissa as its fraction), in
// integer and conversion arithmetic only
__host__ __device__ __forceinline__ float gsr_meas_log2(float x)
{
    return (float)(int32_t)(__builtin_bit_cast(uint32_t, x) - 0x3f800000u) * 0x1p-23f;
}

// Where x counts in a spec's bins + 3 words: [0, bins) the bins, then under, over, nan.  The host has checked the spec (1 <= bins <= 256,
// lo < hi finite, inv_w finite and > 0), so t below is >= 0 or +inf, never a NaN; t >= bins is the clamp (and the only way an
// overflowing x - lo is ever converted).
__host__ __device__ __forceinline__ int gsr_meas_slot(const GsrHistSpec& s, float x)
{
    const int under = s.bins, over = s.bins + 1, nan = s.bins + 2;
    if (!(x == x)) return nan;
    if (s.flags & GSR_HISTF_LOG2) {
        if (!(x > 0.0f)) return under;
        if (!gsr_meas_finite(x)) return over;
        x = gsr_meas_log2(x);
    }
    if (!(x >= s.lo)) return under;
    if (!(x < s.hi)) return over;
    const float t = (x - s.lo) * s.inv_w;
    return t >= (float)s.bins ? s.bins - 1 : (int)t;
}

// (What a lane loads is k_select_attrs' word, GSR_ATTRL_*: the host derives it from the request and the visibility in force.)

// ---- the tree ------------------------------------------------------------------------------------------------------------------------
// Each of the nine sums is the value of the perfect binary tree over upload indices: leaf i holds splat i's term (+0.0 where i is not
// measured or not below n), every inner node is left + right in binary64, and the tree spans 2^k >= max(n, 64) leaves, the smallest
// such.  Binary64 addition commutes in every bit (no NaN payload is at stake below a finite sum), so a butterfly -- every lane adds
// what its partner across 1, 2, 4, 8, 16, 32 lanes holds -- leaves in EVERY lane the node over the wave's 64 consecutive indices: the
// pairs, the order and the roundings are the tree's.  Partners 1 and 2 apart are a quad permute, 4 and 8 apart the half-row and row
// mirrors (after the first two steps all lanes of a quad hold one value, after three all of a half row: the mirror image of a lane
// lies in the partner group), all DPP moves with no LDS traffic; 16 and 32 apart go through ds_bpermute.
template <int D>
__device__ __forceinline__ int gsr_meas_partner(int v)
{
    if constexpr (D == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);        // quad_perm [1, 0, 3, 2]
    else if constexpr (D == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);   // quad_perm [2, 3, 0, 1]
    else if constexpr (D == 4) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    else if constexpr (D == 8) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);  // row_mirror
    else return __shfl_xor(v, D, 64);
}
template <int D>
__device__ __forceinline__ double gsr_meas_step(double v)
{
    const double o = __hiloint2double(gsr_meas_partner<D>(__double2hiint(v)), gsr_meas_partner<D>(__double2loint(v)));
    return v + o;
}
// the node over the first `span` (a power of two, 1..64) lanes' values, in lane 0 (span = 64: in every lane).  Every lane of the wave
// must be here.
__device__ __forceinline__ double gsr_meas_wave_tree(double v, int span = 64)
{
    if (span > 1) v = gsr_meas_step<1>(v);
    if (span > 2) v = gsr_meas_step<2>(v);
    if (span > 4) v = gsr_meas_step<4>(v);
    if (span > 8) v = gsr_meas_step<8>(v);
    if (span > 16) v = gsr_meas_step<16>(v);
    if (span > 32) v = gsr_meas_step<32>(v);
    return v;
}
__device__ __forceinline__ uint32_t gsr_meas_wave_max(uint32_t v)
{
    uint32_t o;
    o = (uint32_t)gsr_meas_partner<1>((int)v); v = v > o ? v : o;
    o = (uint32_t)gsr_meas_partner<2>((int)v); v = v > o ? v : o;
    o = (uint32_t)gsr_meas_partner<4>((int)v); v = v > o ? v : o;
    o = (uint32_t)gsr_meas_partner<8>((int)v); v = v > o ? v : o;
    o = (uint32_t)gsr_meas_partner<16>((int)v); v = v > o ? v : o;
    o = (uint32_t)gsr_meas_partner<32>((int)v); v = v > o ? v : o;
    return v;
}
__device__ __forceinline__ uint32_t gsr_meas_wave_add(uint32_t v)
{
    v += (uint32_t)gsr_meas_partner<1>((int)v);
    v += (uint32_t)gsr_meas_partner<2>((int)v);
    v += (uint32_t)gsr_meas_partner<4>((int)v);
    v += (uint32_t)gsr_meas_partner<8>((int)v);
    v += (uint32_t)gsr_meas_partner<16>((int)v);
    v += (uint32_t)gsr_meas_partner<32>((int)v);
    return v;
}
// the node over a workgroup's `waves` (1, 2 or 4) first wave nodes
__device__ __forceinline__ double gsr_meas_join(double (*w)[9], int k, int waves)
{
    return waves >= 4 ? (w[0][k] + w[1][k]) + (w[2][k] + w[3][k]) : waves == 2 ? w[0][k] + w[1][k] : w[0][k];
}

// ---- the result block (uint32 words; zeroed in front of the launch) ------------------------------------------------------------------
#define GSR_MEAS_R_COUNTS  0           // n_selected, n_measured, n_extent
#define GSR_MEAS_R_BOUNDS  4           // enc_lo[3], enc_hi[3], then the extent's enc_lo[3], enc_hi[3]
#define GSR_MEAS_R_SUMS    16          // nine doubles (byte 64)
#define GSR_MEAS_R_HIST    36          // the specs' bins + 3 words, back to back
#define GSR_MEAS_R_WORDS   (GSR_MEAS_R_HIST + GSR_MEAS_TABLE)

// One thread per UPLOAD index i and 256 per chunk, k_select's shape; a workgroup takes the chunks blockIdx.x, blockIdx.x + gridDim.x,
// ... (the host caps the grid at GSR_MEASURE_BLOCKS, what the device holds at once, so that what leaves a workgroup through atomics
// -- three counts, up to twelve keys, the non-zero words of its histogram table -- leaves it once and not once per 256 splats).
// A lane whose mask bit is clear loads nothing; a wave whose 64 bits are clear goes to the chunk's tree with zeros.  A selected lane
// gathers through j = inv[i] (inv: upload index -> storage slot; NULL: upload order) only the planes `loads` names (uniform: scalar
// branches).  Per chunk the nine terms go up the tree: the wave's butterfly, the four wave nodes through LDS (two buffers by the
// parity of the trip, so one barrier per chunk), and the chunk's node to partials[chunk][9] with a plain store; k_measure_fold takes
// the tree on from there.  top_waves (1, 2, 4): how many wave nodes the tree of a cloud of at most 64, 128, or more splats joins.
// Counts and keys stay in registers over the chunks and leave at the end: a wave reduction, the four waves through LDS, then one
// integer atomic per value that says something.  Histograms: a workgroup-private LDS table, zeroed, filled with LDS atomic adds,
// flushed with one global atomicAdd per non-zero word.
#define GSR_MEASURE_THREADS 256
#define GSR_MEASURE_BLOCKS  2048
static_assert(GSR_MEASURE_THREADS == GSR_SELECT_THREADS, "a chunk of k_measure is a workgroup of k_select");
__global__ void __launch_bounds__(GSR_MEASURE_THREADS, 8)   // (eight waves per SIMD: at most 64 VGPRs, so GSR_MEASURE_BLOCKS workgroups are resident at once)
k_measure(uint32_t n, uint32_t nchunks, int loads, int top_waves, const uint32_t* __restrict__ inv, const float4* __restrict__ geoA,
          const uint4* __restrict__ geoB, const uint4* __restrict__ col, const float* __restrict__ alpha0,
          const uint32_t* __restrict__ vis_mask /* NULL: none */, const uint32_t* __restrict__ mask /* NULL: every splat */, GsrMeasureRule rq,
          GsrVisRule vis, uint32_t* __restrict__ res, double* __restrict__ partials)
{
    __shared__ uint32_t s_hist[GSR_MEAS_TABLE];
    __shared__ double s_tree[2][4][9];
    __shared__ uint32_t s_fin[4][16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int what = rq.what, n_hist = rq.n_hist;
    int hoff[GSR_MEAS_HISTS + 1];
    hoff[0] = 0;
#pragma unroll
    for (int h = 0; h < GSR_MEAS_HISTS; ++h) hoff[h + 1] = hoff[h] + (h < n_hist ? rq.hist[h].bins + 3 : 0);
    const int table = hoff[GSR_MEAS_HISTS];              // <= GSR_MEAS_TABLE: the host has checked every spec
    if (n_hist) {
        for (int t = (int)threadIdx.x; t < table; t += GSR_MEASURE_THREADS) s_hist[t] = 0u;
        __syncthreads();
    }
    uint32_t fin[15];                                    // three counts, then the twelve encoded keys: all 0 = nothing yet
#pragma unroll
    for (int k = 0; k < 15; ++k) fin[k] = 0u;
    uint32_t trip = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x, ++trip) {
        const uint32_t i = chunk * (uint32_t)GSR_MEASURE_THREADS + threadIdx.x;
        bool sel = i < n && (mask ? ((mask[i >> 5] >> (i & 31u)) & 1u) != 0u : true);
        double t[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = 0.0;
        if (__ballot(sel)) {                             // (wave-uniform)
            if (sel) {
                const bool gathers = (loads & (GSR_ATTRL_GEOA | GSR_ATTRL_GEOB | GSR_ATTRL_COL)) != 0;
                const uint32_t j = gathers && inv ? inv[i] : i;
                float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                uint4 b = make_uint4(0u, 0u, 0u, 0u), c = make_uint4(0u, 0u, 0u, 0u);
                if (loads & GSR_ATTRL_GEOA) a = geoA[j];
                if (loads & GSR_ATTRL_GEOB) b = geoB[j];
                if (loads & GSR_ATTRL_COL) c = col[j];
                const float alpha = (loads & GSR_ATTRL_ALPHA0) ? alpha0[i] : a.w;
                if ((loads & GSR_ATTRL_HIDDEN) && !gsr_splat_visible(vis, a.x, a.y, a.z, vis_mask ? vis_mask[i >> 5] : 0u, i)) sel = false;
                if (sel) {
                    const uint32_t s0 = b.x & 0xffffu, s1 = b.x >> 16, s2 = b.y & 0xffffu;
                    fin[0] += 1u;
                    if (what & GSR_MEASW_ALL) {
                        if (gsr_meas_finite(a.x) && gsr_meas_finite(a.y) && gsr_meas_finite(a.z)) {
                            fin[1] += 1u;
                            const float p[3] = {a.x, a.y, a.z};
                            if (what & GSR_MEASW_BOUNDS) {
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                    const uint32_t lo = gsr_meas_enc_lo(p[k]), hi = gsr_meas_enc_hi(p[k]);
                                    fin[3 + k] = fin[3 + k] > lo ? fin[3 + k] : lo;
                                    fin[6 + k] = fin[6 + k] > hi ? fin[6 + k] : hi;
                                }
                            }
                            if ((what & GSR_MEASW_EXTENT) && gsr_meas_half_finite(s0) && gsr_meas_half_finite(s1) && gsr_meas_half_finite(s2)) {
                                fin[2] += 1u;
                                float smax, smin;
                                gsr_meas_scales(s0, s1, s2, &smax, &smin);
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                    const uint32_t lo = gsr_meas_enc_lo(__builtin_fmaf(-rq.extent_k, smax, p[k]));
                                    const uint32_t hi = gsr_meas_enc_hi(__builtin_fmaf(rq.extent_k, smax, p[k]));
                                    fin[9 + k] = fin[9 + k] > lo ? fin[9 + k] : lo;
                                    fin[12 + k] = fin[12 + k] > hi ? fin[12 + k] : hi;
                                }
                            }
                            if (what & GSR_MEASW_MOMENTS) gsr_meas_terms(rq.ref, a.x, a.y, a.z, t);
                        }
                    }
#pragma unroll
                    for (int h = 0; h < GSR_MEAS_HISTS; ++h) {
                        if (h < n_hist) {
                            const float x = gsr_meas_channel(rq.hist[h].channel, a.x, a.y, a.z, alpha, s0, s1, s2, c.x & 0xffffu, c.x >> 16, c.y & 0xffffu);
                            atomicAdd(&s_hist[hoff[h] + gsr_meas_slot(rq.hist[h], x)], 1u);
                        }
                    }
                }
            }
            if (what & GSR_MEASW_MOMENTS) {              // (every lane of the wave is here again)
#pragma unroll
                for (int k = 0; k < 9; ++k) t[k] = gsr_meas_wave_tree(t[k]);
            }
        }
        if (what & GSR_MEASW_MOMENTS) {
            double (*const w)[9] = s_tree[trip & 1u];
            if (lane == 0u) {
#pragma unroll
                for (int k = 0; k < 9; ++k) w[wave][k] = t[k];
            }
            __syncthreads();
            if (threadIdx.x < 9u) partials[(size_t)chunk * 9u + threadIdx.x] = gsr_meas_join(w, (int)threadIdx.x, top_waves);
        }
    }
    // ---- what the workgroup has to say: the counts and keys of its lanes, its histogram table
    fin[0] = gsr_meas_wave_add(fin[0]);
    fin[1] = gsr_meas_wave_add(fin[1]);
    fin[2] = gsr_meas_wave_add(fin[2]);
#pragma unroll
    for (int k = 3; k < 15; ++k) fin[k] = gsr_meas_wave_max(fin[k]);
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 15; ++k) s_fin[wave][k] = fin[k];
    }
    __syncthreads();                                     // (also: every LDS atomic of the table has landed)
    if (threadIdx.x < 15u) {
        const uint32_t k = threadIdx.x, v0 = s_fin[0][k], v1 = s_fin[1][k], v2 = s_fin[2][k], v3 = s_fin[3][k];
        if (k < 3u) {
            const uint32_t v = v0 + v1 + v2 + v3;
            if (v) atomicAdd(res + GSR_MEAS_R_COUNTS + k, v);
        } else {
            const uint32_t m01 = v0 > v1 ? v0 : v1, m23 = v2 > v3 ? v2 : v3, v = m01 > m23 ? m01 : m23;
            if (v) atomicMax(res + GSR_MEAS_R_BOUNDS + (k - 3u), v);
        }
    }
    for (int t = (int)threadIdx.x; t < table; t += GSR_MEASURE_THREADS) {
        const uint32_t v = s_hist[t];
        if (v) atomicAdd(res + GSR_MEAS_R_HIST + t, v);
    }
}

// The tree above the chunks: workgroup g joins entries [256 g, 256 g + 256) of `in` (m entries of nine doubles; +0.0 behind them) into
// out[g][9] -- the butterfly, then the four wave nodes through LDS.  span = 256, or, in the last launch (one workgroup), the power of
// two the tree still spans (1..256): the node over exactly that many entries, so that no +0.0 from behind the tree is ever added.
__global__ void __launch_bounds__(256)
k_measure_fold(uint32_t m, int span, const double* __restrict__ in, double* __restrict__ out)
{
    __shared__ double s_tree[4][9];
    const uint32_t e = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = e < m ? in[(size_t)e * 9u + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = gsr_meas_wave_tree(t[k], span < 64 ? span : 64);
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_tree[wave][k] = t[k];
    }
    __syncthreads();
    if (threadIdx.x < 9u) out[(size_t)blockIdx.x * 9u + threadIdx.x] = gsr_meas_join(s_tree, (int)threadIdx.x, span >= 256 ? 4 : span == 128 ? 2 : 1);
}
