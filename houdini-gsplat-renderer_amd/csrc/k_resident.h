// k_resident.h -- K0: the kernels that write, edit and re-order the RESIDENT layout.  They run once per geometry
// change, never per frame: k_pack (upload), k_update / k_update_f32 + k_cluster_extents (gsr_update, gsr_update_device),
// k_move_positions + k_repack / k_cluster_bounds (gsr_move), k_quantize_raw (raw float32 attributes); k_add.h and k_read.h build on
// the pieces below.
//
// THE LAYOUT.  n splats in `cap` slots, in storage order (slot j holds the splat perm[j] of the upload; inv is the inverse):
//   geoA[j]       float4  P.xyz, opacity
//   geoB[j]       uint4   eight halves: scale.xyz, orient.ijkr, and an upper bound of the splat's extent (gsr_extent_half)
//   col[c][j]     uint4   chunk c = 0..5 of the 48 colour halves Cd.rgb, sh1.rgb, .., sh15.rgb (half h = 3 * coefficient + channel),
//                         chunks strided by the capacity; without SH only chunk 0 exists, and only its halves 0..2 are not zero
//   colrow[j][8]  uint4   SH only: ONE 128-byte line per splat = geoA[j], the six colour chunks, 16 bytes of zeros
//   clusA/clusB   float4  per cluster of 64 slots: lo.xyz of the positions + the largest extent bound; hi.xyz + the "never cull" flag
// THE WORK SHAPE.  A workgroup of GSR_PACK_THREADS = 512 covers 64 splats (with k_pack, k_repack, k_add_pack: one cluster), eight
// lanes per splat, all eight in one wave.  Lane q of a splat carries one 16-byte PIECE of it:
//   q = 0      geoA: P + opacity; it also brings the three Cd halves into the LDS row
//   q = 1..6   colour chunk q - 1; SH sources arrive as x / y / z rows of 16 halves (coefficient co at flat index co - 1), so the lanes
//              put 16 bytes each into the splat's LDS row  x[16] y[16] z[16] Cd[3] (+ pad: 112-byte rows)  and read their chunk back
//              out of it: a 16 x 3 -> 3 x 16 transpose.  Without SH only lane 1 has a chunk
//   q = 7      geoB: scale + orient + the extent half; its eighth of the colrow line is the padding
//   every q    piece q of the colrow line: a wave moves eight whole 128-byte lines in one instruction
// The LDS row is written and read by the splat's own wave only, so gsr_wave_lds_sync() between the two is all it needs.
// Every verb promises planes and bounds that are bit for bit those of a fresh upload of the edited arrays; that holds because each
// rule below is written once and every kernel goes through it.
#pragma once
#include "gsr_device.h"
#include "k_cluster.h"

#define GSR_PACK_THREADS 512
#define GSR_ROW_HALVES 56          // halves of a splat's LDS row: x[16] y[16] z[16] Cd[3] + pad

__device__ __forceinline__ uint32_t gsr_pk(uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }
__device__ __forceinline__ uint16_t gsr_lo16(uint32_t w) { return (uint16_t)(w & 0xffffu); }
__device__ __forceinline__ uint16_t gsr_hi16(uint32_t w) { return (uint16_t)(w >> 16); }
__device__ __forceinline__ uint4 gsr_as_uint4(float4 a) { return make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w)); }
__device__ __forceinline__ float4 gsr_as_float4(uint4 p) { return make_float4(__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), __uint_as_float(p.w)); }
__device__ __forceinline__ uint16_t gsr_f2h(float f)
{
    const _Float16 h = (_Float16)f;      // v_cvt_f16_f32: round to nearest even
    return __builtin_bit_cast(uint16_t, h);
}
// a source value as the resident half: staged halves as they are, float32 sources quantised in registers
__device__ __forceinline__ uint16_t gsr_src_half(uint16_t h) { return h; }
__device__ __forceinline__ uint16_t gsr_src_half(float f) { return gsr_f2h(f); }

// between the writes and the reads of the LDS rows (a splat's eight lanes sit in one wave: no workgroup barrier)
__device__ __forceinline__ void gsr_wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------
// geoB.  Its eighth half is an upper bound of |diag(scale) R(orient)^T|_F, the only thing K1's cheap extent bound needs of the
// scale and the (unnormalised) quaternion -- so the bound costs a dozen instructions per splat instead of ninety.
__device__ __forceinline__ uint16_t gsr_extent_half(uint16_t s0, uint16_t s1, uint16_t s2, uint16_t o0, uint16_t o1, uint16_t o2, uint16_t o3)
{
    const float sx = gsr_h2f(s0), sy = gsr_h2f(s1), sz = gsr_h2f(s2);
    const float qi = gsr_h2f(o0), qj = gsr_h2f(o1), qk = gsr_h2f(o2), qr = gsr_h2f(o3);
    const float r00 = 1.0f - 2.0f * gsr_fma(qj, qj, qk * qk), r01 = 2.0f * gsr_fma(qi, qj, -(qr * qk)), r02 = 2.0f * gsr_fma(qi, qk, qr * qj);
    const float r10 = 2.0f * gsr_fma(qi, qj, qr * qk), r11 = 1.0f - 2.0f * gsr_fma(qi, qi, qk * qk), r12 = 2.0f * gsr_fma(qj, qk, -(qr * qi));
    const float r20 = 2.0f * gsr_fma(qi, qk, -(qr * qj)), r21 = 2.0f * gsr_fma(qj, qk, qr * qi), r22 = 1.0f - 2.0f * gsr_fma(qi, qi, qj * qj);
    const float mf2 = sx * sx * (r00 * r00 + r10 * r10 + r20 * r20) + sy * sy * (r01 * r01 + r11 * r11 + r21 * r21) +
                      sz * sz * (r02 * r02 + r12 * r12 + r22 * r22);
    const float mfv = __builtin_sqrtf(mf2) * 1.001f;
    const _Float16 hh = (_Float16)mfv;              // rounded up (to nearest, then one step if that fell short): mf >= 0
    uint16_t mf_h = __builtin_bit_cast(uint16_t, hh);
    if ((float)hh < mfv) mf_h += 1;                 // (0x7bff + 1 = inf; inf / NaN stay what they are: K1 then takes the full path)
    return mf_h;
}
struct GsrShape { uint16_t s0, s1, s2, o0, o1, o2, o3; };      // the seven halves of geoB that are given; the eighth is derived
__device__ __forceinline__ GsrShape gsr_shape_split(uint4 b)
{
    return GsrShape{gsr_lo16(b.x), gsr_hi16(b.x), gsr_lo16(b.y), gsr_hi16(b.y), gsr_lo16(b.z), gsr_hi16(b.z), gsr_lo16(b.w)};
}
__device__ __forceinline__ uint4 gsr_shape_join(const GsrShape& h)
{
    return make_uint4(gsr_pk(h.s0, h.s1), gsr_pk(h.s2, h.o0), gsr_pk(h.o1, h.o2), gsr_pk(h.o3, gsr_extent_half(h.s0, h.s1, h.s2, h.o0, h.o1, h.o2, h.o3)));
}
// rows t of source arrays (staged halves, or the caller's float32) -> the LDS row's Cd slots / the shape's halves
template <typename T> __device__ __forceinline__ void gsr_load_cd(const T* Cd, size_t t, uint16_t* row)
{
    const T* c = Cd + 3 * t;
    row[48] = gsr_src_half(c[0]); row[49] = gsr_src_half(c[1]); row[50] = gsr_src_half(c[2]);
}
template <typename T> __device__ __forceinline__ void gsr_load_scale(const T* scale, size_t t, GsrShape& h)
{
    const T* s = scale + 3 * t;
    h.s0 = gsr_src_half(s[0]); h.s1 = gsr_src_half(s[1]); h.s2 = gsr_src_half(s[2]);
}
template <typename T> __device__ __forceinline__ void gsr_load_orient(const T* orient, size_t t, GsrShape& h)
{
    const T* o = orient + 4 * t;
    h.o0 = gsr_src_half(o[0]); h.o1 = gsr_src_half(o[1]); h.o2 = gsr_src_half(o[2]); h.o3 = gsr_src_half(o[3]);
}

// ---------------------------------------------------------------------------
// The colours.  Where things sit in a splat's LDS row x[16] y[16] z[16] Cd[3]:
//   float f = 3 * slot + channel of a splat's `3 * vpp` float32 SH row (slot = coefficient - 1)
__device__ __forceinline__ int gsr_sh_float_slot(int f)
{
    const int slot = f / 3, chn = f - 3 * slot;
    return 16 * chn + slot;
}
//   half k of colour chunk c: half hh = 8 c + k of the 48 is coefficient co = hh / 3 (0 = Cd), channel chn = hh - 3 co
__device__ __forceinline__ int gsr_colour_half_slot(int c, int k)
{
    const int hh = 8 * c + k, co = hh / 3, chn = hh - 3 * co;
    return co == 0 ? 48 + chn : 16 * chn + (co - 1);
}
template <bool SH> __device__ __forceinline__ bool gsr_colour_lane(int q) { return q >= 1 && (SH ? q <= 6 : q == 1); }
// chunk c out of the row: the 16 x 3 -> 3 x 16 transpose (without SH the row holds Cd alone, and every other half is zero)
template <bool SH>
__device__ __forceinline__ uint4 gsr_colour_chunk(const uint16_t* row, int c)
{
    uint16_t h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int at = gsr_colour_half_slot(c, k);
        h[k] = (SH || at >= 48) ? row[at] : (uint16_t)0;
    }
    return make_uint4(gsr_pk(h[0], h[1]), gsr_pk(h[2], h[3]), gsr_pk(h[4], h[5]), gsr_pk(h[6], h[7]));
}
// lanes 1..6 bring x[0..7] x[8..15] y[0..7] y[8..15] z[0..7] z[8..15] of row t of the staged SH rows (16 halves = 32 bytes each)
__device__ __forceinline__ void gsr_load_sh_rows(int q, size_t t, const uint16_t* shx, const uint16_t* shy, const uint16_t* shz, uint16_t* row)
{
    const int ch = (q - 1) >> 1, part = (q - 1) & 1;
    const uint16_t* from = (ch == 0 ? shx : (ch == 1 ? shy : shz)) + 16 * t + 8 * part;
    *reinterpret_cast<uint4*>(&row[16 * ch + 8 * part]) = *reinterpret_cast<const uint4*>(from);
}

// ---------------------------------------------------------------------------
// The bounds of ONE cluster (k_cluster.h), folded by a workgroup of GSR_PACK_THREADS: what each lane brings starts neutral;
// gsr_lane_bounds adds the lane's piece -- lane 0 the position (never cull: a non-finite coordinate), lane 7 the extent half
// (never cull: !(mf < 6e4)) -- and a lane without one, or of a slot behind n, brings the neutral values.
struct GsrClusterIn {
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, mf = 0.0f;
    bool bad = false;
};
__device__ __forceinline__ bool gsr_position_bad(float x, float y, float z)
{
    return !(__builtin_fabsf(x) < 3.0e38f) || !(__builtin_fabsf(y) < 3.0e38f) || !(__builtin_fabsf(z) < 3.0e38f);
}
__device__ __forceinline__ void gsr_lane_bounds(int q, uint4 piece, GsrClusterIn& in)
{
    if (q == 0) {
        const float4 a = gsr_as_float4(piece);
        in.bad |= gsr_position_bad(a.x, a.y, a.z);
        in.lo[0] = in.hi[0] = a.x; in.lo[1] = in.hi[1] = a.y; in.lo[2] = in.hi[2] = a.z;
    } else if (q == 7) {
        in.mf = gsr_h2f(gsr_hi16(piece.w));
        in.bad |= !(in.mf < 6.0e4f);
    }
}
__device__ __forceinline__ void gsr_cluster_fold(GsrClusterIn& in, float (&s_red)[8][8], float4* __restrict__ clusA, float4* __restrict__ clusB)
{
    float (&lo)[3] = in.lo, (&hi)[3] = in.hi, mf = in.mf;
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool any_bad = __ballot(in.bad) != 0ull;
#pragma unroll
    for (int d = 8; d < 64; d <<= 1) {     // (the position lanes are q = 0, the extent lanes q = 7: strides of eight)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = __builtin_fminf(lo[k], __shfl_xor(lo[k], d, 64));
            hi[k] = __builtin_fmaxf(hi[k], __shfl_xor(hi[k], d, 64));
        }
        mf = __builtin_fmaxf(mf, __shfl_xor(mf, d, 64));
    }
    const int lane = tid & 63;
    if (lane == 0) { s_red[wave][0] = lo[0]; s_red[wave][1] = lo[1]; s_red[wave][2] = lo[2]; s_red[wave][3] = hi[0]; s_red[wave][4] = hi[1]; s_red[wave][5] = hi[2]; s_red[wave][7] = any_bad ? 1.0f : 0.0f; }
    if (lane == 7) s_red[wave][6] = mf;
    __syncthreads();
    if (tid == 0) {
        const GsrClusterIn none;
        float l0 = none.lo[0], l1 = none.lo[1], l2 = none.lo[2], h0 = none.hi[0], h1 = none.hi[1], h2 = none.hi[2], m = none.mf, b = 0.0f;
        for (int w = 0; w < 8; ++w) {
            l0 = __builtin_fminf(l0, s_red[w][0]); l1 = __builtin_fminf(l1, s_red[w][1]); l2 = __builtin_fminf(l2, s_red[w][2]);
            h0 = __builtin_fmaxf(h0, s_red[w][3]); h1 = __builtin_fmaxf(h1, s_red[w][4]); h2 = __builtin_fmaxf(h2, s_red[w][5]);
            m = __builtin_fmaxf(m, s_red[w][6]); b = __builtin_fmaxf(b, s_red[w][7]);
        }
        clusA[blockIdx.x] = make_float4(l0, l1, l2, m);
        clusB[blockIdx.x] = make_float4(h0, h1, h2, b != 0.0f ? 1.0f : 0.0f);
    }
}

// ---------------------------------------------------------------------------
// A splat's pieces, in and out.
// A NEW splat, from row t of the staged arrays (in front of gsr_wave_lds_sync): lane 0 forms geoA's piece and lane 7 geoB's, lanes
// 0..6 fill the LDS row; behind the sync a lane with gsr_colour_lane<SH>(q) takes its piece from gsr_colour_chunk<SH>(row, q - 1).
struct GsrPackSrc {
    const float* P; const float* alpha;
    const uint16_t *Cd, *scale, *orient, *shx, *shy, *shz;
};
template <bool SH>
__device__ __forceinline__ uint4 gsr_stage_new_splat(int q, size_t t, const GsrPackSrc& src, uint16_t* row)
{
    if (q == 0) {
        const float px = src.P[3 * t], py = src.P[3 * t + 1], pz = src.P[3 * t + 2], op = src.alpha[t];
        gsr_load_cd(src.Cd, t, row);
        return gsr_as_uint4(make_float4(px, py, pz, op));
    }
    if (q == 7) {
        GsrShape h;
        gsr_load_scale(src.scale, t, h);
        gsr_load_orient(src.orient, t, h);
        return gsr_shape_join(h);
    }
    if (SH) gsr_load_sh_rows(q, t, src.shx, src.shy, src.shz, row);
    return make_uint4(0u, 0u, 0u, 0u);
}
// Lanes 0 and 7 store their piece into slot j of geoA / geoB, and bring the cluster what it takes from them.
__device__ __forceinline__ void gsr_store_geo(int q, uint32_t j, uint4 piece, float4* __restrict__ geoA, uint4* __restrict__ geoB, GsrClusterIn& in)
{
    if (q == 0) { geoA[j] = gsr_as_float4(piece); gsr_lane_bounds(0, piece, in); }
    else if (q == 7) { geoB[j] = piece; gsr_lane_bounds(7, piece, in); }
}

// ---------------------------------------------------------------------------
// K0 (round 6): the registerUpdate()-layout arrays of a whole upload (in the staging arena, device memory, upload order) -> the
// resident layout, straight INTO STORAGE ORDER, with the cluster bounds on the way out.
//   storage slot j <- splat perm[j] (the stable order of the positions' Morton codes, k_cluster.h; NULL: upload order)
// A wave WRITES eight whole 128-byte colrow lines, 128 contiguous bytes of geoA, of geoB and of each colour chunk, and READS, per
// splat, its rows of the source arrays (96 + 36 bytes; a gather when perm is a permutation).  Before round 6 this was three passes:
// k_repack (one thread per splat, 2-byte loads at a 32-byte stride, 16-byte stores at a 128-byte stride: 1.5 x write amplification,
// 0.19 of HBM), then k_permute_geo + k_permute_rows over a second copy of the geometry, then k_cluster_bounds.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_pack(uint32_t n, uint32_t cap, GsrPackSrc src, const uint32_t* __restrict__ perm,
       float4* __restrict__ geoA, uint4* __restrict__ geoB, uint4* __restrict__ col, uint4* __restrict__ colrow,
       float4* __restrict__ clusA, float4* __restrict__ clusB)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = one cluster");
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][GSR_ROW_HALVES];
    __shared__ float s_red[8][8];                                           // per wave: lo.xyz hi.xyz mf bad
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t j = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    const bool live = j < n;
    const uint32_t i = live ? (perm ? perm[j] : j) : 0u;
    GsrClusterIn in;
    uint4 rowpiece = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        const uint4 piece = gsr_stage_new_splat<SH>(q, i, src, s_h[sp]);
        gsr_store_geo(q, j, piece, geoA, geoB, in);
        if (q == 0) rowpiece = piece;
    }
    gsr_wave_lds_sync();
    if (live && gsr_colour_lane<SH>(q)) {
        rowpiece = gsr_colour_chunk<SH>(s_h[sp], q - 1);
        col[(size_t)(q - 1) * cap + j] = rowpiece;     // SoA chunks: coalesced for a pass over ALL splats (eager colour)
    }
    // ... and as ONE 128-byte row per splat, gathered by index (lazy colour): piece q from lane q, the eight pieces of a row in ONE store
    // instruction (as three -- position, colours, padding -- a quarter of the rows went out as partial lines: PMC 1.16 x the output)
    if (SH && live) colrow[(size_t)j * 8 + q] = rowpiece;
    gsr_cluster_fold(in, s_red, clusA, clusB);
}

// ---------------------------------------------------------------------------
// K0u: attributes of RESIDENT splats rewritten in place (gsr_update, gsr_update_device): k_pack mirrored.  Rows [0, cnt) of the
// source arrays = splats [first, first + cnt) of the upload are read coalesced and scattered into the storage slots
//   j = inv[first + t]     (NULL: upload order, j = first + t)
// An array that is NULL is left as it is in HBM, and pieces of a splat's colrow line that do not change are not written:
//   q = 0      alpha -> geoA[j].w and colrow[j][0].w (4-byte stores; the position stays); Cd (or, SH without Cd, the resident Cd) -> LDS
//   q = 1..6   SH -> LDS, then chunk q - 1 -> col[q - 1][j] and colrow[j][q]; Cd alone: lane 1 rewrites halves 0..2 of chunk 0
//              (an SH context: read-modify-write, sh1.rgb and sh2.rg survive; no SH: Cd + zero halves, and there is no colrow)
//   q = 7      scale and / or orient (the other from the resident geoB[j]) -> geoB[j] with its extent bound
// !live lanes stay until behind the sync.  The cluster bounds follow in k_cluster_extents.
// Src is where the rows come from: its Cd / scale / orient go through gsr_src_half, and it says how lane q brings its SH.
struct GsrUpdateSrc {            // the staging arena: halves, k_pack's x / y / z rows
    const float* alpha;
    const uint16_t *Cd, *scale, *orient, *shx, *shy, *shz;
    __device__ __forceinline__ bool has_sh() const { return shx != nullptr; }        // (all three or none: the host checks)
    __device__ __forceinline__ void load_sh(int q, size_t t, uint16_t* row) const { gsr_load_sh_rows(q, t, shx, shy, shz, row); }
};
// float32 rows in DEVICE memory, read once and quantised in registers: no staging copy of the halves, nothing crosses the link.
// Every source value is ONE 4-byte load inside its array (rows are not 16-byte aligned: 15 vec3 are 180 bytes).  Per splat
// 4 + 12 + 12 + 16 + 12 vpp bytes are read of what is given (224 with everything at vpp = 15) against 122 of halves.
struct GsrUpdateSrcF32 {
    const float *alpha, *Cd, *scale, *orient, *sh;
    int32_t vpp;                 // vec3 per point of sh: 1..16
    __device__ __forceinline__ bool has_sh() const { return sh != nullptr; }
    // lane q: floats [8 (q - 1), 8 (q - 1) + 8) of the splat's 3 * vpp; a slot without data is a zero HALF, as k_quantize_raw leaves it
    __device__ __forceinline__ void load_sh(int q, size_t t, uint16_t* row) const
    {
        const int nf = 3 * vpp;                        // floats of a splat's row (<= 48)
        const float* from = sh + t * (size_t)nf;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int f = 8 * (q - 1) + k;
            row[gsr_sh_float_slot(f)] = f < nf ? gsr_f2h(from[f]) : (uint16_t)0;
        }
    }
};
template <bool SH, typename Src>
__device__ __forceinline__ void gsr_update_body(uint32_t first, uint32_t cnt, uint32_t cap, const Src src, const uint32_t* __restrict__ inv,
                                                float4* __restrict__ geoA, uint4* __restrict__ geoB, uint4* __restrict__ col, uint4* __restrict__ colrow,
                                                uint16_t* row /* this splat's LDS row */)
{
    const int q = threadIdx.x & 7;
    const uint32_t t = blockIdx.x * (uint32_t)GSR_CLUSTER + (threadIdx.x >> 3);
    const bool live = t < cnt;
    const uint32_t j = live ? (inv ? inv[first + t] : first + t) : 0u;
    const bool sh = SH && src.has_sh();
    if (live) {
        if (q == 0) {
            if (src.alpha) {
                const float op = src.alpha[t];
                reinterpret_cast<float*>(geoA + j)[3] = op;
                if (SH) reinterpret_cast<float*>(colrow + (size_t)j * 8)[3] = op;
            }
            if (src.Cd) {
                gsr_load_cd(src.Cd, t, row);
            } else if (sh) {                           // new SH under the resident Cd: halves 0..2 of chunk 0
                const uint2 w = *reinterpret_cast<const uint2*>(col + j);
                row[48] = gsr_lo16(w.x); row[49] = gsr_hi16(w.x); row[50] = gsr_lo16(w.y);
            }
        } else if (q == 7) {
            if (src.scale || src.orient) {
                GsrShape h{};
                if (!src.scale || !src.orient) h = gsr_shape_split(geoB[j]);
                if (src.orient) gsr_load_orient(src.orient, t, h);
                if (src.scale) gsr_load_scale(src.scale, t, h);
                geoB[j] = gsr_shape_join(h);
            }
        } else if (sh) {
            src.load_sh(q, t, row);
        }
    }
    gsr_wave_lds_sync();
    if (!live) return;
    if (sh) {
        if (q >= 1 && q <= 6) {
            const uint4 v = gsr_colour_chunk<true>(row, q - 1);
            col[(size_t)(q - 1) * cap + j] = v;
            colrow[(size_t)j * 8 + q] = v;
        }
    } else if (q == 1 && src.Cd) {
        const uint32_t w0 = gsr_pk(row[48], row[49]), c2 = row[50];
        if (SH) {
            uint4 v = col[j];
            v.x = w0; v.y = (v.y & 0xffff0000u) | c2;
            col[j] = v;
            colrow[(size_t)j * 8 + 1] = v;
        } else {
            col[j] = make_uint4(w0, c2, 0u, 0u);
        }
    }
}
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_update(uint32_t first, uint32_t cnt, uint32_t cap, GsrUpdateSrc src, const uint32_t* __restrict__ inv,
         float4* __restrict__ geoA, uint4* __restrict__ geoB, uint4* __restrict__ col, uint4* __restrict__ colrow)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][GSR_ROW_HALVES];
    gsr_update_body<SH>(first, cnt, cap, src, inv, geoA, geoB, col, colrow, s_h[threadIdx.x >> 3]);
}

// ... and the w fields of the cluster bounds after scale / orient changed: clusA[c].w = the largest extent bound of the cluster's live
// slots, clusB[c].w = the "never cull" flag -- from the resident geoA / geoB, by gsr_lane_bounds, so a bound is neither stale-large
// after a shrink nor stale-small after a growth.  lo.xyz / hi.xyz depend on the positions alone and are not touched.  One WAVE per
// cluster, one lane per splat (32 bytes read), so a lane brings both pieces of its splat.
__global__ void __launch_bounds__(256)
k_cluster_extents(uint32_t n, uint32_t nclus, const float4* __restrict__ geoA, const uint4* __restrict__ geoB,
                  float4* __restrict__ clusA, float4* __restrict__ clusB)
{
    static_assert(GSR_CLUSTER == 64, "one wave = one cluster");
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (c >= nclus) return;                            // (wave-uniform)
    const uint32_t j = c * (uint32_t)GSR_CLUSTER + (uint32_t)lane;
    GsrClusterIn in;
    if (j < n) {
        gsr_lane_bounds(0, gsr_as_uint4(geoA[j]), in);
        gsr_lane_bounds(7, geoB[j], in);
    }
    float mf = in.mf;
    const bool any_bad = __ballot(in.bad) != 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) mf = __builtin_fmaxf(mf, __shfl_xor(mf, d, 64));
    // (gsr_cluster_fold folds the same values with fmaxf, which drops a NaN operand, so the order of the fold does not matter; its last
    //  fold starts from 0, which turns a cluster whose bounds are ALL NaN into 0: so does this one)
    mf = __builtin_fmaxf(0.0f, mf);
    if (lane == 0) {
        reinterpret_cast<float*>(clusA + c)[3] = mf;
        reinterpret_cast<float*>(clusB + c)[3] = any_bad ? 1.0f : 0.0f;
    }
}

// ---------------------------------------------------------------------------
// K0m: new POSITIONS for resident splats (gsr_move).  A position decides the storage order, so a move is: the new rows written where
// the splats sit now (k_move_positions), the ordering of an upload over ALL positions in upload order (k_bbox_partials,
// k_morton_codes, the radix sort), and the resident planes carried from the old order into the new one (k_repack) -- nothing but
// the new P rows crosses the link.
// k_move_positions: one thread per resident splat i (upload order), old slot j = inv[i] (inv: the inverse of the storage permutation
// in force; NULL: j = i).  Splats [first, first + cnt) take row i - first of Pnew into geoA[j].xyz and, with SH, into piece 0 of
// their colour row (three 4-byte stores each; .w, the opacity, stays); the others keep what geoA holds, which is the raw P bits of
// their upload.  Either way the position goes to Pup[3 i ..]: the whole cloud's positions in upload order, what the ordering reads.
__global__ void __launch_bounds__(256)
k_move_positions(uint32_t first, uint32_t cnt, uint32_t n, const float* __restrict__ Pnew, const uint32_t* __restrict__ inv,
                 float4* __restrict__ geoA, uint4* __restrict__ colrow /* NULL: no SH */, float* __restrict__ Pup)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = inv ? inv[i] : i;
    float px, py, pz;
    if (i - first < cnt) {                             // (unsigned: also false for i < first)
        const float* p = Pnew + 3 * (size_t)(i - first);
        px = p[0]; py = p[1]; pz = p[2];
        float* a = reinterpret_cast<float*>(geoA + j);
        a[0] = px; a[1] = py; a[2] = pz;
        if (colrow) {
            float* r = reinterpret_cast<float*>(colrow + (size_t)j * 8);
            r[0] = px; r[1] = py; r[2] = pz;
        }
    } else {
        const float4 a = geoA[j];
        px = a.x; py = a.y; pz = a.z;
    }
    float* o = Pup + 3 * (size_t)i;
    o[0] = px; o[1] = py; o[2] = pz;
}

// k_repack: the resident planes from the old storage order into the new one, into the SPARE copy of the planes (the host swaps the
// two sets afterwards).  One workgroup = one destination cluster:
//   slot j' <- the splat i = perm_new[j'] (NULL: i = j'), which sits in slot j = inv_old[i] (NULL: j = i)
// Every lane carries its pieces as they are, each load and its store in the SAME lane branch: with the loads in one set of branches and
// the stores in another the compiler waits in front of each store for the store before it, 0.1 ms of 0.9 at 6 M splats (LAB_NOTES.md,
// "Resident-layout kernels in one header").  Slots behind n in the last cluster are not written, as k_pack leaves them.  The colour
// chunks are strided by the SOURCE capacity where they are read and by the DESTINATION capacity where they are written, as k_add_pack's
// are: the two differ only for a gsr_duplicate that grows the context.
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_repack(uint32_t n, uint32_t cap_src, uint32_t cap_dst, const uint32_t* __restrict__ perm_new, const uint32_t* __restrict__ inv_old,
         const float4* __restrict__ geoA, const uint4* __restrict__ geoB, const uint4* __restrict__ col, const uint4* __restrict__ colrow,
         float4* __restrict__ geoA2, uint4* __restrict__ geoB2, uint4* __restrict__ col2, uint4* __restrict__ colrow2,
         float4* __restrict__ clusA2, float4* __restrict__ clusB2)
{
    static_assert(GSR_PACK_THREADS == 8 * GSR_CLUSTER, "one workgroup = one cluster");
    __shared__ float s_red[8][8];
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t jn = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    GsrClusterIn in;
    if (jn < n) {
        const uint32_t i = perm_new ? perm_new[jn] : jn;
        const uint32_t j = inv_old ? inv_old[i] : i;
        if (SH) colrow2[(size_t)jn * 8 + q] = colrow[(size_t)j * 8 + q];
        if (q == 0) gsr_store_geo(0, jn, gsr_as_uint4(geoA[j]), geoA2, geoB2, in);
        else if (q == 7) gsr_store_geo(7, jn, geoB[j], geoA2, geoB2, in);
        else if (gsr_colour_lane<SH>(q)) col2[(size_t)(q - 1) * cap_dst + jn] = col[(size_t)(q - 1) * cap_src + j];
    }
    gsr_cluster_fold(in, s_red, clusA2, clusB2);
}

// ... and where no permutation is in force before or after the move (upload order kept): the splats stay where they are and only the
// cluster bounds are formed again, in place, from the resident geoA / geoB -- k_repack without the copies.
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_cluster_bounds(uint32_t n, const float4* __restrict__ geoA, const uint4* __restrict__ geoB, float4* __restrict__ clusA, float4* __restrict__ clusB)
{
    __shared__ float s_red[8][8];
    const int tid = threadIdx.x, q = tid & 7, sp = tid >> 3;
    const uint32_t j = blockIdx.x * (uint32_t)GSR_CLUSTER + (uint32_t)sp;
    GsrClusterIn in;
    if (j < n) {
        if (q == 0) gsr_lane_bounds(0, gsr_as_uint4(geoA[j]), in);
        else if (q == 7) gsr_lane_bounds(7, geoB[j], in);
    }
    gsr_cluster_fold(in, s_red, clusA, clusB);
}

// ---------------------------------------------------------------------------
// K0': raw float32 point attributes (as a Houdini detail holds them) -> the half arrays k_pack takes.  What
// GR_PrimGsplat::update does on the CPU in a tbb::parallel_for (/root/reference/gsplat_plugin/src/GR_GSplat.C:302-372):
// fp32 -> fp16 (HDK's fpreal16: round to nearest even, overflow to infinity -- what v_cvt_f16_f32 does), the defaults for
// missing attributes, and the three spherical-harmonics naming schemes -> coefficient j in flat slot j of the x / y / z rows.
struct GsrRawSh {
    int32_t scheme;              // 0 none, 1 = one array of `vec3_per_point` vec3 per point, 2 = sh1..sh15 (vec3 arrays), 3 = f_rest_0..44 (float arrays)
    int32_t vec3_per_point;      // scheme 1
    const float* array;          // scheme 1
    const float* ptr[45];        // scheme 2: [0..14] (NULL from the first gap on), scheme 3: [0..44] (likewise)
};
__global__ void __launch_bounds__(256)
k_quantize_raw(uint32_t n, const float* __restrict__ Cd, const float* __restrict__ scale, const float* __restrict__ orient, GsrRawSh sh,
               uint16_t* __restrict__ oCd, uint16_t* __restrict__ oS, uint16_t* __restrict__ oO,
               uint16_t* __restrict__ ox, uint16_t* __restrict__ oy, uint16_t* __restrict__ oz)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        oCd[3 * (size_t)i + k] = Cd ? gsr_f2h(Cd[3 * (size_t)i + k]) : (uint16_t)0;            // missing Cd: black
        oS[3 * (size_t)i + k] = scale ? gsr_f2h(scale[3 * (size_t)i + k]) : (uint16_t)0x3c00;  // missing scale: 1
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) oO[4 * (size_t)i + k] = orient ? gsr_f2h(orient[4 * (size_t)i + k]) : (uint16_t)(k == 3 ? 0x3c00 : 0);   // (0, 0, 0, 1)
    if (sh.scheme == 0) return;
    for (int j = 0; j < 16; ++j) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        bool have = false;
        if (sh.scheme == 1) {
            have = j < sh.vec3_per_point;
            if (have) { const float* v = sh.array + ((size_t)i * sh.vec3_per_point + j) * 3; x = v[0]; y = v[1]; z = v[2]; }
        } else if (sh.scheme == 2) {
            have = j < 15 && sh.ptr[j];
            if (have) { const float* v = sh.ptr[j] + 3 * (size_t)i; x = v[0]; y = v[1]; z = v[2]; }
        } else if (j < 15) {   // channel-major INRIA layout: (f_rest_j, f_rest_{j+15}, f_rest_{j+30}); a missing array leaves zeros
            have = true;
            x = sh.ptr[j] ? sh.ptr[j][i] : 0.0f; y = sh.ptr[j + 15] ? sh.ptr[j + 15][i] : 0.0f; z = sh.ptr[j + 30] ? sh.ptr[j + 30][i] : 0.0f;
        }
        // (a slot without data is a zero HALF, not the conversion of 0.0f: the same bits, said explicitly)
        ox[16 * (size_t)i + j] = have ? gsr_f2h(x) : (uint16_t)0;
        oy[16 * (size_t)i + j] = have ? gsr_f2h(y) : (uint16_t)0;
        oz[16 * (size_t)i + j] = have ? gsr_f2h(z) : (uint16_t)0;
    }
}

// K0u': k_update for float32 sources in DEVICE memory (gsr_update_device; GsrUpdateSrcF32 above)
template <bool SH>
__global__ void __launch_bounds__(GSR_PACK_THREADS)
k_update_f32(uint32_t first, uint32_t cnt, uint32_t cap, GsrUpdateSrcF32 src, const uint32_t* __restrict__ inv,
             float4* __restrict__ geoA, uint4* __restrict__ geoB, uint4* __restrict__ col, uint4* __restrict__ colrow)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_h[GSR_CLUSTER][GSR_ROW_HALVES];
    gsr_update_body<SH>(first, cnt, cap, src, inv, geoA, geoB, col, colrow, s_h[threadIdx.x >> 3]);
}
