// k_connect.h -- resident splats selected by the connected clump of occupied cells they lie in (gsr_select_connected):
// "every clump of fewer than k splats" (floaters come in clumps), "grow my selection to the whole object".
//
// THE rule, in one place.  The grid, the population and what is outside are k_density.h's (gsr_density_axis, gsr_density_class,
// gsr_density_row); what this file adds is gsr_connect_row (which rows of cells a cell looks at: the FORWARD half of its neighbourhood,
// the backward half looks at it), gsr_connect_hook (which of two roots goes under the other), gsr_connect_bin and gsr_connect_hit (the
// verdict over a component's size and seed).  All are __host__ __device__; the kernels and gsr_select_connected_eval go through them.
// Everything behind the cell is integer arithmetic and integer atomics: no stored value depends on the order the waves run in.
//
// THE CELL TABLE (what LAB_NOTES.md, "Density selection", asked for): the occupied cells in key order, ckey[c] rising, cstart[c] the
// position of the cell's first entry in the sorted (key, upload index) pairs, cstart[n_cells] = n_pop, so that the population of the
// cells [a, b) is cstart[b] - cstart[a]; cidx[j] is the cell of sorted entry j.  The graph pass runs over the table: a search is a chain
// over n_cells entries, and there is one thread per cell, not per splat.  No frame kernel changes, and a context that never selects by
// connectivity launches nothing of this file.
#pragma once
#include "k_density.h"
#include "k_remove.h"

#define GSR_CON_BINS     32            // comp_hist / splat_hist: bin b holds the components with floor(log2(size)) == b
#define GSR_CON_NOLABEL  0xFFFFFFFFu   // the label of a splat that is not population
#define GSR_CON_SEEDED   0x80000000u   // the bit of a component's size word (and of a splat's label word) that says "holds a seed"
                                       // (a size is at most n < 2^31 and a label is an upload index < n: neither reaches the bit)

// the rule as the kernels take it: the density rule's grid, population and flags (den.count_lo / count_hi are not looked at), the size
// range, and whether there is a seed clause
struct GsrConnectRule {
    GsrDensityRule den;
    uint32_t size_lo, size_hi;
    int32_t has_seed;
};

// the words of the result block (uint32 each): [0] and [1] are k_density_keys' 64-bit atomic, the rest this file's
#define GSR_CON_R_POP      GSR_DEN_R_POP
#define GSR_CON_R_OUTSIDE  GSR_DEN_R_OUTSIDE
#define GSR_CON_R_CELLS    GSR_DEN_R_CELLS
#define GSR_CON_R_COMPS    4
#define GSR_CON_R_SEEDED   5
#define GSR_CON_R_LARGEST  6
#define GSR_CON_R_CHIST    8
#define GSR_CON_R_SHIST    (GSR_CON_R_CHIST + GSR_CON_BINS)
#define GSR_CON_R_WORDS    (GSR_CON_R_SHIST + GSR_CON_BINS)

// The keys *lo .. *hi (inclusive) of the cells in row (iy + dy, iz + dz) that the cell of `key` links itself to.  Adjacency is
// symmetric, so a cell looks FORWARD only: at the +x side of its own row and at every row lexicographically behind it (dz > 0, or
// dz == 0 and dy > 0) -- 13 cells at reach 1, 62 at reach 2; the cells in front of it look at it.  false: no such cell exists (a row
// outside 0..1023 in y or z; the backward half; its own row at reach 0 or at ix = 1023).  The x clamp is gsr_density_row's: key 1023
// of one row and key 0 of the next are consecutive numbers and never adjacent.
__host__ __device__ __forceinline__ bool gsr_connect_row(uint32_t key, int reach, int dy, int dz, uint32_t* lo, uint32_t* hi)
{
    if (dz < 0 || (dz == 0 && dy < 0)) return false;
    if (!gsr_density_row(key, reach, dy, dz, lo, hi)) return false;
    if (dy == 0 && dz == 0) {
        if (*hi == key) return false;
        *lo = key + 1u;
    }
    return true;
}

// Which of two distinct roots goes under the other: the LARGER table index under the SMALLER.  parent[x] <= x therefore holds on
// every path, a cycle cannot form, and the root of a finished component is its smallest table index whatever the order of the unions.
__host__ __device__ __forceinline__ void gsr_connect_hook(uint32_t a, uint32_t b, uint32_t* under, uint32_t* over)
{
    *under = a > b ? a : b;
    *over = a > b ? b : a;
}

// the bin of comp_hist / splat_hist a component of `size` >= 1 falls into: floor(log2(size))
__host__ __device__ __forceinline__ uint32_t gsr_connect_bin(uint32_t size) { return 31u - (uint32_t)__builtin_clz(size); }

// The verdict over a splat's size word (k_density_keys' count word: GSR_DEN_CNT_OUTSIDE for an outside splat, 0 for one that is not
// population, else the population of its component) and whether its component holds a seed: an outside splat by the flag alone; a
// population splat iff the size lies in the range, compared as unsigned integers, and -- where there is a seed clause -- the
// component is seeded; everything else never.
__host__ __device__ __forceinline__ bool gsr_connect_hit(const GsrConnectRule& r, uint32_t word, bool seeded)
{
    if (word & GSR_DEN_CNT_OUTSIDE) return (r.den.flags & GSR_DENF_HIT_OUTSIDE) != 0;
    if (word == 0u || !(r.size_lo <= word && word <= r.size_hi)) return false;
    return !r.has_seed || seeded;
}

#define GSR_CONNECT_THREADS GSR_DENSITY_THREADS
#define GSR_CONNECT_ROUNDS  8
#define GSR_CONNECT_BLOCK   (GSR_CONNECT_THREADS * GSR_CONNECT_ROUNDS)      // sorted entries one workgroup of the table kernels spans
#define GSR_CONNECT_SLOTS   (GSR_CONNECT_BLOCK / 64)
static_assert(GSR_CONNECT_THREADS == 256 && GSR_CONNECT_SLOTS == 32, "the table kernel scans a block's 32 wave-slots in half a wave");

// the population the key kernel counted, as every kernel below reads it (never more than n: the arrays hold n entries)
__device__ __forceinline__ uint32_t gsr_connect_word(const uint32_t* __restrict__ res, int word, uint32_t n)
{
    const uint32_t v = res[word];
    return v < n ? v : n;
}

// 1a. MARK.  The run starts of the sorted keys (key[j] != key[j - 1], j < n_pop; the sentinels sort behind n_pop and start nothing):
// a workgroup spans GSR_CONNECT_BLOCK entries in 8 rounds of four waves, k_remove_mark's shape; a wave's 64 verdicts are one ballot,
// and the workgroup leaves how many runs start in its block.  k_remove_scan, as it is, turns the block counts into block offsets and
// the total, n_cells.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_mark(uint32_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ res, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_cnt[GSR_CONNECT_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_pop = gsr_connect_word(res, GSR_CON_R_POP, n);
    uint32_t starts = 0u;                              // (wave-uniform)
#pragma unroll
    for (uint32_t r = 0; r < GSR_CONNECT_ROUNDS; ++r) {
        const uint32_t j = blockIdx.x * (uint32_t)GSR_CONNECT_BLOCK + (r * (GSR_CONNECT_THREADS / 64u) + wave) * 64u + lane;
        const bool first = j < n_pop && (j == 0u || keys[j - 1u] != keys[j]);
        starts += (uint32_t)__popcll(__ballot(first));
    }
    if (lane == 0u) s_cnt[wave] = starts;
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// 1b. TABLE.  The same ballots again (eight 64-bit words a wave keeps in registers); their popcounts meet in a 32-word LDS table the
// first wave scans; the run that starts at entry j is cell
//     c = offsets[block] + table[wave-slot] + mbcnt(word)        (the run starts of its wave's word below its own lane)
// and writes ckey[c], cstart[c], parent[c] = c and the zeros the tally adds into.  EVERY entry j < n_pop writes cidx[j], the cell it
// lies in (the run starts at and below it, less one: an entry whose run began in an earlier block gets the last cell of those blocks).
// Thread 0 of workgroup 0 leaves n_cells in the result block and the sentinel cstart[n_cells] = n_pop.  Plain vector stores only.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_table(uint32_t n, const uint32_t* __restrict__ keys, uint32_t* __restrict__ res, const uint32_t* __restrict__ offsets,
                uint32_t* __restrict__ ckey, uint32_t* __restrict__ cstart, uint32_t* __restrict__ parent, uint32_t* __restrict__ csize,
                uint32_t* __restrict__ clabel, uint32_t* __restrict__ cseed, uint32_t* __restrict__ cidx)
{
    __shared__ uint32_t s_pre[GSR_CONNECT_SLOTS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_pop = gsr_connect_word(res, GSR_CON_R_POP, n);
    unsigned long long words[GSR_CONNECT_ROUNDS];
    uint32_t mykey[GSR_CONNECT_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < GSR_CONNECT_ROUNDS; ++r) {
        const uint32_t s = r * (GSR_CONNECT_THREADS / 64u) + wave;
        const uint32_t j = blockIdx.x * (uint32_t)GSR_CONNECT_BLOCK + s * 64u + lane;
        mykey[r] = j < n_pop ? keys[j] : 0u;
        const bool first = j < n_pop && (j == 0u || keys[j - 1u] != mykey[r]);
        words[r] = __ballot(first);
        if (lane == 0u) s_pre[s] = (uint32_t)__popcll(words[r]);
    }
    __syncthreads();
    if (wave == 0u) {
        const uint32_t v = lane < (uint32_t)GSR_CONNECT_SLOTS ? s_pre[lane] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < GSR_CONNECT_SLOTS; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane < (uint32_t)GSR_CONNECT_SLOTS) s_pre[lane] = incl - v;
    }
    __syncthreads();
    const uint32_t base = offsets[blockIdx.x];
#pragma unroll
    for (uint32_t r = 0; r < GSR_CONNECT_ROUNDS; ++r) {
        const uint32_t s = r * (GSR_CONNECT_THREADS / 64u) + wave;
        const uint32_t j = blockIdx.x * (uint32_t)GSR_CONNECT_BLOCK + s * 64u + lane;
        if (j >= n_pop) continue;
        const unsigned long long word = words[r];
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(word >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)word, 0u));
        const uint32_t first = (uint32_t)((word >> lane) & 1ull);
        const uint32_t c = base + s_pre[s] + below + first - 1u;           // (entry 0 starts a run: never 0 - 1)
        cidx[j] = c;
        if (first) {
            ckey[c] = mykey[r];
            cstart[c] = j;
            parent[c] = c;
            csize[c] = 0u;
            clabel[c] = GSR_CON_NOLABEL;
            cseed[c] = 0u;
        }
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        const uint32_t total = offsets[gridDim.x], n_cells = total < n_pop ? total : n_pop;
        res[GSR_CON_R_CELLS] = n_cells;
        cstart[n_cells] = n_pop;
    }
}

// 1c. SEEDS (launched only where there is a seed clause).  One thread per sorted entry j < n_pop: the seed bit of its upload index
// (always below n: a bit at or behind n is never looked at; a splat that is not population is no entry) marks its cell.  Every word of
// the seed is consumed here, launches before the one that writes the mask: the seed may BE the mask.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_seed(uint32_t n, uint32_t nchunks, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ res, const uint32_t* __restrict__ seed,
               const uint32_t* __restrict__ cidx, uint32_t* __restrict__ cseed)
{
    const uint32_t n_pop = gsr_connect_word(res, GSR_CON_R_POP, n);
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_CONNECT_THREADS >= n_pop) break;
        const uint32_t j = chunk * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
        if (j >= n_pop) continue;
        const uint32_t i = vals[j];
        if (i < n && ((seed[i >> 5] >> (i & 31u)) & 1u)) atomicOr(cseed + cidx[j], 1u);
    }
}

// The lock-free union-find of the link kernel.  parent[] only ever falls (a root x is hooked by ONE compare-and-swap x -> smaller;
// a word that is not a root is only lowered further, to an ancestor, by the path halving), so parent[x] <= x always, a walk ends, and a
// stale value is still an ancestor.  The loads are relaxed agent-scope atomics: they are served by the L2, not by a CU's L1, so the
// retry loop sees what a failed compare-and-swap has just been told.  No thread waits for another: a compare-and-swap fails only
// because somebody else's succeeded, and each success lowers a word that can be lowered finitely often.
__device__ __forceinline__ uint32_t gsr_connect_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t gsr_connect_find(uint32_t* __restrict__ parent, uint32_t x)
{
    uint32_t p = gsr_connect_load(parent + x);
    while (p != x) {
        const uint32_t gp = gsr_connect_load(parent + p);
        if (gp != p) (void)__hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // halve the path
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void gsr_connect_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = gsr_connect_find(parent, a);
        b = gsr_connect_find(parent, b);
        if (a == b) return;
        uint32_t under, over;
        gsr_connect_hook(a, b, &under, &over);
        const uint32_t was = atomicCAS(parent + under, under, over);
        if (was == under) return;
        a = was;                                       // somebody hooked `under` first, below it: go on from where it hangs now
        b = over;
    }
}

// 2. LINK.  One thread per occupied cell c < n_cells.  Its own row's +x side, and per z plane dz = 0 .. reach the up to five rows of
// gsr_connect_row: each row's first key is found in ckey[0, n_cells) by k_density_count's branchless lower bound, the searches of a
// plane in lock step (every step issues all its loads before it looks at one; a row that does not exist searches for key 0 and stays at
// 0; every index is clamped into the table, so no load depends on a comparison).  From there the row's at most 2 reach + 1 occupied
// cells are consecutive table entries: each is united with c.  No scratch: every array is indexed by unrolled constants.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_link(uint32_t n, uint32_t nchunks, int reach, const uint32_t* __restrict__ res, const uint32_t* __restrict__ ckey, uint32_t* __restrict__ parent)
{
    const uint32_t n_cells = gsr_connect_word(res, GSR_CON_R_CELLS, n);
    const uint32_t top = n_cells ? 1u << (31 - __clz((int)n_cells)) : 0u;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_CONNECT_THREADS >= n_cells) break;
        const uint32_t c = chunk * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
        if (c >= n_cells) continue;
        const uint32_t key = ckey[c];
        for (int dz = 0; dz <= reach; ++dz) {
            uint32_t klo[GSR_DEN_ROWS], khi[GSR_DEN_ROWS], pos[GSR_DEN_ROWS];
            uint32_t on = 0u;
#pragma unroll
            for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                const int dy = r - 2;
                uint32_t a = 0u, b = 0u;
                const bool ok = dy >= -reach && dy <= reach && gsr_connect_row(key, reach, dy, dz, &a, &b);
                klo[r] = ok ? a : 0u;
                khi[r] = ok ? b : 0u;
                pos[r] = 0u;
                on |= ok ? 1u << r : 0u;
            }
            for (uint32_t s = top; s; s >>= 1) {
                uint32_t va[GSR_DEN_ROWS];
#pragma unroll
                for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                    va[r] = 0u;
                    if (r - 2 >= -reach && r - 2 <= reach && (dz > 0 || r >= 2)) {     // (uniform)
                        const uint32_t ta = pos[r] + s;
                        va[r] = ckey[(ta < n_cells ? ta : n_cells) - 1u];
                    }
                }
#pragma unroll
                for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                    const uint32_t ta = pos[r] + s;
                    if (ta <= n_cells && va[r] < klo[r]) pos[r] = ta;
                }
            }
#pragma unroll
            for (int r = 0; r < GSR_DEN_ROWS; ++r) {
                if (!((on >> r) & 1u)) continue;
                for (uint32_t p = pos[r]; p < n_cells; ++p) {
                    if (ckey[p] > khi[r]) break;
                    gsr_connect_unite(parent, c, p);
                }
            }
        }
    }
}

// 3. FLATTEN AND TALLY, a launch of its own: parent[] is final, plain loads see it.  One thread per cell: croot[c] = the root of c,
// and the cell's run length, its smallest upload index (the sort is stable: the first entry of its run) and its seed mark go to the
// root -- an integer add, an integer min and an OR of GSR_CON_SEEDED into the size word.  A cloud is mostly ONE big component, and
// n_cells atomics on one address queue (k_visibility.h records what that costs), so the lanes of a wave that hold the same root meet
// first: the wave takes the root of its first waiting lane, sums, minimises and ORs over the lanes that share it by butterflies, and
// that lane alone sends.  Integer atomics only: what is stored does not depend on the order.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_flatten(uint32_t n, uint32_t nchunks, const uint32_t* __restrict__ res, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ cstart,
                  const uint32_t* __restrict__ parent, const uint32_t* __restrict__ cseed, uint32_t* __restrict__ croot, uint32_t* __restrict__ csize,
                  uint32_t* __restrict__ clabel)
{
    const uint32_t n_cells = gsr_connect_word(res, GSR_CON_R_CELLS, n);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_CONNECT_THREADS >= n_cells) break;
        const uint32_t c = chunk * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
        bool todo = c < n_cells;
        uint32_t root = 0u, len = 0u, lab = GSR_CON_NOLABEL, sd = 0u;
        if (todo) {
            root = c;
            for (uint32_t p = parent[root]; p != root; p = parent[root]) root = p;
            croot[c] = root;
            const uint32_t at = cstart[c];
            len = cstart[c + 1u] - at;
            lab = vals[at];
            sd = cseed[c] ? GSR_CON_SEEDED : 0u;
        }
        for (;;) {
            const unsigned long long waiting = __ballot(todo);
            if (!waiting) break;                       // (wave-uniform)
            const int first = __ffsll((long long)waiting) - 1;
            const uint32_t r = (uint32_t)__shfl((int)root, first, 64);
            const bool mine = todo && root == r;
            uint32_t s = mine ? len : 0u, l = mine ? lab : GSR_CON_NOLABEL, f = mine ? sd : 0u;
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                s += (uint32_t)__shfl_xor((int)s, d, 64);
                const uint32_t lo = (uint32_t)__shfl_xor((int)l, d, 64);
                l = lo < l ? lo : l;
                f |= (uint32_t)__shfl_xor((int)f, d, 64);
            }
            if (lane == (uint32_t)first) {
                atomicAdd(csize + r, s);
                atomicMin(clabel + r, l);
                if (f) atomicOr(csize + r, f);
            }
            todo = todo && !mine;
        }
    }
}

// 4. STATS, behind the tally.  One thread per cell; a root (croot[c] == c) is a component: how many there are and how many hold a
// seed are ballots summed over a wave's chunks, the largest size and the two histograms are privatised in LDS; each leaves the
// workgroup once, under the capped grid of the density kernels (GSR_DENSITY_BLOCKS).
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_stats(uint32_t n, uint32_t nchunks, const uint32_t* __restrict__ croot, const uint32_t* __restrict__ csize, uint32_t* __restrict__ res)
{
    __shared__ uint32_t s_hist[2 * GSR_CON_BINS];
    __shared__ uint32_t s_word[3];
    if (threadIdx.x < 2u * GSR_CON_BINS) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x >= 64u && threadIdx.x < 67u) s_word[threadIdx.x - 64u] = 0u;
    __syncthreads();
    const uint32_t n_cells = gsr_connect_word(res, GSR_CON_R_CELLS, n);
    uint32_t comps = 0u, seeded = 0u;                  // (wave-uniform)
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_CONNECT_THREADS >= n_cells) break;
        const uint32_t c = chunk * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
        bool is_root = false, has_seed = false;
        if (c < n_cells && croot[c] == c) {
            const uint32_t word = csize[c], size = word & ~GSR_CON_SEEDED;
            is_root = true;
            has_seed = (word & GSR_CON_SEEDED) != 0u;
            if (size) {
                const uint32_t b = gsr_connect_bin(size);
                atomicAdd(&s_hist[b], 1u);
                atomicAdd(&s_hist[GSR_CON_BINS + b], size);
                atomicMax(&s_word[2], size);
            }
        }
        comps += (uint32_t)__popcll(__ballot(is_root));
        seeded += (uint32_t)__popcll(__ballot(has_seed));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (comps) atomicAdd(&s_word[0], comps);
        if (seeded) atomicAdd(&s_word[1], seeded);
    }
    __syncthreads();
    if (threadIdx.x < 2u * GSR_CON_BINS && s_hist[threadIdx.x]) atomicAdd(res + GSR_CON_R_CHIST + threadIdx.x, s_hist[threadIdx.x]);
    if (threadIdx.x == 64u && s_word[0]) atomicAdd(res + GSR_CON_R_COMPS, s_word[0]);
    if (threadIdx.x == 65u && s_word[1]) atomicAdd(res + GSR_CON_R_SEEDED, s_word[1]);
    if (threadIdx.x == 66u && s_word[2]) atomicMax(res + GSR_CON_R_LARGEST, s_word[2]);
}

// 5a. SCATTER.  One thread per sorted entry j < n_pop: the size and the label of its cell's root go to its upload index through
// vals -- usize[i] (k_density_keys' count word: it wrote 0, or the outside bit, into every word) and ulabel[i], the label with
// GSR_CON_SEEDED in its top bit.  One scattered dword each.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_scatter(uint32_t n, uint32_t nchunks, const uint32_t* __restrict__ res, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ cidx,
                  const uint32_t* __restrict__ croot, const uint32_t* __restrict__ csize, const uint32_t* __restrict__ clabel,
                  uint32_t* __restrict__ usize, uint32_t* __restrict__ ulabel)
{
    const uint32_t n_pop = gsr_connect_word(res, GSR_CON_R_POP, n);
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (chunk * (uint32_t)GSR_CONNECT_THREADS >= n_pop) break;
        const uint32_t j = chunk * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
        if (j >= n_pop) continue;
        const uint32_t i = vals[j], root = croot[cidx[j]];
        const uint32_t word = csize[root];
        if (i < n) {
            usize[i] = word & ~GSR_CON_SEEDED;
            ulabel[i] = clabel[root] | (word & GSR_CON_SEEDED);
        }
    }
}

// 5b. HIT.  One thread per UPLOAD index i: the size word of i, the verdict, the label and the size into labels_out / sizes_out
// (NULL: skipped; GSR_CON_NOLABEL and 0 for what is not population), and k_select's epilogue unchanged.
__global__ void __launch_bounds__(GSR_CONNECT_THREADS)
k_connect_hit(uint32_t n, GsrConnectRule rule, const uint32_t* __restrict__ usize, const uint32_t* __restrict__ ulabel,
              uint32_t* __restrict__ labels_out /* NULL: none */, uint32_t* __restrict__ sizes_out /* NULL: none */, uint32_t* __restrict__ mask,
              unsigned long long* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * (uint32_t)GSR_CONNECT_THREADS + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t word = usize[i];
        const bool pop = word != 0u && !(word & GSR_DEN_CNT_OUTSIDE);
        const uint32_t lw = pop ? ulabel[i] : GSR_CON_NOLABEL;
        hit = gsr_connect_hit(rule, word, pop && (lw & GSR_CON_SEEDED) != 0u);
        if (labels_out) labels_out[i] = pop ? lw & ~GSR_CON_SEEDED : GSR_CON_NOLABEL;
        if (sizes_out) sizes_out[i] = pop ? word : 0u;
    }
    gsr_select_epilogue(n, i, hit, rule.den.op, mask, counters);
}
