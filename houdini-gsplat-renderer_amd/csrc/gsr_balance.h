// gsr_balance.h -- bands of tile rows balanced by the blend work of their rows (GSR_OPT_SHARD_LAYOUT = 2 of gsr_multi).  Host only, no
// HIP, no context: gsr_debug_balance_rows (gsplat_hip.h states the contract) is this function, and tests/test_balanced_bands.py holds it
// to a brute-force search.
//
// The optimum: the smallest limit L under which a greedy walk needs at most `count` bands (bisection over 64-bit sums; splitting a band
// never raises a sum, so "at most count" bands can always be cut further into exactly count non-empty ones while tiles_y >= count).
// The tie-break: boundary by boundary from the first, the feasible position closest to layout 1's equal split (the smaller one on a
// tie); a position is feasible when its band stays within L and the rows behind it still fit into the bands that are left.
#pragma once
#include <stdint.h>
#include <vector>

// layout 1's boundaries: bands of ceil(tiles_y / count) rows, the trailing ones shorter or empty
static inline void gsr_equal_split(int tiles_y, int count, int32_t* first /* [count + 1] */)
{
    const int rpb = (tiles_y + count - 1) / count;
    for (int g = 0; g <= count; ++g) first[g] = (int32_t)((int64_t)g * rpb < tiles_y ? g * rpb : tiles_y);
    first[count] = tiles_y;
}

// the largest band sum of a partition
static inline uint64_t gsr_bands_max(const uint32_t* row_work, int count, const int32_t* first)
{
    uint64_t worst = 0;
    for (int g = 0; g < count; ++g) {
        uint64_t s = 0;
        for (int r = first[g]; r < first[g + 1]; ++r) s += row_work[r];
        if (s > worst) worst = s;
    }
    return worst;
}

// -> 1 changed, 0 kept, -1 bad argument
static inline int gsr_balance_rows(const uint32_t* row_work, int tiles_y, int count, const int32_t* cur_first, int min_gain_permille,
                                   int32_t* out_first)
{
    if (!row_work || !out_first || tiles_y < 1 || tiles_y > 1024 || count < 1 || count > 64 || min_gain_permille < 0 || min_gain_permille > 1000)
        return -1;
    if (cur_first) {
        if (cur_first[0] != 0 || cur_first[count] != tiles_y) return -1;
        for (int g = 0; g < count; ++g)
            if (cur_first[g + 1] < cur_first[g]) return -1;
    }
    std::vector<int32_t> eq((size_t)count + 1), prop((size_t)count + 1);
    gsr_equal_split(tiles_y, count, eq.data());
    std::vector<uint64_t> pre((size_t)tiles_y + 1, 0);
    uint64_t biggest = 0;
    for (int r = 0; r < tiles_y; ++r) {
        pre[r + 1] = pre[r] + row_work[r];
        if (row_work[r] > biggest) biggest = row_work[r];
    }
    const uint64_t total = pre[tiles_y];
    if (total == 0) {
        prop = eq;                                   // nothing to balance: layout 1 itself
    } else if (count >= tiles_y) {
        for (int g = 0; g <= count; ++g) prop[g] = g < tiles_y ? g : tiles_y;   // a row each; the trailing bands are empty
    } else {
        // reach(i, L): one past the last row of the longest band that begins at row i and stays within L (>= i + 1 for L >= biggest)
        auto bands_needed = [&](uint64_t L) {
            int k = 0;
            for (int i = 0; i < tiles_y; ++k) {
                int j = i + 1;
                while (j < tiles_y && pre[j + 1] - pre[i] <= L) ++j;
                i = j;
            }
            return k;
        };
        uint64_t lo = biggest, hi = total;           // the answer lies in [lo, hi]; bands_needed(hi) = 1
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (bands_needed(mid) <= count) hi = mid; else lo = mid + 1;
        }
        const uint64_t L = lo;
        // need[i]: the fewest bands within L that hold the rows [i, tiles_y)
        std::vector<int32_t> need((size_t)tiles_y + 1, 0), reach((size_t)tiles_y + 1, tiles_y);
        for (int i = tiles_y - 1, j = tiles_y; i >= 0; --i) {
            while (pre[j] - pre[i] > L) --j;         // (j > i: a single row fits)
            reach[i] = j;
            need[i] = 1 + need[j];
        }
        prop[0] = 0; prop[count] = tiles_y;
        for (int g = 1; g < count; ++g) {
            const int left = count - g;              // bands behind this boundary
            auto feasible = [&](int b) {
                return b > prop[g - 1] && b <= reach[prop[g - 1]] && tiles_y - b >= left && need[b] <= left;
            };
            int pick = -1;
            for (int d = 0; d <= tiles_y && pick < 0; ++d) {
                if (eq[g] - d >= 1 && feasible(eq[g] - d)) pick = eq[g] - d;
                else if (d > 0 && eq[g] + d < tiles_y && feasible(eq[g] + d)) pick = eq[g] + d;
            }
            if (pick < 0) return -1;                 // (cannot happen: L is feasible)
            prop[g] = pick;
        }
    }
    bool adopt = true;
    if (cur_first) {
        const uint64_t was = gsr_bands_max(row_work, count, cur_first), now = gsr_bands_max(row_work, count, prop.data());
        adopt = now * 1000ull <= was * (uint64_t)(1000 - min_gain_permille);   // (sums < 2^42: no overflow)
    }
    bool changed = cur_first == nullptr;
    for (int g = 0; g <= count; ++g) {
        out_first[g] = adopt ? prop[g] : cur_first[g];
        if (cur_first && out_first[g] != cur_first[g]) changed = true;
    }
    return changed ? 1 : 0;
}
