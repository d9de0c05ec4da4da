"""Balanced bands without a GPU: the balancer (csrc/gsr_balance.h through gsr_debug_balance_rows) against a brute-force search, its
degenerate inputs and its hysteresis, and the new verbs' refusals through the C ABI.

The brute force restates the contract of include/gsplat_hip.h: among all contiguous partitions of [0, tiles_y) into `count` bands
(every band non-empty while tiles_y >= count) those with the smallest largest band sum, and among them the one whose interior
boundaries are closest to layout 1's equal split e[g] = min(g * ceil(tiles_y / count), tiles_y), boundary by boundary from the first
(|b[g] - e[g]|, then the smaller b[g]).  All-zero work is layout 1 itself; count > tiles_y is a row each."""
import ctypes as C
import itertools

import numpy as np
import pytest


def equal_split(tiles_y, count):
    rpb = -(-tiles_y // count)
    return [min(g * rpb, tiles_y) for g in range(count)] + [tiles_y]


def band_sums(work, first):
    return [int(sum(int(x) for x in work[first[g]:first[g + 1]])) for g in range(len(first) - 1)]


def brute_force(work, count):
    tiles_y = len(work)
    e = equal_split(tiles_y, count)
    if sum(int(x) for x in work) == 0:
        return 0, e
    if count >= tiles_y:
        return max(int(x) for x in work), [min(g, tiles_y) for g in range(count + 1)]
    best = None
    for cut in itertools.combinations(range(1, tiles_y), count - 1):
        first = [0] + list(cut) + [tiles_y]
        worst = max(band_sums(work, first))
        key = (worst,) + tuple(v for g in range(1, count) for v in (abs(first[g] - e[g]), first[g]))
        if best is None or key < best[0]:
            best = (key, first)
    return best[0][0], best[1]


def test_balancer_matches_brute_force(pkg):
    rng = np.random.default_rng(2024)
    E = pkg.engine
    cases = 0
    for tiles_y in range(1, 13):
        for count in range(1, 5):
            for trial in range(6):
                kind = trial % 3
                if kind == 0:
                    work = rng.integers(0, 1000, tiles_y)
                elif kind == 1:     # many ties: few distinct values, zeros among them
                    work = rng.integers(0, 3, tiles_y) * 7
                else:               # a landscape: heavy rows below, sky above
                    work = (rng.integers(0, 50, tiles_y) + np.where(np.arange(tiles_y) < tiles_y // 2, 5000, 0))
                work = work.astype(np.uint32)
                changed, first = E.balance_rows(work, count)
                want_max, want_first = brute_force(work, count)
                first = first.tolist()
                assert changed is True
                assert first[0] == 0 and first[-1] == tiles_y and all(b >= a for a, b in zip(first, first[1:])), (work, count, first)
                assert max(band_sums(work, first)) == want_max, (work.tolist(), count, first, want_first)
                assert first == want_first, (work.tolist(), count, first, want_first)
                if tiles_y >= count and work.sum() > 0:
                    assert all(b > a for a, b in zip(first, first[1:])), "every band holds a row"
                cases += 1
    assert cases == 12 * 4 * 6


def test_balancer_degenerate_inputs(pkg):
    E = pkg.engine
    # all-zero work: layout 1's boundaries, ceil(tiles_y / count) rows per band (the last ones shorter, or empty)
    for tiles_y, count in [(10, 4), (9, 4), (15, 2), (15, 3), (5, 4), (68, 8), (1, 1), (3, 8)]:
        _, first = E.balance_rows(np.zeros(tiles_y, np.uint32), count)
        assert first.tolist() == equal_split(tiles_y, count), (tiles_y, count)
    # more ranks than rows: a row each, the trailing bands empty
    _, first = E.balance_rows(np.array([5, 1, 9], np.uint32), 5)
    assert first.tolist() == [0, 1, 2, 3, 3, 3]
    # one row holds all the work: it gets a band of its own where it can, and the optimum is that row
    work = np.zeros(12, np.uint32)
    work[7] = 123456
    _, first = E.balance_rows(work, 4)
    assert max(band_sums(work, first.tolist())) == 123456 and first.tolist() == brute_force(work, 4)[1]
    # sums near 2^32 per row: 64-bit accumulation (a 32-bit sum of two rows wraps to almost nothing and would merge them)
    big = np.full(8, 0xFFFFFFF0, np.uint32)
    _, first = E.balance_rows(big, 4)
    assert first.tolist() == [0, 2, 4, 6, 8]
    big2 = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1, 1, 1], np.uint32)
    _, first = E.balance_rows(big2, 3)
    assert max(band_sums(big2, first.tolist())) == 0xFFFFFFFF + 3 and first.tolist() == brute_force(big2, 3)[1]


def test_balancer_hysteresis(pkg):
    E = pkg.engine
    # current: [0, 2, 4] over work 600 | 400 || 0 | 0  -> largest band 1000; the proposal [0, 1, 4] has 600: a gain of exactly 400 permille
    work = np.array([600, 400, 0, 0], np.uint32)
    cur = np.array([0, 2, 4], np.int32)
    _, prop = E.balance_rows(work, 2)
    assert prop.tolist() == [0, 1, 4]
    changed, first = E.balance_rows(work, 2, cur, 401)
    assert changed is False and first.tolist() == cur.tolist(), "a proposal below the threshold is not adopted"
    changed, first = E.balance_rows(work, 2, cur, 400)
    assert changed is True and first.tolist() == [0, 1, 4], "a proposal exactly at the threshold is adopted"
    changed, first = E.balance_rows(work, 2, cur, 0)
    assert changed is True and first.tolist() == [0, 1, 4]
    # min_gain_permille = 0 adopts even a proposal that gains nothing
    flat = np.array([5, 5, 5, 5], np.uint32)
    changed, first = E.balance_rows(flat, 2, np.array([0, 2, 4], np.int32), 0)
    assert changed is False and first.tolist() == [0, 2, 4], "the proposal IS the current partition: kept"
    changed, first = E.balance_rows(np.array([9, 0, 0, 9], np.uint32), 2, np.array([0, 1, 4], np.int32), 0)
    assert changed is True and first.tolist() == [0, 2, 4], "same largest sum, closer to the equal split: adopted at gain 0"
    changed, first = E.balance_rows(np.array([9, 0, 0, 9], np.uint32), 2, np.array([0, 1, 4], np.int32), 1)
    assert changed is False and first.tolist() == [0, 1, 4]


def test_c_abi_refusals_without_a_gpu(pkg):
    E = pkg.engine
    L = pkg.load_library()
    INVALID = -1
    out = np.zeros(4, np.uint32)
    frame = C.c_int64(0)
    assert L.gsr_set_row_band(None, 0, 1) == INVALID
    assert b"gsr_set_row_band" in L.gsr_last_error()
    assert L.gsr_read_row_work(None, out.ctypes.data, 4, C.byref(frame)) == INVALID
    assert L.gsr_multi_get_bands(None, None, None) == INVALID
    assert E.OPT_ROW_WORK == 17
    first = np.zeros(3, np.int32)
    work = np.ones(4, np.uint32)
    bad = [
        (None, 4, 2, None, 0, first.ctypes.data),                                  # no work
        (work.ctypes.data, 4, 2, None, 0, None),                                   # no output
        (work.ctypes.data, 0, 2, None, 0, first.ctypes.data),                      # no rows
        (work.ctypes.data, 4, 0, None, 0, first.ctypes.data),                      # no bands
        (work.ctypes.data, 4, 2, None, -1, first.ctypes.data),                     # gain outside 0..1000
        (work.ctypes.data, 4, 2, None, 1001, first.ctypes.data),
        (work.ctypes.data, 4, 2, np.array([0, 3, 5], np.int32).ctypes.data, 0, first.ctypes.data),   # cur_first does not end at tiles_y
        (work.ctypes.data, 4, 2, np.array([0, 5, 4], np.int32).ctypes.data, 0, first.ctypes.data),   # ... is not monotone
        (work.ctypes.data, 4, 2, np.array([1, 2, 4], np.int32).ctypes.data, 0, first.ctypes.data),   # ... does not begin at 0
    ]
    for args in bad:
        assert L.gsr_debug_balance_rows(*args) < 0, args
    with pytest.raises(E.GsrError):
        E.balance_rows(work, 2, min_gain_permille=2000)


def test_band_helpers_for_an_explicit_band(pkg):
    mg = pkg.multigpu
    full = np.arange(150 * 3 * 4, dtype=np.float32).reshape(150, 3, 4)             # 10 tile rows, the last 6 pixel rows high
    assert mg.owned_tile_rows(150, band=(1, 6)) == [1, 2, 3, 4, 5, 6]
    assert mg.owned_tile_rows(150, band=(9, 3)) == [9] and mg.owned_tile_rows(150, band=(4, 0)) == []
    b = mg.extract_band(full, band=(9, 3))
    assert b.shape == (48, 3, 4) and np.array_equal(b[:6], full[144:]) and not b[6:].any()
    assert np.array_equal(mg.extract_band(full, band=(1, 6)), full[16:112])
    assert mg.extract_band(full, band=(4, 0)).shape == (0, 3, 4)
    # the sharded forms are what they were
    assert mg.owned_tile_rows(150, 1, 3, 1) == [4, 5, 6, 7] and mg.owned_tile_rows(150, 1, 3) == [1, 4, 7]
