"""The host model of the depth horizons (tests/horizon_ref.py) against brute force, and its constants against the headers.  No GPU.

pyr_max is what lets k_tile_pass check a tile against the look-up of the tile itself, so two properties carry the whole scheme: over a
pyramid of plain block maxima it is never below the true maximum of level 0 over the rect, and it is monotone under rect inclusion.
Both are checked EXHAUSTIVELY, over every rect of grids that reach every level, the walk over up to 4 x 4 top cells and the +inf
beyond it (257 x 3); level 0 holds random values with +inf, 0 and equal neighbours among them.  The dilation is held to a double loop
at every radius it supports.  The constants the model restates are parsed out of the headers, so a retune of the kernels fails here."""
import os
import re

import numpy as np
import pytest

import horizon_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "houdini-gsplat-renderer_amd", "csrc")
GRIDS = [(1, 1), (7, 5), (13, 8), (33, 17), (41, 19), (257, 3)]          # (tiles_x, tiles_y)


def _level0(tx, ty, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 40.0, (ty, tx)).astype(np.float32)
    pick = rng.uniform(size=(ty, tx))
    v[(pick < 0.08) & (np.arange(tx) < 40)] = np.inf                      # (the wide grid keeps top-level cells without one)
    v[(pick >= 0.08) & (pick < 0.2)] = 0.0
    eq = (pick >= 0.2) & (pick < 0.35)
    eq[:, 0] = False
    v[eq] = np.roll(v, 1, axis=1)[eq]                                      # equal neighbours
    return v


def _signed(tx, ty, seed):
    rng = np.random.default_rng(seed + 1000)
    v = _level0(tx, ty, seed)
    return np.where(rng.uniform(size=v.shape) < 0.2, -v, v).astype(np.float32)   # (-0.0 and -inf among them)


def _all_rects(tx, ty):
    xs = np.array([(a, b) for a in range(tx) for b in range(a, tx)], np.int64)
    ys = np.array([(a, b) for a in range(ty) for b in range(a, ty)], np.int64)
    x0, y0 = np.meshgrid(xs[:, 0], ys[:, 0], indexing="ij")
    x1, y1 = np.meshgrid(xs[:, 1], ys[:, 1], indexing="ij")
    return x0.ravel(), y0.ravel(), x1.ravel(), y1.ravel(), (len(xs), len(ys))


def _true_max(l0, x0, y0, x1, y1):
    """the maximum of level 0 over every rect, by running maxima: row-interval maxima first, then column-interval maxima of those"""
    ty, tx = l0.shape
    rowmax = np.zeros((ty, tx, tx), np.float32)                  # [y, a, b] = max l0[y, a..b]
    for a in range(tx):
        rowmax[:, a, a:] = np.maximum.accumulate(l0[:, a:], axis=1)
    out = np.empty(x0.shape, np.float32)
    for c in range(ty):
        acc = np.maximum.accumulate(rowmax[c:], axis=0)         # [d - c, a, b] = max over rows c..d
        m = y0 == c
        out[m] = acc[y1[m] - c, x0[m], x1[m]]
    return out


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_pyr_max_bounds_the_true_maximum_and_is_monotone(grid):
    tx, ty = grid
    l0 = _level0(tx, ty, 11 * tx + ty)
    levels, _ = HR.dilate_and_pyramid(l0, 0, HR.pyr_offsets(tx, ty))
    x0, y0, x1, y1, (nx, ny) = _all_rects(tx, ty)
    h, L, br = HR.pyr_max(levels, x0, y0, x1, y1)
    true = _true_max(l0, x0, y0, x1, y1)
    assert (h >= true).all(), "a look-up below the largest horizon of its rect"
    assert (h[br == HR.LK_INF] == np.inf).all()
    single = (x0 == x1) & (y0 == y1)
    assert np.array_equal(h[single], l0[y0[single], x0[single]]) and (L[single] == 0).all(), "a single tile reads level 0"
    # monotone: growing a rect by one column or row on any side never lowers its value (every inclusion is a chain of such steps)
    key =x0 * 1000003 + x1 * 1009 + y0 * 100000007 + y1 * 10007
    order = np.argsort(key)
    skey = key[order]

    def find(a0, b0, a1, b1):
        k = a0 * 1000003 + a1 * 1009 + b0 * 100000007 + b1 * 10007
        pos = np.searchsorted(skey, k)
        assert np.array_equal(skey[pos], k)
        return order[pos]

    for dx0, dy0, dx1, dy1 in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        m = (x0 + dx0 >= 0) & (y0 + dy0 >= 0) & (x1 + dx1 < tx) & (y1 + dy1 < ty)
        big = find(x0[m] + dx0, y0[m] + dy0, x1[m] + dx1, y1[m] + dy1)
        assert (h[big] >= h[m]).all(), f"not monotone under growth by {(dx0, dy0, dx1, dy1)}"
    # the grids reach what they are here for
    want_levels = set(range({(1, 1): 0, (7, 5): 2, (13, 8): 3, (33, 17): 5, (41, 19): 5, (257, 3): 5}[grid] + 1))
    assert set(np.unique(L[br == HR.LK_CORNERS]).tolist()) == want_levels, "the grid does not reach the levels it is here for"
    if grid == (257, 3):
        assert (br == HR.LK_WALK).any() and (br == HR.LK_INF).any(), "the wide grid reaches the 4 x 4 walk and the +inf beyond it"
        walk = br == HR.LK_WALK
        assert (((x1[walk] >> 5) - (x0[walk] >> 5)) <= 3).all() and (((x1[br == HR.LK_INF] >> 5) - (x0[br == HR.LK_INF] >> 5)) > 3).all()
        assert (h[walk] < np.inf).any(), "every walk met a +inf: the walk's maximum is not under test"
    else:
        assert (br == HR.LK_CORNERS).all()


@pytest.mark.parametrize("r", [0, 1, 2, 3])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_dilation_and_levels_against_a_double_loop(grid, r):
    tx, ty = grid
    raw = _signed(tx, ty, 7 * tx + ty + r)
    levels, stat = HR.dilate_and_pyramid(raw, r, HR.pyr_offsets(tx, ty))
    neg = np.signbit(raw)
    l0 = np.zeros((ty, tx), np.float32)
    st = np.zeros((ty, tx), np.float32)
    for y in range(ty):
        for x in range(tx):
            ys, xs = slice(max(y - r, 0), min(y + r, ty - 1) + 1), slice(max(x - r, 0), min(x + r, tx - 1) + 1)
            l0[y, x] = np.abs(raw[ys, xs]).max()
            st[y, x] = 0.0 if neg[ys, xs].any() else 1.0
    assert np.array_equal(levels[0].view(np.uint32), l0.view(np.uint32)) and np.array_equal(stat, st)
    assert len(levels) == HR.PYR_LEVELS
    for l in range(1, HR.PYR_LEVELS):
        assert levels[l].shape == (HR.pyr_dim(ty, l), HR.pyr_dim(tx, l)) and levels[l].dtype == np.float32
        for y in range(levels[l].shape[0]):
            for x in range(levels[l].shape[1]):
                assert levels[l][y, x] == l0[y << l:(y + 1) << l, x << l:(x + 1) << l].max(), (l, y, x)
    if r == 0:
        assert np.array_equal(levels[0], np.abs(raw))


def test_horizon_key_and_the_drop_rule_on_chosen_values():
    f = np.float32
    kmin, kmax = int(f(2.0).view(np.uint32)), int(f(50.0).view(np.uint32))
    h = np.array([np.inf, 3.0e38, 0.0, 1.0, 2.0, 9.0, 50.0, 80.0, np.nan], f)
    hk = HR.horizon_key(h, kmin, kmax)
    b9 = int(f(9.0).view(np.uint32))
    assert hk.tolist() == [0xffffffff, 0xffffffff, 0, 0, 0, b9 - kmin, kmax - kmin, kmax - kmin, 0xffffffff]
    # one tile, one level of each: a splat AT the horizon stays, one ulp beyond it goes; no horizon keeps everything
    meta = dict(tiles_x=1, tiles_y=1, rect_shift=0, key_min=kmin, key_max=kmax)
    levels = [np.full((1, 1), 9.0, f)] * HR.PYR_LEVELS
    key = np.array([9.0, np.nextafter(f(9.0), f(10.0)), 3.0, 49.0], f)
    drop, L, br = HR.k1_drops(np.zeros(4, np.uint32), key, levels, meta, 2)
    assert drop.tolist() == [False, True, False, True] and (L == 0).all() and (br == HR.LK_CORNERS).all()
    drop, _, _ = HR.k1_drops(np.zeros(4, np.uint32), key, [np.full((1, 1), np.inf, f)] * HR.PYR_LEVELS, meta, 0)
    assert not drop.any()
    # rects in pairs of tiles (rect_shift = 1) are unpacked outwards and clamped to the grid
    x0, y0, x1, y1 = HR.unpack_rect(np.array([3 | (1 << 8) | (4 << 16) | (1 << 24)], np.uint32), 1)
    assert (int(x0[0]), int(y0[0]), int(x1[0]), int(y1[0])) == (6, 2, 9, 3)


def test_raw_rule_on_hand_made_tiles():
    """one super-tile list of 6000 entries with key = position; six tiles, one per rule"""
    f = np.float32
    keys = np.arange(6000, dtype=f)

    def word(opaque=1, first=0, geom=0, unc=0, es_all=0xff, es_u=0xff):
        return opaque | (first << 1) | (geom << 14) | (unc << 15) | (es_all << 16) | (es_u << 24)

    tw = np.zeros((1, 6, 4), np.uint32)
    tw[0, 0] = (2000, 0, 0, word())                          # c2: want = 2000 + 500 + 1024 = 3524
    tw[0, 1] = (5000, 0, 0, word(first=2, es_all=4))         # rd = 4096, first = 2048: want = 4096 + 512 + 1024 = 5632 < 6000
    tw[0, 2] = (5500, 0, 0, word())                          # too short: 5500 + 1375 + 1024 > 6000
    tw[0, 3] = (700, 0, 0, word(opaque=0))                   # open
    tw[0, 4] = (0, 0, 0, word(opaque=0, unc=1, es_u=0))      # uncovered pixels needed nothing: none, not classic
    tw[0, 5] = (900, 0, 0, word(geom=1, unc=1, es_u=0xff))   # met geometry: the sign is set, horizon from the uncovered pixels' scan
    args = dict(tiles_y=1, shard=HR.Shard(), super_shift=3, stiles_x=1, list_cap=1 << 20)
    raw, broke, br = HR.raw_horizons(tw, [0], [6000], keys, **args)
    assert br[0].tolist() == [HR.BR_C2, HR.BR_C2, HR.BR_UNPLACED, HR.BR_OPEN, HR.BR_NONE, HR.BR_C2]
    assert raw[0, :2].tolist() == [3524.0, 5632.0] and raw[0, 2] == np.inf and raw[0, 3] == -np.inf
    assert raw[0, 4] == 0 and np.signbit(raw[0, 4]) and raw[0, 5] == -(900 + 225 + 1024) and not broke.any()
    # the same frame culled against horizons of 3000 everywhere, depth-culled: the short list takes the old horizon pushed out; tile 0
    # (last entry scanned 1999 <= 3000) holds, tiles 1 and 2 looked past 3000 and break, the open tile breaks
    pyr = [np.full((1, HR.pyr_dim(6, l)), 3000.0, f) for l in range(HR.PYR_LEVELS)]
    raw, broke, br = HR.raw_horizons(tw, [0], [6000], keys, pyr_in=pyr, cull=True, cull_dilate=1, depth_culled=True, **args)
    assert br[0].tolist() == [HR.BR_C2, HR.BR_C2, HR.BR_HOLD, HR.BR_OPEN, HR.BR_NONE, HR.BR_C2]
    assert raw[0, 2] == f(3000.0) * f(1.05) and broke[0].tolist() == [False, True, True, True, True, False]
    # without horizons but behind a depth buffer the short list's last entry, pushed out, stands in (c3); another rank's row reads 0
    tw2 = np.concatenate([tw, tw])
    raw, broke, br = HR.raw_horizons(tw, [0], [6000], keys, depth_culled=True, **args)
    assert br[0, 2] == HR.BR_C3 and raw[0, 2] == f(5999.0) * f(1.05) and not broke.any()
    raw, broke, br = HR.raw_horizons(tw2[:1], [0], [6000], keys, **{**args, "tiles_y": 2, "shard": HR.Shard(1, 2)})
    assert (br[0] == HR.BR_OTHER).all() and (raw[0].view(np.uint32) == 0).all() and br[1, 0] == HR.BR_C2
    # the incoming status: a tile predicted NOT classic is checked by its uncovered pixels (tile 4 promised and needed nothing)
    stat = np.zeros((1, 6), f)
    _, broke, _ = HR.raw_horizons(tw, [0], [6000], keys, pyr_in=pyr, cull=True, stat_in=stat, stat_in_use=True, **args)
    assert broke[0].tolist() == [False, True, True, True, False, False]


def _define(text, name):
    return re.search(r"#define\s+%s\s+([^\s/]+)" % name, text).group(1)


def test_the_models_constants_are_the_headers():
    blend = open(os.path.join(CSRC, "k_blend.h")).read()
    cluster = open(os.path.join(CSRC, "k_cluster.h")).read()
    pre = open(os.path.join(CSRC, "k_preprocess.h")).read()
    dev = open(os.path.join(CSRC, "gsr_device.h")).read()
    assert int(_define(cluster, "GSR_PYR_LEVELS")) == HR.PYR_LEVELS
    assert int(_define(cluster, "GSR_DILATE_EXACT_MAX")) == HR.DILATE_EXACT_MAX
    assert int(_define(blend, "SW_HEADROOM_SHIFT")) == HR.HEADROOM_SHIFT
    assert int(_define(blend, "SW_HEADROOM_ADD").rstrip("u")) == HR.HEADROOM_ADD
    # k_tile_pass places the horizon by the two constants (and k_slab_mid and the prefix rule with it)
    tile_pass = blend[blend.index("k_tile_pass(const uint4*"):blend.index("k_slab_mid(const uint4*")]
    assert re.search(r"const uint32_t want = rd \+ \(\(rd > first \? rd - first : 0u\) >> SW_HEADROOM_SHIFT\) \+ SW_HEADROOM_ADD;", tile_pass)
    # "a horizon" is `< 3.0e38f` wherever one is tested, and nothing else
    for name, text in (("k_blend.h", tile_pass), ("gsr_device.h", dev[dev.index("gsr_horizon_key("):dev.index("// rect packing")]),
                       ("k_preprocess.h", pre[pre.index("gsr_k1_back(GsrFrameArg"):pre.index("struct GsrK1Scatter")])):
        sentinels = set(re.findall(r"<\s*([0-9.]+e38)f", text))
        assert sentinels == {"3.0e38"}, (name, sentinels)
        assert np.float32(float(sentinels.pop())) == HR.NO_HORIZON
    pushes = re.findall(r"h = (?:hold|hnew) \* ([0-9.]+)f;", tile_pass)
    assert len(pushes) == 2 and all(np.float32(float(p)) == HR.PUSH_OUT for p in pushes), pushes
    # the drop rule itself
    assert re.search(r"beyond = o\.kb > gsr_horizon_key\(h, f\.key_min, f\.key_max\);", pre)
    assert re.search(r"gsr_pyr_dim\(int tiles, int level\) \{ return \(\(tiles - 1\) >> level\) \+ 1; \}", cluster)
