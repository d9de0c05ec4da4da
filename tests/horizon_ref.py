"""A host model of the depth horizons, their max pyramid and the drop rule, in numpy with exact float32 / uint32
arithmetic: no tolerance anywhere.  The rules are restated from the comments and code of csrc/k_blend.h (k_tile_pass,
gsr_horizon_dilate), csrc/k_cluster.h (gsr_pyr_dim, gsr_pyr_max), csrc/k_preprocess.h (gsr_k1_back) and csrc/gsr_device.h
(gsr_horizon_key, the rect packing, the shard rules); tests/test_horizon_ref.py holds the constants below to the headers and the model to
brute force, tests/test_horizons_gpu.py holds the kernels to the model.

  raw_horizons        k_tile_pass: the per-tile horizon a frame leaves for the slot's next one, with the tile's status in the sign,
                      and whether the tile broke the promise it made for THIS frame
  dilate_and_pyramid  gsr_horizon_dilate: level 0, the status plane, levels 1..5
  pyr_max             gsr_pyr_max: the look-up, with the level and branch every rect took
  k1_drops            gsr_k1_back's rule for a frame without a depth buffer
"""
import numpy as np

PYR_LEVELS = 6                     # GSR_PYR_LEVELS
DILATE_EXACT_MAX = 3               # GSR_DILATE_EXACT_MAX: the radius the dilation applies tile by tile
HEADROOM_SHIFT = 2                 # SW_HEADROOM_SHIFT: a quarter of what the tile scanned from its first hit on ...
HEADROOM_ADD = 1024                # SW_HEADROOM_ADD: ... plus this many entries
NO_HORIZON = np.float32(3.0e38)    # "h < 3.0e38f": a horizon; anything else (+inf, NaN) is none
PUSH_OUT = np.float32(1.05)        # a horizon that cannot be placed is the old one pushed out by 5 % (in distance^2)

# which rule gave a tile's raw horizon
BR_OTHER, BR_OPEN, BR_NONE, BR_C2, BR_HOLD, BR_C3, BR_UNPLACED = range(7)
BRANCH_NAMES = ("other-rank", "open", "none", "c2", "hold x 1.05", "c3", "opaque, unplaced")
# which path a look-up took
LK_CORNERS, LK_WALK, LK_INF = range(3)

F32_INF = np.float32(np.inf)


def pyr_dim(tiles, level):
    return ((int(tiles) - 1) >> level) + 1


def pyr_offsets(tiles_x, tiles_y):
    off, o = [], 0
    for l in range(PYR_LEVELS):
        off.append(o)
        o += pyr_dim(tiles_x, l) * pyr_dim(tiles_y, l)
    return off


class Shard:
    """tile-row ownership of a rank (gsr_device.h: GsrShard): interleaved rows (rpb == 0) or the band [first, first + rpb)"""

    def __init__(self, index=0, count=1, rpb=0, first=0):
        self.index, self.count, self.rpb, self.first = int(index), int(count), int(rpb), int(first)

    def owns(self, rows):
        rows = np.asarray(rows, np.int64)
        if self.rpb > 0:
            return (rows >= self.first) & (rows - self.first < self.rpb)
        return rows % self.count == self.index

    def local_row(self, rows):
        rows = np.asarray(rows, np.int64)
        return rows - self.first if self.rpb > 0 else rows // self.count


def _floor_log2(v):
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for k in range(1, 32):
        out += (v >> k) > 0
    return out


def pyr_max(levels, x0, y0, x1, y1):
    """gsr_pyr_max over the tile rects [x0, x1] x [y0, y1] (arrays; inside the grid).  -> (h float32, level int, branch LK_*): the
    level the rect's 2 x 2 corners were read at, or PYR_LEVELS - 1 for the walk over up to 4 x 4 top cells; +inf beyond that."""
    x0, y0, x1, y1 = (np.atleast_1d(np.asarray(v, np.int64)) for v in (x0, y0, x1, y1))
    assert len(levels) == PYR_LEVELS and (x0 <= x1).all() and (y0 <= y1).all() and (x0 >= 0).all() and (y0 >= 0).all()
    assert (x1 < levels[0].shape[1]).all() and (y1 < levels[0].shape[0]).all()
    span = np.maximum(x1 - x0, y1 - y0)
    L = _floor_log2(span | 1)
    L = L + ((((x1 >> L) - (x0 >> L)) > 1) | (((y1 >> L) - (y0 >> L)) > 1))
    h = np.full(x0.shape, F32_INF, np.float32)
    branch = np.full(x0.shape, LK_INF, np.int64)
    for l in range(PYR_LEVELS):
        m = L == l
        if not m.any():
            continue
        p = levels[l]
        a0, a1, b0, b1 = x0[m] >> l, x1[m] >> l, y0[m] >> l, y1[m] >> l
        h[m] = np.maximum(np.maximum(p[b0, a0], p[b0, a1]), np.maximum(p[b1, a0], p[b1, a1]))
        branch[m] = LK_CORNERS
    T = PYR_LEVELS - 1
    top = levels[T]
    a0, a1, b0, b1 = x0 >> T, x1 >> T, y0 >> T, y1 >> T
    walk = (L >= PYR_LEVELS) & (a1 - a0 <= 3) & (b1 - b0 <= 3)
    hw = np.zeros(x0.shape, np.float32)
    for db in range(4):
        for da in range(4):
            use = walk & (a0 + da <= a1) & (b0 + db <= b1)
            bb, aa = np.where(use, b0 + db, 0), np.where(use, a0 + da, 0)
            hw = np.where(use, np.maximum(hw, top[bb, aa]), hw)
    h[walk] = hw[walk]
    branch[walk] = LK_WALK
    return h, np.where(L < PYR_LEVELS, L, T), branch


def dilate_and_pyramid(raw, r, offsets=None):
    """gsr_horizon_dilate: level 0 = the largest |raw| over the (2r + 1)^2 neighbourhood clamped to the grid, the status plane = 1 where
    every sign of that neighbourhood is clear, levels 1..5 = block maxima of level 0 over 2^l x 2^l tiles.  -> (levels, status)"""
    raw = np.asarray(raw, np.float32)
    ty, tx = raw.shape
    r = int(r)
    assert 0 <= r <= DILATE_EXACT_MAX
    if offsets is not None:
        assert list(offsets) == pyr_offsets(tx, ty), "the pyramid's layout is not the model's"
    mag = np.abs(raw)
    neg = (raw.view(np.uint32) >> 31) != 0
    pm = np.zeros((ty + 2 * r, tx + 2 * r), np.float32)          # (|raw| >= 0: zeros outside the grid change no maximum)
    pn = np.zeros((ty + 2 * r, tx + 2 * r), bool)
    pm[r:r + ty, r:r + tx] = mag
    pn[r:r + ty, r:r + tx] = neg
    l0 = np.zeros((ty, tx), np.float32)
    anyneg = np.zeros((ty, tx), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            l0 = np.maximum(l0, pm[dy:dy + ty, dx:dx + tx])
            anyneg |= pn[dy:dy + ty, dx:dx + tx]
    levels = [l0]
    for l in range(1, PYR_LEVELS):
        b = 1 << l
        h, w = pyr_dim(ty, l), pyr_dim(tx, l)
        pad = np.zeros((h * b, w * b), np.float32)
        pad[:ty, :tx] = l0
        levels.append(pad.reshape(h, b, w, b).max(axis=(1, 3)))
    return levels, np.where(anyneg, np.float32(0), np.float32(1)).astype(np.float32)


def horizon_key(h, key_min, key_max):
    """gsr_horizon_key: a horizon in a frame's sort-key domain (uint32 arrays as int64)"""
    h = np.asarray(h, np.float32)
    b = np.where(h > 0, h, np.float32(0)).astype(np.float32).view(np.uint32).astype(np.int64)
    b = np.clip(b, int(key_min), int(key_max)) - int(key_min)
    return np.where(h < NO_HORIZON, b, 0xffffffff)


def unpack_rect(rect, rect_shift):
    """a packed rect in tiles: x0, y0, x1, y1 (x1, y1 inclusive, NOT clamped to the grid)"""
    rect = np.asarray(rect, np.uint32).astype(np.int64)
    g = int(rect_shift)
    return (rect & 255) << g, ((rect >> 8) & 255) << g, ((((rect >> 16) & 255) + 1) << g) - 1, (((rect >> 24) + 1) << g) - 1


def k1_drops(rect, key, levels, meta, cull_dilate):
    """gsr_k1_back's rule without a depth buffer: the splat's rect, widened by cull_dilate tiles and clamped to the grid, is looked up
    in the pyramid; the splat is dropped iff its stored key lies beyond that horizon's.  key: distance^2 as float32 (unclamped bits).
    -> (dropped, level, branch)"""
    tx, ty = int(meta["tiles_x"]), int(meta["tiles_y"])
    x0, y0, x1, y1 = unpack_rect(rect, meta["rect_shift"])
    r = int(cull_dilate)
    h, L, br = pyr_max(levels, np.maximum(x0 - r, 0), np.maximum(y0 - r, 0), np.minimum(x1 + r, tx - 1), np.minimum(y1 + r, ty - 1))
    kmin, kmax = int(meta["key_min"]), int(meta["key_max"])
    kb = np.clip(np.asarray(key, np.float32).view(np.uint32).astype(np.int64), kmin, kmax) - kmin
    return kb > horizon_key(h, kmin, kmax), L, br


def raw_horizons(tile_work, list_start, list_end, entry_key, tiles_y, shard, super_shift, stiles_x, list_cap,
                 pyr_in=None, cull=False, cull_dilate=0, stat_in=None, stat_in_use=False, depth_culled=False):
    """k_tile_pass for a frame that is no front slab.
    tile_work  [local rows, tiles_x, 4] uint32: the blend kernel's bookkeeping of the shard's tiles.  Word 0 = list entries scanned;
               word 3: bit 0 every pixel opaque, bits 1-13 the 1024-entry step of the first hit, bit 14 met geometry, bit 15 the
               uncovered pixels opaque, bits 16-23 es_all, bits 24-31 es_u (the step that held everything gathered; 0xff = unknown)
    list_start / list_end, entry_key   the super-tile lists and the key (distance^2, float32) of every list entry
    pyr_in, cull, cull_dilate          the pyramid the frame was culled against (if it was) and the plan's widening (the dilation
                                       BUILT INTO pyr_in is no input: the plan's cull_dilate is what remains of the policy's on top of it)
    stat_in, stat_in_use               the incoming status plane, and whether the frame's K1 applied it
    depth_culled                       the frame's K1 dropped splats behind the depth buffer where no horizon applied
    -> (raw [tiles_y, tiles_x] float32 with the status sign, broke [tiles_y, tiles_x] bool, branch [tiles_y, tiles_x] BR_*)"""
    tw = np.asarray(tile_work, np.uint32).astype(np.int64)
    local_rows, tiles_x = tw.shape[0], tw.shape[1]
    n_tiles = local_rows * tiles_x
    gty, tx = np.meshgrid(np.arange(tiles_y, dtype=np.int64), np.arange(tiles_x, dtype=np.int64), indexing="ij")
    lty = shard.local_row(gty)
    own = shard.owns(gty) & (lty >= 0) & (lty * tiles_x + tx < n_tiles)
    w = np.where(own[..., None], tw[np.where(own, lty, 0), tx], 0)
    w0, w3 = w[..., 0], w[..., 3]
    st = (gty >> super_shift) * stiles_x + (tx >> super_shift)
    st = np.where(own, st, 0)
    s0 = np.asarray(list_start, np.int64)[st]
    e0 = np.minimum(np.asarray(list_end, np.int64)[st], int(list_cap))
    length = np.where(own & (e0 > s0), e0 - s0, 0)
    hold = np.full(gty.shape, F32_INF, np.float32)
    if cull:     # (at least) the value of the tile itself, widened like every rect
        r = int(cull_dilate)
        hv, _, _ = pyr_max(pyr_in, np.maximum(tx - r, 0).ravel(), np.maximum(gty - r, 0).ravel(),
                           np.minimum(tx + r, tiles_x - 1).ravel(), np.minimum(gty + r, tiles_y - 1).ravel())
        hold = np.where(own, hv.reshape(gty.shape), F32_INF).astype(np.float32)
    has_hold = hold < NO_HORIZON

    def depth_read(es):          # how deep the tile looked: the steps that hold everything it gathered, never more than it read
        return np.where((es == 0xff) | ((es << 10) > w0), w0, es << 10)

    rd_all, rd_u = depth_read((w3 >> 16) & 0xff), depth_read((w3 >> 24) & 0xff)
    opaque_all = own & ((w3 & 1) != 0)
    classic_now = opaque_all & ((w3 & 0x4000) == 0)
    unc_opaque = (w3 & 0x8000) != 0
    pred_classic = np.ones(gty.shape, bool)
    if stat_in is not None and stat_in_use:
        pred_classic = np.asarray(stat_in, np.float32) != 0
    rdc = np.where(pred_classic, rd_all, rd_u)                                           # the promise that is checked
    opaque_c = own & np.where(pred_classic, opaque_all, classic_now | unc_opaque)
    rd = np.where(classic_now, rd_all, rd_u)                                             # the horizon that is left
    opaque = own & (classic_now | unc_opaque)
    first = ((w3 >> 1) & 0x1fff) << 10
    want = (rd + (np.maximum(rd - first, 0) >> HEADROOM_SHIFT) + HEADROOM_ADD) & 0xffffffff
    ok = opaque & (rd > 0) & (rd <= length)
    c1 = opaque_c & (rdc > 0) & (rdc <= length) & has_hold
    c2 = ok & (want < length)
    c3 = ok & ~c2 & ~has_hold & bool(depth_culled)
    keys = np.asarray(entry_key, np.float32)
    if keys.size == 0:
        keys = np.zeros(1, np.float32)
    klast = keys[np.where(c1, s0 + rdc - 1, 0)]
    hnew = keys[np.where(c2, s0 + want, np.where(c3, s0 + length - 1, 0))]
    none_c = opaque_c & ~pred_classic & (rdc == 0)
    none = opaque & ~classic_now & (rd == 0)
    broke = own & has_hold & ~none_c & (~opaque_c | ~c1 | ~(klast <= hold))
    pushed = (hold * PUSH_OUT).astype(np.float32)
    hnew_pushed = (hnew * PUSH_OUT).astype(np.float32)
    h = np.full(gty.shape, F32_INF, np.float32)
    branch = np.full(gty.shape, BR_OPEN, np.int64)
    placed = opaque & ~none
    for m, v, tag in ((placed & ~c2 & ~has_hold & ~c3, h, BR_UNPLACED), (placed & ~c2 & ~has_hold & c3, hnew_pushed, BR_C3),
                      (placed & ~c2 & has_hold, pushed, BR_HOLD), (placed & c2, hnew, BR_C2), (none, np.float32(0), BR_NONE),
                      (~own, np.float32(0), BR_OTHER)):
        h = np.where(m, v, h).astype(np.float32)
        branch = np.where(m, tag, branch)
    raw = np.where(own & ~classic_now, -h, h).astype(np.float32)
    return raw, broke, branch
