"""The models and the case table of the selection-overlay tests (gsr_render_marks; include/gsplat_hip.h, "selection overlay"), shared by
test_marks.py (no GPU) and test_marks_gpu.py.  Everything expected comes from yardsticks that exist -- gsr_select_eval's centres, the
oracle's wire overlay, gsr_composite_over, gsr_convert_pixels -- and numpy, never from the GPU path.

The DOT model: a splat is drawn iff its mask bit is set, gsr_select_eval says hit for the everywhere-rect and its centre lies in the
image; its fragments are the square of pixels around (int)cx, (int)cy, clipped; per pixel the smallest (bits(zw) << 32) | index wins.
The OUTLINE model: oracle.render_wire of the drawn subset in ascending upload order -- its covered pixels and its (Cd, 1) colours.
The resolve model: the winner against the depth buffer, then the colour over the decoded frame by gsr_composite_over, in the target
format, at the written pixels alone.

A case = a cloud, a camera and an origin.  Clouds of SIZES splats (the word, wave and workgroup edges) with seeded splats spread over
the upload indices: centres in the edge pixels of all four edges, in the four corners, and one pixel outside each edge; two splats at
one position with different colours; one below the opacity test and one of opacity 0."""
import types

import numpy as np

from helpers import unproject

SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
FRAMES = ((64, 48), (37, 29))
RADII = (0, 1, 8)
EMPTY = np.uint64(0xffffffffffffffff)
ORIGIN = (0.25, -0.5, 0.125)
_CACHE = {}


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def dot_keys(centres, drawn, width, height, radius):
    """the z-buffer of the DOT shape: centres float32 (n, 3) = cx, cy, zw; drawn bool (n,): mask bit set and hit -> uint64 (height, width),
    EMPTY where no dot lies.  A centre outside the image draws nothing."""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    z = np.full((height, width), EMPTY, np.uint64)
    W, H = np.float32(width), np.float32(height)
    for i in np.flatnonzero(drawn):
        cx, cy, zw = c[i]
        if not (cx >= 0 and cx < W and cy >= 0 and cy < H) or np.isnan(zw):
            continue
        qx, qy = int(cx), int(cy)
        key = (np.uint64(np.float32(zw).view(np.uint32)) << np.uint64(32)) | np.uint64(i)
        ys, xs = slice(max(qy - radius, 0), min(qy + radius, height - 1) + 1), slice(max(qx - radius, 0), min(qx + radius, width - 1) + 1)
        z[ys, xs] = np.minimum(z[ys, xs], key)
    return z


def decode(under):
    """a frame in a target format -> float32, by the background's decode rule"""
    if under.dtype == np.uint8:
        return under.astype(np.float32) / np.float32(255.0)
    return under.astype(np.float32)


def resolve(pkg, under, winner, zw, colour, Cd, fmt, depth=None, bias=0.0):
    """the resolve step.  under (H, W, 4) in the target format; winner int64 (H, W) upload index or -1; zw float32 (H, W) of the winner
    (only read under a depth buffer); colour = (r, g, b, a) or "cd" with Cd uint16 (n, 3) halves -> (image, pixels written)"""
    E = pkg.engine
    write = winner >= 0
    if depth is not None:
        with np.errstate(invalid="ignore"):
            write = write & (zw <= (np.asarray(depth, np.float32).reshape(winner.shape) + np.float32(bias)).astype(np.float32))
    D = decode(under)
    if isinstance(colour, str):
        c = np.zeros(D.shape, np.float32)
        c[write, :3] = np.asarray(Cd, np.uint16).view(np.float16)[winner[write]].astype(np.float32)
        c[write, 3] = 1.0
        over = E.composite_over(D, c, fmt)
    else:
        over = E.composite_over(D, tuple(float(x) for x in colour), fmt)
    out = under.copy()
    out[write] = over[write]
    return out, int(write.sum())


def split_keys(z):
    """uint64 keys -> (winner int64 upload index or -1, zw float32)"""
    winner = np.where(z == EMPTY, -1, (z & np.uint64(0xffffffff)).astype(np.int64))
    zw = (z >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return winner, zw


def dot_centres(pkg, case, resident_alpha=None, any_opacity=False):
    """(hit, centres) of the everywhere-rect: gsr_select_eval, the rule of a dot's first two clauses"""
    E = pkg.engine
    a = case.splats.alpha if resident_alpha is None else resident_alpha
    return E.select_eval(case.cam, case.origin, E.select_region(None, any_opacity=any_opacity), case.splats.P, a, centres=True)


def expected_dots(pkg, case, under, marked, radius, colour, fmt, depth=None, bias=0.0, resident_alpha=None, any_opacity=False):
    hit, c = dot_centres(pkg, case, resident_alpha, any_opacity)
    z = dot_keys(c, hit & marked, case.cam.width, case.cam.height, radius)
    winner, zw = split_keys(z)
    return resolve(pkg, under, winner, zw, colour, case.splats.Cd, fmt, depth, bias)


def outline_winners(oracle, splats, cam, drawn):
    """the OUTLINE shape's covered pixels and (Cd, 1) colours: oracle.render_wire of the drawn subset, ascending upload order
    -> float32 (H, W, 4), alpha 1 where covered, 0 elsewhere"""
    idx = np.flatnonzero(drawn)
    if idx.size == 0:
        return np.zeros((cam.height, cam.width, 4), np.float32)
    if hasattr(splats, "subset"):
        return oracle.render_wire(splats.subset(idx), cam)
    part = {k: (None if getattr(splats, k, None) is None else np.ascontiguousarray(getattr(splats, k)[idx])) for k in ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz")}
    return oracle.render_wire(types.SimpleNamespace(n=int(idx.size), **part), cam)          # (a golden fixture's cloud: helpers.load_golden)


def expected_outlines(pkg, oracle, case, under, marked, colour, fmt, resident_alpha=None, any_opacity=False, depth_pass=None):
    """depth_pass: bool (H, W), where a depth buffer of -1s (no window depth passes) and 1s (every one does) holds a 1; None: no test"""
    E = pkg.engine
    a = case.splats.alpha if resident_alpha is None else resident_alpha
    drawn = marked if any_opacity else marked & (a >= np.float32(1) / np.float32(255))
    wire = outline_winners(oracle, case.splats, case.cam, drawn)
    covered = wire[..., 3] > 0
    if depth_pass is not None:
        covered = covered & depth_pass
        wire = np.where(covered[..., None], wire, np.float32(0.0))
    D = decode(under)
    over = E.composite_over(D, wire if isinstance(colour, str) else tuple(float(x) for x in colour), fmt)
    out = under.copy()
    out[covered] = over[covered]
    return out, int(covered.sum())


# ---- the frames underneath ------------------------------------------------------------------------------------------------------------
def frame_under(pkg, width, height, fmt, seed=0):
    """a finite random frame (height, width, 4) in the target format: every pixel distinct from what a mark would write"""
    E = pkg.engine
    rng = np.random.default_rng(900 + seed)
    if fmt == E.TARGET_RGBA8:
        return rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
    return (rng.random((height, width, 4), dtype=np.float32) * np.float32(0.75)).astype(E.target_dtype(fmt))


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, splats, cam, origin, specials):
        self.name, self.splats, self.cam, self.origin, self.specials = name, splats, cam, tuple(origin), specials
        self.n = splats.n

    def __repr__(self):
        return self.name


SPECIALS = ("left", "right", "bottom", "top", "corner00", "corner10", "corner01", "corner11", "out_left", "out_right", "out_bottom", "out_top")


def _make(pkg, n, frame_wh, seed):
    w, h = frame_wh
    cam = pkg.camera.make_camera(w, h, sh_order=3, frame=seed % 5, near=0.01, far=50.0)
    s = pkg.scenes.make_scene(n, seed=100 + seed, sh=True, log_scale_range=(-3.5, -2.2))
    s.alpha[:] = np.maximum(s.alpha, np.float32(0.02))
    at = {}
    if n >= 31:
        xy = {"left": (0.5, h * 0.4), "right": (w - 0.5, h * 0.6), "bottom": (w * 0.3, 0.5), "top": (w * 0.7, h - 0.5),
              "corner00": (0.5, 0.5), "corner10": (w - 0.5, 0.5), "corner01": (0.5, h - 0.5), "corner11": (w - 0.5, h - 0.5),
              "out_left": (-0.5, h * 0.5), "out_right": (w + 0.5, h * 0.5), "out_bottom": (w * 0.5, -0.5), "out_top": (w * 0.5, h + 0.5)}
        step = max(n // len(SPECIALS), 1)
        used = {n - 7, n - 3, n - 12, n - 15}                               # (the twins and the two faint splats, below)
        for k, label in enumerate(SPECIALS):
            i = (k * step + 1) % n
            while i in used:
                i = (i + 1) % n
            used.add(i)
            at[label] = i
            # (the select rule takes P through the origin round trip; the centres the tests use are the rule's own, so where exactly
            # a seeded splat lands is checked, not assumed: test_marks.py)
            s.P[i] = unproject(cam, xy[label][0], xy[label][1], 2.0 + 0.25 * k).astype(np.float32)
        # two splats at one position, different colours: the lower upload index shows
        a, b = n - 7, n - 3
        s.P[b] = s.P[a] = unproject(cam, w * 0.52, h * 0.47, 1.75).astype(np.float32)
        s.Cd[a] = pkg.scenes.f16bits(np.array([1.0, 0.0, 0.25]))
        s.Cd[b] = pkg.scenes.f16bits(np.array([0.0, 1.0, 0.5]))
        s.alpha[a] = s.alpha[b] = 0.9
        at["twin_lo"], at["twin_hi"] = a, b
        low = np.float32(1.0) / np.float32(255.0)
        at["below_255"], at["zero_opacity"] = n - 12, n - 15
        s.P[n - 12] = unproject(cam, w * 0.25, h * 0.75, 1.5).astype(np.float32)
        s.alpha[n - 12] = np.nextafter(low, np.float32(0.0))
        s.P[n - 15] = unproject(cam, w * 0.75, h * 0.25, 1.5).astype(np.float32)
        s.alpha[n - 15] = 0.0
    else:
        s.P[0] = unproject(cam, w * 0.5, h * 0.5, 2.0).astype(np.float32)
    return Case(f"n{n}_{w}x{h}", s, cam, ORIGIN if seed % 2 else (0.0, 0.0, 0.0), at)


def case(pkg, n, frame_wh):
    key = (n, tuple(frame_wh))
    if key not in _CACHE:
        _CACHE[key] = _make(pkg, n, frame_wh, seed=SIZES.index(n) * 2 + FRAMES.index(tuple(frame_wh)) if n in SIZES else n)
    return _CACHE[key]


def masks(pkg, n, seed):
    """the masks of a cloud of n splats: {label: bool (n,) or None}"""
    last = np.zeros(n, bool)
    last[n - 1] = True
    return {"random": np.random.default_rng(300 + seed).random(n) < 0.6, "null": None, "all_clear": np.zeros(n, bool), "last_bit": last}


def words_with_garbage(pkg, m):
    """packed words of a bool mask with GARBAGE in the bits behind n of the last word (the verb must not look at them)"""
    words = pkg.engine.pack_mask(m)
    if m.size % 32:
        words[-1] |= np.uint32((0xffffffff << (m.size % 32)) & 0xffffffff)
    return words
