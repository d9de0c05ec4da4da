"""Sweeps across every boundary of k_cluster_cull, built on the host in float64: the cases of tests/test_cull_edges.py
(CPU) and tests/test_cull_edges_gpu.py.

A CLUMP is 64 coincident splats: one Morton code, so exactly one cluster of the storage order.  A SWEEP is a row of clumps that steps
from well inside one boundary to well outside it along ONE object-space axis (the one that moves the boundary coordinate most), so that
the nearest steps are exact: one float32 ulp of that coordinate, or 1/64 px on screen where an ulp is less.  Around the crossing the
sweep holds the clump nearest to it and three steps either side; inside, two clumps well in; outside, a ladder far past every margin
of the cull.  Each clump's BOUNDARY COORDINATE is computed in float64 from its float32 position and the frame's float32 matrices, the
way K1 forms it (the flip-Y sandwich included), positive inside:
  screen edges   pixels from the edge (x = 0, x = W, y = 0, y = H of the window, y up)
  near / far     view depth from the plane, in world units: (clz + clw) / |P22 + P32| and (clw - clz) / |P22 - P32|
  band rows      pixels above a band's first tile row / below its last ("row Y up" / "row Y down")
  depth          d0 minus the window depth z / w * 0.5 + 0.5, against a depth buffer that holds d0 everywhere
Where a GSplatOrigin moves positions (fl32(P - o) + o), the sweep also holds the clumps next to the crossing that the round trip moves
from outside to inside, if there are any.

Every scene comes twice: with all its clumps coincident ("point"), and with the same clumps SPREAD wherever their Morton cell leaves the
room (spread_clumps): the probe splat, the clump's first, stays where the coincident clump was and carries the boundary coordinate; the
other 63 lie further outside, in a box that starts at the probe, some SPREAD_PX pixels across (a quarter of the near distance deep at
the planes).  All 64 keep one Morton code, so the clump still fills one cluster -- but that cluster's box is no point, and what the
cull takes over a box (the hull of the eight projected corners, the smallest w and |view z|, the largest z + w and w - z, the smallest
z / w) is put at the edge by a splat on the box's inner face.  The corner clump below is moved out for these scenes, so that a cell
is at least four such boxes wide.

Variants: the five perspective ones (pivot 0; the far pivot with origin 0, = pivot and = -pivot; the object transform) cross every
boundary; the orthographic camera crosses the screen edges and its own near / far planes; the off-centre camera the screen edges only
(its frustum has planes of its own, 0.01 and 1e3, which no sweep here reaches).

helpers.unproject and helpers.world_sigma assume a centred perspective projection at the pivot's distance; these scenes also need the
orthographic and the off-centre camera and clumps next to the near plane, so positions come from the module's own `unproject` (any
projection without shear, through the float32 matrices K1 reads) and scales from px_per_unit at each clump; helpers.make_splats packs
the cloud.

Every scene also holds two FLAGGED clumps that no per-splat rule keeps but the cull must: one off screen whose last splat has a NaN
position (placed at the cloud's largest Morton corner, so that the NaN splat, which sorts last, stays in its cluster) and one behind the
eye whose last splat has an infinite scale.
"""
import functools
import math

import numpy as np

import helpers
from helpers import OBJECT_MATRIX as OBJ

W, H = 160, 96
CLUMP = 64
PIVOT = (3.0e4, -2.0e4, 1.0e4)
NEAR, FAR = 0.05, 6.0
ORTHO = (-1.7, 1.3, -1.0, 1.2)
OFFCENTRE = (-0.003, 0.005, -0.002, 0.0035, 0.01, 1.0e3)
ALPHA_MIN = float(np.nextafter(np.float32(1.0 / 255.0), np.float32(1.0)) if float(np.float32(1.0 / 255.0)) < 1.0 / 255.0
                  else np.float32(1.0 / 255.0))          # the smallest float32 >= 1/255
OPACITIES = (1.0, ALPHA_MIN)        # every clump: its even splats opaque, its odd ones at the opacity clause's edge
SHAPES = {"tiny": (0.05, 0.05), "needle": (6.0, 0.05)}  # (long, short) projected sigma in px: tiny sits at the low-pass floor
CLUMPS = ("point", "spread")        # a scene's clumps: all coincident, or spread over a box wherever their Morton cell allows
SPREAD_PX = 8.0                     # a spread clump's box on screen: this far outward and half of it to either side
SCREEN_EDGES = ("left", "right", "bottom", "top")
PLANES = ("near", "far")

# variant: (pivot, origin, object matrix, projection)
VARIANTS = {
    "pivot 0": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None, "persp"),
    "far, origin 0": (PIVOT, (0.0, 0.0, 0.0), None, "persp"),
    "far, origin pivot": (PIVOT, PIVOT, None, "persp"),
    "far, origin -pivot": (PIVOT, tuple(-v for v in PIVOT), None, "persp"),
    "object": ((0.0, 0.0, 0.0), (0.25, -0.5, 0.125), OBJ, "persp"),
    "offcentre": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None, "offcentre"),
    "ortho": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None, "ortho"),
}
PERSP = ("pivot 0", "far, origin 0", "far, origin pivot", "far, origin -pivot", "object")
# scene kind: (variants, camera with the near / far planes NEAR / FAR)
KINDS = {
    "screen": (tuple(VARIANTS), False),
    "planes": (PERSP + ("ortho",), True),
    "band shard": (PERSP, False),
    "band rows": (PERSP, False),
    "depth": (PERSP, True),
}
# the band modes: (set_row_shard with GSR_OPT_SHARD_LAYOUT 1: shard 1 of 3 owns tile rows [2, 4) of 6; set_row_band: [3, 5), mid-frame)
BANDS = {"band shard": ("shard", (1, 3), (2, 4)), "band rows": ("rows", (3, 2), (3, 5))}

SCREEN_LADDER = 20                 # outside clumps of a screen sweep ...
PLANE_LADDER = 40                  # ... and of a plane sweep (geometric, from 4 ulp to PLANE_REACH)
PLANE_REACH = 0.5                  # world depth units past the plane
SCREEN_REACH = {"tiny": 8.0, "needle": 30.0}     # px past the edge
DEPTH_REACH = 5e-3                 # window depth past d0 (some two world units)


def camera(pkg, variant, kind):
    planes = KINDS[kind][1]
    pivot, _, obj, proj = VARIANTS[variant]
    C = pkg.camera
    near, far = (NEAR, FAR) if planes else (0.01, 1.0e5)
    kw = dict(pivot=pivot, object_matrix=obj, sh_order=0, near=near, far=far)
    if proj == "offcentre":
        kw["proj_matrix"] = C.frustum(*OFFCENTRE)
    elif proj == "ortho":
        kw["proj_matrix"] = C.orthographic(*ORTHO, near, far)
    return C.make_camera(W, H, **kw)


def _mats(cam):
    ov = np.asarray(cam.obj_view, np.float32).astype(np.float64).reshape(4, 4).T
    pr = np.asarray(cam.proj, np.float32).astype(np.float64).reshape(4, 4).T
    return ov, pr


def clip(cam, P):
    """float64 (window x, window y, clz, clw) of object-space points, as K1 forms them from the float32 matrices"""
    ov, pr = _mats(cam)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    tv = P @ ov[:3, :3].T + ov[:3, 3]
    tv[:, 1] = -tv[:, 1]                          # (the flip-Y sandwich)
    cl = tv @ pr[:, :3].T + pr[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = (cl[:, 0] / cl[:, 3] * 0.5 + 0.5) * cam.width
        Y = ((-cl[:, 1]) / cl[:, 3] * 0.5 + 0.5) * cam.height
    return X, Y, cl[:, 2], cl[:, 3]


def boundary_coord(cam, P, boundary):
    """float64, positive inside.  Besides the screen edges and the planes: "row Y up" / "row Y down" = pixels above / below the pixel
    row boundary Y (a band's first / last tile row), "depth D0" = D0 minus the window depth z / w * 0.5 + 0.5"""
    X, Y, z, w = clip(cam, P)
    _, pr = _mats(cam)
    if boundary.startswith("row "):
        _, y, d = boundary.split()
        return Y - float(y) if d == "up" else float(y) - Y
    if boundary.startswith("depth "):
        return float(boundary.split()[1]) - (z / w * 0.5 + 0.5)
    return {"left": X, "right": cam.width - X, "bottom": Y, "top": cam.height - Y,
            "near": (z + w) / abs(pr[2, 2] + pr[3, 2]), "far": (w - z) / abs(pr[2, 2] - pr[3, 2])}[boundary]


def unproject(cam, X, Y, D):
    """the object-space point at window (X, Y) and view depth D (any projection without shear terms)"""
    ov, pr = _mats(cam)
    vz = -D
    w = pr[3, 2] * vz + pr[3, 3]
    nx, ny = 2.0 * X / cam.width - 1.0, 2.0 * Y / cam.height - 1.0
    # ndcx = (p00 vx - p01 vy + p02 vz + p03) / w,  ndcy = -(p10 vx - p11 vy + p12 vz + p13) / w
    A = np.array([[pr[0, 0], -pr[0, 1]], [-pr[1, 0], pr[1, 1]]])
    b = np.array([nx * w - pr[0, 2] * vz - pr[0, 3], ny * w + pr[1, 2] * vz + pr[1, 3]])
    vx, vy = np.linalg.solve(A, b)
    return np.linalg.solve(ov[:3, :3], np.array([vx, vy, vz]) - ov[:3, 3])


def round_trip(P, origin):
    """fl32(P - origin) + origin in float32, what K1 positions (the GSplatOrigin round trip)"""
    P = np.asarray(P, np.float32)
    o = np.asarray(origin, np.float32)
    return (P - o) + o


def _axis(cam, P0, boundary):
    """the object axis that moves the boundary coordinate most, and the coordinate's derivative along it (per world unit)"""
    g = np.zeros(3)
    for a in range(3):
        h = 1e-4 * max(1.0, abs(P0[a]))
        Pp, Pm = P0.copy(), P0.copy()
        Pp[a] += h
        Pm[a] -= h
        g[a] = (boundary_coord(cam, Pp, boundary)[0] - boundary_coord(cam, Pm, boundary)[0]) / (2 * h)
    a = int(np.argmax(np.abs(g)))
    return a, g[a]


def _solve(cam, P0, a, boundary, target):
    """P0 moved along axis a until its boundary coordinate is `target` (float64 bisection)"""
    def f(t):
        P = P0.copy()
        P[a] += t
        return boundary_coord(cam, P, boundary)[0] - target
    lo, hi = -1.0, 1.0
    while f(lo) * f(hi) > 0:
        lo, hi = 2 * lo, 2 * hi
    flo = f(lo)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        fm = f(mid)
        if (fm > 0) == (flo > 0):
            lo, flo = mid, fm
        else:
            hi = mid
    P = P0.copy()
    P[a] += 0.5 * (lo + hi)
    return P


def px_per_unit(cam, P):
    """window pixels per object-space unit at P (largest over the axes, for the x edges' direction)"""
    return max(abs(_axis(cam, np.asarray(P, np.float64), b)[1]) for b in ("left", "bottom"))


class Sweep:
    def __init__(self, boundary, P, coord, kind):
        self.boundary, self.P, self.coord, self.kind = boundary, P, coord, kind     # P float32 [k, 3], coord float64 [k]; kind: per clump


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def build_sweep(cam, origin, boundary, D, reach):
    """one sweep: float32 clump positions ordered from inside to outside"""
    exact = boundary in PLANES or boundary.startswith("depth")     # (no pixel unit: the steps are ulps)
    if boundary in PLANES:
        Xc, Yc = 0.5 * cam.width, 0.5 * cam.height
        D = NEAR if boundary == "near" else FAR
    elif boundary.startswith("row "):
        Xc, Yc = 0.5 * cam.width, float(boundary.split()[1])
    elif boundary.startswith("depth"):
        Xc, Yc = 0.5 * cam.width, 0.5 * cam.height
    else:
        Xc = {"left": 0.0, "right": cam.width, "bottom": 0.5 * cam.width, "top": 0.5 * cam.width}[boundary]
        Yc = {"left": 0.5 * cam.height, "right": 0.5 * cam.height, "bottom": 0.0, "top": cam.height}[boundary]
    P0 = unproject(cam, Xc, Yc, D)
    a, g = _axis(cam, P0, boundary)
    P0 = _solve(cam, P0, a, boundary, 0.0)
    Z = P0.astype(np.float32).astype(np.float64)
    # the step: one ulp of the swept coordinate, or 1/64 px where that is more (planes: always one ulp)
    ulp = _ulp(Z[a])
    step = ulp if exact else max(ulp, (1.0 / 64.0) / abs(g))
    toward_out = -math.copysign(1.0, g)           # moving the coordinate this way lowers the boundary coordinate
    pts, kinds = [], []

    def at(t):
        P = Z.copy()
        P[a] = float(np.float32(Z[a] + toward_out * t))
        return P

    if exact:
        inside = [(0.4 * NEAR if boundary in PLANES else 0.4 * DEPTH_REACH) / abs(g), 64 * step]
        t0, t1 = 4 * step, reach / abs(g)
        ladder = [t0 * (t1 / t0) ** (j / (PLANE_LADDER - 1.0)) for j in range(PLANE_LADDER)]
        for j in range(1, PLANE_LADDER):          # (at least a step apart: no two clumps of a sweep coincide)
            ladder[j] = max(ladder[j], ladder[j - 1] + step)
    else:
        inside = [4.0 / abs(g), 1.0 / abs(g)]
        ladder = [max(step * 4, reach * j / SCREEN_LADDER / abs(g)) for j in range(1, SCREEN_LADDER + 1)]
    for t in inside:
        pts.append(at(-t)); kinds.append("inside")
    for k in range(-3, 4):
        pts.append(at(k * step)); kinds.append("fine")
    for t in ladder:
        pts.append(at(4 * step + t)); kinds.append("ladder")
    # round-trip straddlers: outside by their own position, inside where K1 puts them
    if np.any(np.asarray(origin) != 0):
        cand = [at(k * step) for k in range(-16, 17)]
        raw = boundary_coord(cam, np.array(cand), boundary)
        rt = boundary_coord(cam, round_trip(np.array(cand), origin).astype(np.float64), boundary)
        for k in np.nonzero((raw < 0) & (rt > 0))[0][:2]:
            pts.append(cand[k]); kinds.append("round trip")
    seen, keep = set(), []
    for i, p in enumerate(pts):
        if p.tobytes() not in seen:
            seen.add(p.tobytes())
            keep.append(i)
    P = np.array([pts[i] for i in keep], np.float32)
    kinds = [kinds[i] for i in keep]
    coord = boundary_coord(cam, P.astype(np.float64), boundary)
    o = np.argsort(-coord, kind="stable")
    sw = Sweep(boundary, P[o], coord[o], [kinds[i] for i in o])
    sw.axis, sw.out, sw.grad = a, toward_out, abs(g)      # (the swept object axis, the sign that leads outside, |d coord / d axis|)
    return sw, a


def _needle_quat(axis):
    """(x, y, z, w) taking the local x axis onto object axis `axis`"""
    s = math.sqrt(0.5)
    return [(0.0, 0.0, 0.0, 1.0), (0.0, 0.0, s, s), (0.0, -s, 0.0, s)][axis]


def morton_cells(P32, lo, hi):
    """the storage order's quantisation (10 bits per axis inside the cloud's box [lo, hi]) of float32 positions, restated in float32"""
    flo = lo.astype(np.float32)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    fsc = np.where(ext > 0, 1023.999 / np.where(ext > 0, ext, 1.0), 0.0).astype(np.float32)
    t = (np.asarray(P32, np.float32) - flo) * fsc
    return np.clip(t, np.float32(0), np.float32(1023)).astype(np.uint32), flo, fsc


def _spread_cap(boundary, grad):
    """how far a spread clump's box reaches outward along the swept axis, in object units: SPREAD_PX on screen, a quarter of the near
    distance at the planes, a quarter of the sweep's reach in window depth"""
    if boundary in PLANES:
        return 0.25 * NEAR / grad
    return (0.25 * DEPTH_REACH if boundary.startswith("depth") else SPREAD_PX) / grad


def _px_per_unit_at(cam, P):
    """window pixels per object-space unit at P, from a difference a thousandth of P's clip w wide (px_per_unit's step is relative to
    |P|: too wide next to the near plane of a camera far from the origin)"""
    h = 1e-3 * abs(float(clip(cam, P)[3][0]))
    D = np.vstack([P + h * np.eye(3), P - h * np.eye(3)])
    X, Y, _, _ = clip(cam, D)
    return float(max(np.abs(X[:3] - X[3:]).max(), np.abs(Y[:3] - Y[3:]).max()) / (2 * h))


def spread_clumps(cam, Pc, sweeps, seed):
    """Turn the clumps of the sweeps into SPREAD clumps where their Morton cell leaves the room.  A spread clump keeps its probe splat
    (the clump's first) where the coincident clump was; its other 63 splats lie further OUTSIDE the boundary, in a box that starts at
    the probe along the swept axis (so the probe sits on the box's inner face), reaches min(_spread_cap, what is left of the cell) outward
    and SPREAD_PX / 2 px to either side, and stays 5 % of a cell clear of the cell's faces: one Morton code, so the clump still fills
    exactly one cluster, whose box is no point any more.  A clump whose cell leaves less than a quarter of the cap stays coincident.
    Pc: float32 [64 nc, 3], changed in place; the cloud's box is that of Pc as it comes (the spread splats stay inside it).
    -> bool [nc]"""
    nc = Pc.shape[0] // CLUMP
    lo, hi = Pc.min(axis=0), Pc.max(axis=0)
    is_spread = np.zeros(nc, bool)
    rng = np.random.default_rng(seed)
    for sw in sweeps:
        a, out = sw.axis, sw.out
        cap = _spread_cap(sw.boundary, sw.grad)
        for k, c0 in zip(sw.clumps, sw.coord):
            P = Pc[k * CLUMP].astype(np.float64)
            q, flo, fsc = morton_cells(Pc[k * CLUMP], lo, hi)
            f_lo = flo.astype(np.float64) + (q + 0.05) / fsc.astype(np.float64)
            f_hi = np.where(q < 1023, flo.astype(np.float64) + (q + 0.95) / fsc.astype(np.float64), hi.astype(np.float64))
            room = f_hi[a] - P[a] if out > 0 else P[a] - f_lo[a]
            L = min(room, cap)
            if not (L >= 0.25 * cap and L >= 16 * _ulp(P[a])):
                continue
            h = 0.5 * SPREAD_PX / _px_per_unit_at(cam, P)
            # (sideways the box stops at the cell's faces too, or at the probe where that lies within 5 % of one)
            s_lo, s_hi = np.maximum(np.minimum(f_lo, P), P - h), np.minimum(np.maximum(f_hi, P), P + h)
            m = 256
            u = rng.uniform(0.05, 1.0, m)
            u[0] = 1.0
            C = np.empty((m, 3))
            for ax in range(3):
                C[:, ax] = P[ax] + out * u * L if ax == a else rng.uniform(s_lo[ax], s_hi[ax], m)
            C32 = C.astype(np.float32)
            ok = (morton_cells(C32, lo, hi)[0] == q).all(axis=1) & ((C32[:, a] - Pc[k * CLUMP, a]) * out > 0)
            ok &= boundary_coord(cam, C32.astype(np.float64), sw.boundary) < c0
            C32 = C32[ok]
            if len(C32) < CLUMP - 1:
                continue
            Pc[k * CLUMP + 1:(k + 1) * CLUMP] = C32[:CLUMP - 1]
            is_spread[k] = True
    return is_spread


def enough_spread(sw, spread):
    """what a spread scene asks of each sweep: half its clumps spread or more, three of the seven next to the crossing among them,
    two inside the boundary and three outside"""
    sp = spread[np.array(sw.clumps)]
    fine = np.array([k == "fine" for k in sw.kind])
    return bool(sp.sum() * 2 >= sp.size and (sp & fine).sum() >= 3 and (sp & (sw.coord > 0)).sum() >= 2 and (sp & (sw.coord < 0)).sum() >= 3)


@functools.lru_cache(maxsize=None)
def _scene_cached(pkg, kind, variant, shape, clump):
    return _scene(pkg, kind, variant, shape, clump)


def scene(pkg, kind, variant, shape, clump="point"):
    """-> dict(cam, origin, splats, sweeps, flagged clump indices, number of clumps, d0 / band, spread: bool per clump); clump k = upload
    rows [64 k, 64 k + 64), its probe splat -- the one that carries the sweep's boundary coordinate -- is the first of them"""
    return _scene_cached(pkg, kind, variant, shape, clump)


def boundaries(kind, cam, D):
    if kind == "screen":
        return SCREEN_EDGES, None
    if kind == "planes":
        return PLANES, None
    if kind == "depth":
        d0 = float(np.float32(0.5 + 0.5 * (lambda c: c[2][0] / c[3][0])(clip(cam, unproject(cam, 0.5 * cam.width, 0.5 * cam.height, D)))))
        return (f"depth {d0!r}",), d0
    lo, hi = BANDS[kind][2]
    return (f"row {16 * lo} up", f"row {16 * hi} down"), None


def _reach(boundary, shape, clump):
    if boundary in PLANES:
        return PLANE_REACH
    if boundary.startswith("depth"):
        return DEPTH_REACH
    # (a spread clump's box is an object-space box: on screen its corners reach sideways and in depth, so some of them project
    #  further IN than the probe, by up to about the box's width, and the cull rightly keeps the cluster that much longer)
    return SCREEN_REACH[shape] + (2.0 * SPREAD_PX if clump == "spread" else 0.0)


def _scene(pkg, kind, variant, shape, clump):
    cam = camera(pkg, variant, kind)
    origin = VARIANTS[variant][1]
    pivot = np.asarray(VARIANTS[variant][0], np.float64)
    D = float(cam.meta["distance"])
    sweeps, clumps, sig, quat = [], [], [], []
    long_px, short_px = SHAPES[shape]
    bounds, d0 = boundaries(kind, cam, D)
    for b in bounds:
        sw, axis = build_sweep(cam, origin, b, D, _reach(b, shape, clump))
        first = len(clumps)
        for P in sw.P:
            ppu = px_per_unit(cam, P)
            sg = np.array([long_px, short_px, short_px]) / (math.sqrt(2.0) * ppu)
            clumps.append(P.astype(np.float64))
            sig.append(sg)
            quat.append(_needle_quat(axis))
        sw.clumps = list(range(first, len(clumps)))
        sweeps.append(sw)
    # the flagged clumps: behind the eye (inf scale), and off screen at the largest Morton corner (NaN position)
    ov, _ = _mats(cam)
    eye = np.linalg.solve(ov[:3, :3], -ov[:3, 3])
    back = np.linalg.solve(ov[:3, :3], np.array([0.0, 0.0, 1.0]))
    behind = eye + back / np.linalg.norm(back) * 0.5
    off = 8.0 * max(1.0, float(np.max(np.abs(pivot))) * 1e-3)
    if clump == "spread":           # Morton cells of 4 SPREAD_PX at the pivot's distance or more: most clumps find the room to spread
        off = max(off, 1024.0 * 4.0 * SPREAD_PX / px_per_unit(cam, unproject(cam, 0.5 * cam.width, 0.5 * cam.height, D)))
    flagged = {"inf scale behind the eye": len(clumps), "NaN position off screen": len(clumps) + 1}
    nc = len(clumps) + 2
    inner = np.max(np.array(clumps + [behind]), axis=0)
    # (the clumps next to a crossing share one Morton cell: where that cell leaves them no room, the corner moves out by a few per
    #  cent, which moves every cell face, until each sweep has its spread clumps on both sides of the crossing)
    for attempt in range(64):
        corner = inner + off * (1.0 + 0.037 * attempt)
        Pc = np.repeat(np.array(clumps + [behind, corner]), CLUMP, axis=0).astype(np.float32)
        spread = spread_clumps(cam, Pc, sweeps, nc) if clump == "spread" else np.zeros(nc, bool)
        if clump != "spread" or all(enough_spread(sw, spread) for sw in sweeps):
            break
    for P in (behind, corner):
        clumps.append(P)
        sig.append(np.full(3, 0.05 / (math.sqrt(2.0) * px_per_unit(cam, clumps[0]))))
        quat.append((0.0, 0.0, 0.0, 1.0))
    sigma = np.repeat(np.array(sig), CLUMP, axis=0)
    orient = np.repeat(np.array(quat), CLUMP, axis=0)
    rng = np.random.default_rng(len(clumps))
    s = helpers.make_splats(pkg, Pc, sigma, np.resize(np.array(OPACITIES), nc * CLUMP), rng.uniform(0.1, 0.9, (nc * CLUMP, 3)), orient=orient)
    s.P[flagged["NaN position off screen"] * CLUMP + CLUMP - 1, 1] = np.nan
    s.scale[flagged["inf scale behind the eye"] * CLUMP + CLUMP - 1, 0] = 0x7c00
    return dict(cam=cam, origin=origin, splats=s, sweeps=sweeps, flagged=flagged, clumps=nc, d0=d0, band=BANDS.get(kind), spread=spread)


def all_scenes():
    """(kind, variant, shape, clump) of every scene"""
    return [(kind, v, shape, clump) for kind, (variants, _) in KINDS.items() for v in variants for shape in SHAPES for clump in CLUMPS]


def scene_id(c):
    return "-".join(c).replace(" ", "_").replace(",", "")
