"""The case table of the selection tests (gsr_select; include/gsplat_hip.h, "selection"), shared by test_select.py (no GPU) and
test_select_gpu.py.  Everything expected comes from gsr_select_eval -- the rule on the host -- numpy and the oracle, never from the
GPU path.

A case = a cloud, a camera, an origin and a region with all three clauses (rect, image, depth):
  clouds       n in SIZES: 1, 33, 64, 65 (33 and 65: an odd word count), 357 (test_move_gpu's cloud: five clusters of 64 and one of 37),
               GSR_SELECT_BLOCK + 1 (one more than a workgroup's span); random positions in the unit ball, with SEEDED splats spread over
               the upload indices: behind the camera, beyond the far plane, opacity just below 1/255 and exactly 1/255 (both in the middle of
               the rect), opacity 0, a NaN position, infinite positions;
  frames       96 x 64 and 97 x 61: image bits cross word boundaries inside a row;
  projections  perspective, orthographic, off-centre (camera.py), and a non-zero origin.
The image and the depth buffer are built FROM the host-evaluated centres: a random pattern / random depths within the cloud's range,
into which every splat inside the rect forces, by its rank, one outcome at its own pixel -- hit; image bit clear; depth one float
too near -- and every other splat outside the rect is given a set bit and a passing depth, so that every clause has splats that fail
on it alone whatever the seed (test_select.py checks that this came out).  The n = 1 cases cannot hit "more than 0 and fewer than n":
there is one with a hit and one (the splat behind the camera) without."""
import numpy as np

FRAMES = ((96, 64), (97, 61))
OPS = ("REPLACE", "ADD", "SUBTRACT", "INTERSECT", "TOGGLE")
ORIGIN = (1.5, -2.25, 0.75)
_CACHE = {}


class Case:
    def __init__(self, name, splats, cam, origin, rect, image, depth, bias):
        self.name, self.splats, self.cam, self.origin, self.rect = name, splats, cam, tuple(origin), rect
        self.image, self.depth, self.bias = image, depth, float(bias)       # bool (H, W), float32 (H, W): row 0 at the bottom
        self.n = splats.n

    def region(self, pkg, op=0, image=True, depth=True, any_opacity=False, rect="case", **device):
        """(gsr_select_region, keep) of the case: all clauses, or without the image / the depth; rect=None: everywhere"""
        return pkg.engine.select_region(self.rect if rect == "case" else rect, image=self.image if image is True else None,
                                        depth=self.depth if depth is True else None, depth_bias=self.bias, op=op, any_opacity=any_opacity, **device)

    def eval(self, pkg, opacity=None, centres=False, **kw):
        """gsr_select_eval of the case's region (kw: as region takes them) over the cloud; opacity: the RESIDENT one (None: the cloud's)"""
        return pkg.engine.select_eval(self.cam, self.origin, self.region(pkg, **kw), self.splats.P, self.splats.alpha if opacity is None else opacity,
                                      centres=centres)

    def __repr__(self):
        return self.name


def apply_op(op, prior, hit):
    """the numpy restatement of GSR_SELECT_*: prior, hit bool (n,) -> the mask afterwards"""
    return {0: hit, 1: prior | hit, 2: prior & ~hit, 3: prior & hit, 4: prior ^ hit}[int(op)].copy()


def prior_words(pkg, n, seed):
    """a random prior selection of n splats -> (bool (n,), packed words with GARBAGE in the bits behind n of the last word)"""
    prior = np.random.default_rng(seed).random(n) < 0.5
    words = pkg.engine.pack_mask(prior)
    if n % 32:
        words[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    return prior, words


def _camera(pkg, kind, w, h, frame):
    cm = pkg.camera
    near, far = 0.01, 50.0
    if kind == "persp":
        return cm.make_camera(w, h, sh_order=3, frame=frame, near=near, far=far)
    if kind == "ortho":
        a = w / h
        return cm.make_camera(w, h, sh_order=3, frame=frame, proj_matrix=cm.orthographic(-1.25 * a, 1.15 * a, -1.2, 1.2, near, far))
    hw = near / (2.0 * 50.0 / 41.4214)
    hh = hw * h / w
    return cm.make_camera(w, h, sh_order=3, frame=frame, proj_matrix=cm.frustum(-0.8 * hw, 1.2 * hw, -1.1 * hh, 0.9 * hh, near, far))


def _seed_specials(pkg, s, cam, n):
    """the seeded splats, at upload indices spread over the cloud (n >= 33); returns {label: index}"""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    R = V[:3, :3]
    pos = -R.T @ V[:3, 3]
    at = {}
    labels = ("behind", "beyond_far", "below_255", "exactly_255", "zero_opacity", "nan", "inf_x", "neg_inf_z")
    for k, label in enumerate(labels):
        at[label] = (5 * k + 2) % n if n >= 33 else k
    s.P[at["behind"]] = (pos + 1.5 * R[2]).astype(np.float32)
    s.P[at["beyond_far"]] = (pos - 75.0 * R[2]).astype(np.float32)
    low = np.float32(1.0) / np.float32(255.0)
    s.P[at["below_255"]] = (0.02, -0.03, 0.01)
    s.alpha[at["below_255"]] = np.nextafter(low, np.float32(0.0))
    s.P[at["exactly_255"]] = (-0.05, 0.04, 0.0)
    s.alpha[at["exactly_255"]] = low
    s.P[at["zero_opacity"]] = (0.06, 0.05, -0.02)
    s.alpha[at["zero_opacity"]] = 0.0
    s.P[at["nan"]] = (np.nan, 0.1, 0.2)
    s.P[at["inf_x"]] = (np.inf, 0.0, 0.0)
    s.P[at["neg_inf_z"]] = (0.1, 0.2, -np.inf)
    for label in ("behind", "beyond_far", "nan", "inf_x", "neg_inf_z"):
        s.alpha[at[label]] = 0.75
    return at


def _make(pkg, name, n, frame_wh, kind, origin, seed, only_behind=False):
    E = pkg.engine
    w, h = frame_wh
    cam = _camera(pkg, kind, w, h, frame=seed % 7)
    s = pkg.scenes.make_scene(n, seed=seed, sh=True, log_scale_range=(-3.5, -2.0))
    s.alpha[:] = np.maximum(s.alpha, np.float32(0.01))                   # (the random splats pass the opacity test: the seeded ones fail it)
    specials = _seed_specials(pkg, s, cam, n) if n >= 33 else {}
    if n == 1:
        s.P[0] = (0.01, 0.02, -0.01)                                     # (inside the rect: the n1_hit case hits it)
    if only_behind:
        V = np.asarray(cam.view, np.float64).reshape(4, 4).T
        s.P[0] = (-V[:3, :3].T @ V[:3, 3] + 1.5 * V[2, :3]).astype(np.float32)
    rect = (np.float32(w * 0.31), np.float32(h * 0.22), np.float32(w * 0.66), np.float32(h * 0.81))
    # the centres of everything that passes the clip tests, whatever its opacity (the rule on the host, everywhere-rect)
    _, c = E.select_eval(cam, origin, E.select_region(None, any_opacity=True), s.P, s.alpha, centres=True)
    cx, cy, zw = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid="ignore"):
        inframe = (cx >= 0) & (cx < np.float32(w)) & (cy >= 0) & (cy < np.float32(h)) & ~np.isnan(zw)
        inrect = inframe & (rect[0] <= cx) & (cx < rect[2]) & (rect[1] <= cy) & (cy < rect[3])
    rng = np.random.default_rng(1000 + seed)
    image = rng.random((h, w)) < 0.5
    zs = zw[inframe]
    zlo, zhi = (float(zs.min()), float(zs.max())) if zs.size else (0.25, 0.75)
    depth = rng.uniform(zlo, max(zhi, zlo + 1e-6), (h, w)).astype(np.float32)
    bias = np.float32((0.0, 2.0 ** -20, -(2.0 ** -21))[seed % 3])
    qx, qy = np.where(inframe, cx, 0).astype(np.int64), np.where(inframe, cy, 0).astype(np.int64)

    def passing(z):           # a depth the splat passes: its own window depth (bias >= 0) or the next floats above until it does
        d = np.float32(z)
        while not (np.float32(z) <= np.float32(d + bias)):
            d = np.nextafter(d, np.float32(np.inf))
        return d

    def failing(z):           # ... and one it fails: the nearest float below for which the compare is false
        d = np.float32(z)
        while np.float32(z) <= np.float32(d + bias):
            d = np.nextafter(d, np.float32(-np.inf))
        return d

    forced = {}               # pixel -> owner: the first splat to force a pixel keeps it
    opac = {specials.get(k) for k in ("below_255", "exactly_255", "zero_opacity")}
    ranked = [i for i in np.flatnonzero(inrect) if i in opac] + [i for i in np.flatnonzero(inrect) if i not in opac]
    for r, i in enumerate(ranked):
        p = (int(qy[i]), int(qx[i]))
        if p in forced:
            continue
        forced[p] = i
        kind_r = 0 if i in opac else (r % 4)
        if kind_r == 0:
            image[p], depth[p] = True, passing(zw[i])
        elif kind_r == 1:
            image[p], depth[p] = False, passing(zw[i])
        elif kind_r == 2:
            image[p], depth[p] = True, failing(zw[i])
    for r, i in enumerate(np.flatnonzero(inframe & ~inrect)):
        p = (int(qy[i]), int(qx[i]))
        if r % 2 == 0 and p not in forced:
            forced[p] = i
            image[p], depth[p] = True, passing(zw[i])
    case = Case(name, s, cam, origin, rect, image, depth, bias)
    case.specials, case.kind = specials, kind
    return case


def cases(pkg):
    """the table: every size, both frames, every projection, zero and non-zero origins"""
    if "cases" not in _CACHE:
        blk = pkg.engine.SELECT_BLOCK
        zero = (0.0, 0.0, 0.0)
        spec = [("n1_hit", 1, FRAMES[0], "persp", zero, 3, False), ("n1_behind", 1, FRAMES[1], "ortho", ORIGIN, 4, True),
                ("n33_ortho_origin", 33, FRAMES[1], "ortho", ORIGIN, 5, False), ("n64_offcentre", 64, FRAMES[0], "offcentre", zero, 6, False),
                ("n65_persp_origin", 65, FRAMES[1], "persp", ORIGIN, 7, False), ("n357_persp", 357, FRAMES[0], "persp", zero, 11, False),
                ("n357_offcentre_origin", 357, FRAMES[1], "offcentre", (1000.1, -37.5, 12.125), 12, False),
                (f"n{blk + 1}_ortho", blk + 1, FRAMES[0], "ortho", zero, 13, False), (f"n{blk + 1}_persp_origin", blk + 1, FRAMES[1], "persp", ORIGIN, 14, False)]
        _CACHE["cases"] = [_make(pkg, *row) for row in spec]
    return _CACHE["cases"]


def case_names(blk=256):
    return ["n1_hit", "n1_behind", "n33_ortho_origin", "n64_offcentre", "n65_persp_origin", "n357_persp", "n357_offcentre_origin",
            f"n{blk + 1}_ortho", f"n{blk + 1}_persp_origin"]


def case(pkg, name):
    return {c.name: c for c in cases(pkg)}[name]
