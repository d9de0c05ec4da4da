"""The case table of the attribute-selection tests (gsr_select_attrs; include/gsplat_hip.h, "selection by attribute"), shared by
test_select_attrs.py (no GPU) and test_select_attrs_gpu.py.  Everything expected comes from gsr_select_attrs_eval -- the rule on the
host -- and the numpy restatement below (restate), never from the GPU path.

A case = a cloud and a rule with every clause set (RULE: alpha, scale_max, scale_min, anisotropy, colour, and two volumes -- a box and
an inverted ellipsoid):
  clouds   n in SIZES: 1, 33, 64, 65 (odd word counts), GSR_SELECT_BLOCK + 1 (one more than a workgroup's span) and 357, each with
           SH and without.  Every random splat passes each clause, except that with probability FAIL_P per clause it is given a value
           that fails that clause (so splats that fail on one clause alone, and splats that pass all, both occur);
  seeded   splats at upload indices spread over the cloud (n >= 33), each a passing splat with one edge put in: alpha exactly at lo
           and at hi, one float outside each, NaN, +0, -0 and above 1; a NaN scale half, +inf, -inf, +-0 halves, a denormal half,
           negative halves, smin = 0 with smax > 0, all three scales 0, three equal scales (no needle); a NaN Cd half, Cd on the
           lower and on the upper bounds; a position on a face of the box, one inside the inverted ellipsoid, a NaN position.
The bounds are dyadic where a half or a position must land on them exactly.  test_select_attrs.py asserts on the table itself that,
in every case with n >= 33, each clause has a splat that fails on it alone and 0 < hits < n; of the two n = 1 cases one hits and one
does not."""
import numpy as np

OPS = ("REPLACE", "ADD", "SUBTRACT", "INTERSECT", "TOGGLE")
SIZES = (1, 33, 64, 65, 257, 357)
FAIL_P = 0.12
A_LO, A_HI = np.float32(0.125), np.float32(0.875)
SMAX_LO, SMAX_HI = 2.0 ** -7, 2.0 ** -3
SMIN_LO, SMIN_HI = 2.0 ** -9, 2.0 ** -4
ANISO = 6.0
C_LO, C_HI = (0.25, 0.125, 0.375), (0.75, 0.875, 0.625)
BOX = ((0.0, 0.0, 0.0), 0.5)                       # centre, half extent: q = 2 P, exact
ELLIPSOID = ((0.25, 0.25, 0.0), 0.125)             # inverted: a splat inside it fails
CLAUSES = ("alpha", "scale_max", "scale_min", "anisotropy", "colour", "volumes")
_CACHE = {}


def rule_params(pkg, only=None, drop=None):
    """the keyword arguments of engine.attr_rule for the table's rule: every clause, or only those named in `only`, or all but `drop`"""
    E = pkg.engine
    p = {"alpha": (A_LO, A_HI), "scale_max": (SMAX_LO, SMAX_HI), "scale_min": (SMIN_LO, SMIN_HI), "anisotropy": ANISO,
         "colour": (C_LO, C_HI), "volumes": [E.crop_box(*BOX), E.crop_ellipsoid(*ELLIPSOID, invert=True)]}
    if only is not None:
        p = {k: v for k, v in p.items() if k in only}
    if drop is not None:
        p = {k: v for k, v in p.items() if k not in drop}
    return p


def restate(pkg, params, P, alpha, scale, Cd, hidden=None, skip_hidden=False):
    """the numpy restatement of the rule (include/gsplat_hip.h), every comparison in float32; the volumes through gsr_visibility_eval
    -- the visibility's own function, which the rule names -- behind a NaN test of P.  hidden: bool (n,) or None -> bool (n,) hit"""
    E = pkg.engine
    n = P.shape[0]
    hit = np.ones(n, bool)
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        if "alpha" in params:
            lo, hi = (f32(v) for v in params["alpha"])
            hit &= (lo <= alpha) & (alpha <= hi)
        if any(k in params for k in ("scale_max", "scale_min", "anisotropy")):
            s = np.abs(np.ascontiguousarray(scale, np.uint16).view(np.float16).astype(np.float32))
            ok = ~np.isnan(s).any(axis=1)
            smax, smin = np.where(ok, s.max(axis=1), f32(0)), np.where(ok, s.min(axis=1), f32(0))
            if "scale_max" in params:
                lo, hi = (f32(v) for v in params["scale_max"])
                hit &= ok & (lo <= smax) & (smax <= hi)
            if "scale_min" in params:
                lo, hi = (f32(v) for v in params["scale_min"])
                hit &= ok & (lo <= smin) & (smin <= hi)
            if "anisotropy" in params:
                hit &= ok & (smax > f32(0)) & (smax >= f32(params["anisotropy"]) * smin)
        if "colour" in params:
            c = np.ascontiguousarray(Cd, np.uint16).view(np.float16).astype(np.float32)
            lo = np.broadcast_to(np.asarray(params["colour"][0], np.float32), (3,))
            hi = np.broadcast_to(np.asarray(params["colour"][1], np.float32), (3,))
            hit &= ((lo <= c) & (c <= hi)).all(axis=1)
        if params.get("volumes"):
            inside = E.visibility_eval(E.visibility_struct(params["volumes"])[0], P)
            hit &= ~np.isnan(P).any(axis=1) & inside
    if skip_hidden and hidden is not None:
        hit &= ~hidden
    return hit


class Case:
    def __init__(self, name, splats, specials):
        self.name, self.splats, self.specials, self.n = name, splats, specials, splats.n
        self.sh = splats.shx is not None

    def rule(self, pkg, op=0, skip_hidden=False, **sel):
        """gsr_attr_rule of the table's rule (sel: only= / drop= as rule_params takes them)"""
        return pkg.engine.attr_rule(**rule_params(pkg, **sel), op=op, skip_hidden=skip_hidden)

    def eval(self, pkg, cloud=None, **sel):
        """gsr_select_attrs_eval of the rule over the cloud (or another one in read()'s layout)"""
        s = self.splats if cloud is None else cloud
        return pkg.engine.select_attrs_eval(self.rule(pkg, **sel), s.P, s.alpha, s.scale, s.Cd)

    def restate(self, pkg, cloud=None, **sel):
        s = self.splats if cloud is None else cloud
        return restate(pkg, rule_params(pkg, **sel), s.P, s.alpha, s.scale, s.Cd)

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


def _h(v):
    return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def _passing_position(rng):
    """a point inside the box and outside the ellipsoid"""
    c, r = np.asarray(ELLIPSOID[0]), ELLIPSOID[1]
    while True:
        p = rng.uniform(-0.45, 0.45, 3)
        if np.sum(((p - c) / r) ** 2) > 1.5:
            return p


def _row(rng, fail=()):
    """one splat's (P, alpha, scale halves, Cd halves): every clause passes but those named in `fail`"""
    P = _passing_position(rng)
    if "volumes" in fail:
        P = rng.uniform(-0.3, 0.3, 3)
        if rng.random() < 0.5:
            P[rng.integers(3)] = rng.choice((-1.0, 1.0)) * rng.uniform(0.55, 0.9)       # outside the box
        else:
            P = np.asarray(ELLIPSOID[0]) + rng.uniform(-0.05, 0.05, 3)                   # inside the inverted ellipsoid
    a = rng.uniform(0.15, 0.85)
    if "alpha" in fail:
        a = rng.uniform(0.0, 0.1) if rng.random() < 0.5 else rng.uniform(0.9, 1.0)
    cd = [rng.uniform(C_LO[k] + 0.01, C_HI[k] - 0.01) for k in range(3)]
    if "colour" in fail:
        k = rng.integers(3)
        cd[k] = rng.uniform(0.0, C_LO[k] - 0.01) if rng.random() < 0.5 else rng.uniform(C_HI[k] + 0.01, 1.0)
    smax, smin = rng.uniform(0.02, 0.1), None
    if "scale_max" in fail:
        smax = rng.uniform(0.15, 0.5)
    smin = rng.uniform(0.003, min(smax / ANISO * 0.95, 0.06))
    if "scale_min" in fail:
        smin = rng.uniform(0.0003, 0.0015)
    if "anisotropy" in fail:
        smax = rng.uniform(0.02, 0.1) if "scale_max" not in fail else smax
        smin = rng.uniform(smax / ANISO * 1.2, smax * 0.9) if "scale_min" not in fail else smin
    mid = rng.uniform(smin, smax)
    sc = rng.permutation([smax, smin, mid]) * rng.choice((-1.0, 1.0), 3)
    return P, a, sc, cd


SEEDS = ("alpha_at_lo", "alpha_at_hi", "alpha_below_lo", "alpha_above_hi", "alpha_nan", "alpha_pzero", "alpha_nzero", "alpha_above_1",
         "scale_nan", "scale_pinf", "scale_ninf", "scale_signed_zeros", "scale_denormal", "scale_negative", "smin_zero", "scale_all_zero",
         "scale_isotropic",
         "cd_nan", "cd_on_lo", "cd_on_hi", "on_box_face", "in_inverted_ellipsoid", "pos_nan")


def _seed(s, i, label, rng):
    """put the edge `label` into splat i (which passes every clause before)"""
    f32 = np.float32
    nan16, inf16 = np.uint16(0x7e00), np.uint16(0x7c00)
    if label == "alpha_at_lo":
        s.alpha[i] = A_LO
    elif label == "alpha_at_hi":
        s.alpha[i] = A_HI
    elif label == "alpha_below_lo":
        s.alpha[i] = np.nextafter(A_LO, f32(-np.inf))
    elif label == "alpha_above_hi":
        s.alpha[i] = np.nextafter(A_HI, f32(np.inf))
    elif label == "alpha_nan":
        s.alpha[i] = f32(np.nan)
    elif label == "alpha_pzero":
        s.alpha[i] = f32(0.0)
    elif label == "alpha_nzero":
        s.alpha[i] = f32(-0.0)
    elif label == "alpha_above_1":
        s.alpha[i] = f32(1.5)
    elif label == "scale_nan":
        s.scale[i, 1] = nan16
    elif label == "scale_pinf":
        s.scale[i, 0] = inf16
    elif label == "scale_ninf":
        s.scale[i, 2] = inf16 | np.uint16(0x8000)
    elif label == "scale_signed_zeros":
        s.scale[i] = (np.uint16(0x8000), _h(0.05), np.uint16(0))
    elif label == "scale_denormal":
        s.scale[i] = (_h(0.05), np.uint16(0x0001), _h(0.02))
    elif label == "scale_negative":
        s.scale[i] = _h([-0.06, -0.005, -0.03])
    elif label == "smin_zero":
        s.scale[i] = _h([0.0, 0.04, 0.02])
    elif label == "scale_all_zero":
        s.scale[i] = _h([0.0, 0.0, 0.0])
    elif label == "scale_isotropic":
        s.scale[i] = _h([0.03, -0.03, 0.03])
    elif label == "cd_nan":
        s.Cd[i, 2] = nan16
    elif label == "cd_on_lo":
        s.Cd[i] = _h(C_LO)
    elif label == "cd_on_hi":
        s.Cd[i] = _h(C_HI)
    elif label == "on_box_face":
        s.P[i] = (0.5, -0.2, 0.1)
    elif label == "in_inverted_ellipsoid":
        s.P[i] = ELLIPSOID[0]
    elif label == "pos_nan":
        s.P[i] = (0.1, np.nan, 0.0)


def _make(pkg, name, n, sh, seed, single_hit=True):
    s = pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-4.0, -2.5))
    rng = np.random.default_rng(500 + seed)
    for i in range(n):
        fail = () if n == 1 else tuple(c for c in CLAUSES if rng.random() < FAIL_P)
        if n == 1 and not single_hit:
            fail = ("alpha",)
        P, a, sc, cd = _row(rng, fail)
        s.P[i], s.alpha[i], s.scale[i], s.Cd[i] = np.asarray(P, np.float32), np.float32(a), _h(sc), _h(cd)
    specials = {}
    if n >= 33:
        for k, label in enumerate(SEEDS):
            i = (19 * k + 2) % n
            P, a, sc, cd = _row(rng)
            s.P[i], s.alpha[i], s.scale[i], s.Cd[i] = np.asarray(P, np.float32), np.float32(a), _h(sc), _h(cd)
            _seed(s, i, label, rng)
            specials[label] = i
    return Case(name, s, specials)


def case_names(blk=256):
    out = []
    for n in (1, 33, 64, 65, blk + 1, 357):
        out += [f"n{n}_sh", f"n{n}_nosh"]
    return out


def cases(pkg):
    """the table: every size, with SH and without"""
    if "cases" not in _CACHE:
        blk = pkg.engine.SELECT_BLOCK
        table = []
        for k, n in enumerate((1, 33, 64, 65, blk + 1, 357)):
            table.append(_make(pkg, f"n{n}_sh", n, True, 60 + 2 * k, single_hit=True))
            table.append(_make(pkg, f"n{n}_nosh", n, False, 61 + 2 * k, single_hit=False))
        _CACHE["cases"] = table
    return _CACHE["cases"]


def case(pkg, name):
    return {c.name: c for c in cases(pkg)}[name]
