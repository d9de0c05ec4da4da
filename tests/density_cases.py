"""The case table of the density-selection tests (gsr_select_density; include/gsplat_hip.h, "selection by density"), shared by
test_select_density.py (no GPU) and test_select_density_gpu.py.  Everything expected comes from gsr_select_density_eval -- the rule on
the host -- and the numpy restatement below (restate), never from the GPU path.  Nothing here has a tolerance.

restate() shares no code with the library: the cells come from np.float32 arithmetic in the stated order (one subtraction, one
multiplication by inv = float32(1) / float32(cell), a floor, the range test on the float), the counts from np.unique + searchsorted over
the (2 reach + 1)^3 cell offsets with a per-axis bounds test.

A case = a cloud and one rule:
  sizes      n in SIZES (1, 2, 63, 64, 65, 255, 256, 257, 4097, 65537: the last wave owns one mask word, the last workgroup is partial),
             each with SH and without: a random cloud over a grid chosen so that the counts spread over the histogram, some splats
             below the grid's low faces (outside), some below alpha_min; reach 0, 1, 2 by turns; the cell is dyadic with SH and not
             without
  faces      cells with ix, iy, iz in {0, 1, 1022, 1023}, and the seams: (1023, y, z) beside (0, y + 1, z), (x, 1023, z) beside
             (x, 0, z + 1), which must NOT count each other; at reach 1 and 2
  bounds     the edges of the cell rule on each axis: p - origin exactly k cell, -0.0f, a denormal and one ulp below the origin
             (outside), t just below and exactly 1024, 1e30, +-inf, NaN; with and without HIT_OUTSIDE
  onecell    65537 splats in one cell: a run longer than a workgroup, N = n, everything in histogram bin 63
  owncell    every splat in a cell of its own, 6 cells apart at reach 2: N = 1 everywhere
  alpha      alpha exactly at alpha_min, one ulp below, NaN, negative, all in one cell
  floaters   a blob of 3000 splats in a block of 6^3 cells and 17 lone splats at least 4 cells from everything else; reach 1,
             count (1, 3) hits exactly the 17"""
import itertools

import numpy as np

OPS = ("REPLACE", "ADD", "SUBTRACT", "INTERSECT", "TOGGLE")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 65537)
CELLS = 1024
BINS = 64
FULL = (1, 0xffffffff)
N_FLOATERS = 17
_CACHE = {}


def restate(P, alpha, cell, origin, reach=1, count=FULL, alpha_min=-np.inf, hidden=None, skip_hidden=False, hit_outside=False):
    """the numpy restatement of the rule -> (hit bool (n,), N uint32 (n,), (n_population, n_outside, n_cells, count_hist tuple))"""
    f32 = np.float32
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    n = P.shape[0]
    alpha = np.ones(n, f32) if alpha is None else np.ascontiguousarray(alpha, f32).reshape(-1)
    inv = f32(1) / f32(cell)
    with np.errstate(all="ignore"):
        d = P - np.asarray(origin, f32).reshape(1, 3)                   # float32 - float32: rounded once
        t = d * inv                                                       # float32 * float32: rounded once
        f = np.floor(t)
        assert d.dtype == t.dtype == f.dtype == f32
        in_grid = ((f >= f32(0)) & (f < f32(CELLS))).all(axis=1)         # on the floats: a NaN, an infinity or a huge t is outside
        cand = alpha >= f32(alpha_min)                                    # (a NaN alpha: never)
    if skip_hidden and hidden is not None:
        cand = cand & ~np.asarray(hidden, bool)
    pop, outside = cand & in_grid, cand & ~in_grid
    ci = np.where(in_grid[:, None], f, f32(0)).astype(np.int64)[pop]
    key = ci[:, 0] | ci[:, 1] << 10 | ci[:, 2] << 20
    uniq, sizes = np.unique(key, return_counts=True)
    acc = np.zeros(key.shape[0], np.int64)
    if uniq.size:
        for dz, dy, dx in itertools.product(range(-reach, reach + 1), repeat=3):
            x, y, z = ci[:, 0] + dx, ci[:, 1] + dy, ci[:, 2] + dz
            ok = (x >= 0) & (x < CELLS) & (y >= 0) & (y < CELLS) & (z >= 0) & (z < CELLS)      # a cell outside the grid does not exist
            k = np.where(ok, x | y << 10 | z << 20, 0)
            at = np.minimum(np.searchsorted(uniq, k), uniq.size - 1)
            acc += np.where(ok & (uniq[at] == k), sizes[at], 0)
    N = np.zeros(n, np.int64)
    N[pop] = acc
    lo, hi = int(count[0]), int(count[1])
    hit = (pop & (N >= lo) & (N <= hi)) | (outside & bool(hit_outside))
    hist = np.bincount(np.minimum(acc, BINS) - 1, minlength=BINS) if acc.size else np.zeros(BINS, np.int64)
    return hit, N.astype(np.uint32), (int(pop.sum()), int(outside.sum()), int(uniq.size), tuple(int(v) for v in hist))


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


class Case:
    """a cloud and the keyword arguments of engine.density_rule (all but op)"""

    def __init__(self, name, splats, params, marks=None):
        self.name, self.splats, self.params, self.n = name, splats, dict(params), splats.n
        self.marks = marks or {}
        self.sh = splats.shx is not None

    def rule(self, pkg, op=0, **over):
        return pkg.engine.density_rule(**{**self.params, **over}, op=op)

    def eval(self, pkg, cloud=None, vis=None, **over):
        """gsr_select_density_eval of the rule over the cloud (or another one in read()'s layout) -> (hit, counts, result fields)"""
        s = self.splats if cloud is None else cloud
        hit, cnt, res = pkg.engine.select_density_eval(self.rule(pkg, **over), s.P, s.alpha, vis=vis, counts=True, result=True)
        return hit, cnt, res.fields()

    def restate(self, cloud=None, hidden=None, **over):
        s = self.splats if cloud is None else cloud
        return restate(s.P, s.alpha, hidden=hidden, **{**self.params, **over})

    def __repr__(self):
        return self.name


def _scene(pkg, n, seed, sh):
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-4.0, -2.5))


def _centre(origin, cell, idx):
    """float32 positions of the centres of the cells idx (m, 3) of a dyadic grid (exact)"""
    p = np.asarray(origin, np.float64) + (np.asarray(idx, np.float64) + 0.5) * float(cell)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p), "the cell centres are not float32 numbers"
    return p.astype(np.float32)


def _sized(pkg, n, sh, k):
    s = _scene(pkg, n, 300 + k, sh)
    rng = np.random.default_rng(900 + k)
    per_axis = 1 << int(np.ceil(np.log2(max(np.cbrt(4.0 * n), 2.0))))
    cell = np.float32(1.0 / per_axis) if sh else np.float32(1.0 / (1.07 * per_axis))
    s.P[:] = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    s.alpha[:] = rng.uniform(0.05, 1.0, n).astype(np.float32)
    # the low faces cut a slice off the cloud (outside); a fifth of the splats lies below alpha_min
    params = dict(cell=cell, origin=(-0.47, -0.5, -0.44), reach=k % 3, count=(1, 2 + 3 * (k % 3)), alpha_min=0.2)
    return Case(f"n{n}_{'sh' if sh else 'nosh'}", s, params)


def _faces(pkg, reach):
    cell, origin = 2.0 ** -6, (-8.0, -8.0, -8.0)
    edge = (0, 1, 1022, 1023)
    idx, marks = [], {}

    def put(label, cell_idx, copies):
        marks[label] = (len(idx), copies)
        idx.extend([cell_idx] * copies)

    for k, c in enumerate(itertools.product(edge, repeat=3)):
        idx.extend([c] * (1 + k % 3))
    put("x_seam_hi", (1023, 500, 500), 2)          # beside (0, 501, 500) in key order: not neighbours
    put("x_seam_lo", (0, 501, 500), 3)
    put("x_seam2_hi", (1022, 600, 500), 4)         # reach 2: 1022 + 2 would alias into (0, 601, 500)
    put("x_seam2_lo", (0, 601, 500), 5)
    put("yz_seam_hi", (300, 1023, 700), 2)         # beside (300, 0, 701) in key order
    put("yz_seam_lo", (300, 0, 701), 3)
    put("yz_seam2_hi", (300, 1022, 800), 4)
    put("yz_seam2_lo", (300, 1, 801), 5)
    put("xyz_seam_hi", (1023, 1023, 900), 2)       # the last key of a z slab beside the first of the next
    put("xyz_seam_lo", (0, 0, 901), 3)
    put("pair_a", (511, 511, 511), 2)              # true neighbours, for contrast
    put("pair_b", (512, 512, 512), 3)
    put("pair2_a", (400, 400, 400), 2)             # two cells apart: neighbours at reach 2 only
    put("pair2_b", (402, 400, 400), 3)
    idx = np.asarray(idx, np.int64)
    s = _scene(pkg, idx.shape[0], 410 + reach, reach == 1)
    perm = np.random.default_rng(411).permutation(idx.shape[0])
    s.P[perm] = _centre(origin, cell, idx)
    s.alpha[:] = 0.5
    marks = {k: (perm[a:a + m], m) for k, (a, m) in marks.items()}
    return Case(f"faces_r{reach}", s, dict(cell=cell, origin=origin, reach=reach, count=(1, 3)), marks)


BOUNDS_ORIGIN = (0.0, 1.0, -2.0)
BOUNDS_CELL = 0.25


def bounds_values(axis):
    """(label, coordinate, in the grid?, cell index or None) on one axis of the `bounds` case"""
    f32, o = np.float32, np.float32(BOUNDS_ORIGIN[axis])
    top = f32(o + f32(CELLS * BOUNDS_CELL))
    rows = [("at_origin", o, True, 0), ("one_cell", f32(o + f32(0.25)), True, 1), ("seven_cells", f32(o + f32(1.75)), True, 7),
            ("ulp_below_origin", np.nextafter(o, f32(-np.inf)), False, None),
            ("below_1024", np.nextafter(top, f32(-np.inf)), True, 1023), ("at_1024", top, False, None),
            ("huge", f32(1e30), False, None), ("minus_huge", f32(-1e30), False, None), ("pinf", f32(np.inf), False, None),
            ("ninf", f32(-np.inf), False, None), ("nan", f32(np.nan), False, None)]
    if axis == 0:                                  # (only an origin of 0 can leave p - origin = -0.0f, or a denormal)
        rows += [("minus_zero", f32(-0.0), True, 0), ("denormal_below", f32(-1e-45), False, None), ("denormal_above", f32(1e-45), True, 0)]
    return rows


def _bounds(pkg, hit_outside):
    rows = []
    for axis in range(3):
        for label, v, inside, where in bounds_values(axis):
            p = [np.float32(BOUNDS_ORIGIN[c] + (5 + 0.5) * BOUNDS_CELL) for c in range(3)]     # the centre of cell 5 on the other axes
            p[axis] = v
            rows.append((f"{'xyz'[axis]}_{label}", p, inside, where))
    filler = 70 - len(rows)
    s = _scene(pkg, 70, 420, hit_outside)
    rng = np.random.default_rng(421)
    s.P[:] = (np.asarray(BOUNDS_ORIGIN) + rng.uniform(0.0, 3.0, (70, 3))).astype(np.float32)
    s.alpha[:] = 0.5
    at = np.random.default_rng(422).permutation(70)[:len(rows)]
    marks = {}
    for i, (label, p, inside, where) in zip(at, rows):
        s.P[i] = p
        marks[label] = (int(i), inside, where)
    assert filler > 0
    return Case("bounds_hit_outside" if hit_outside else "bounds", s,
                dict(cell=BOUNDS_CELL, origin=BOUNDS_ORIGIN, reach=1, count=(1, 4), hit_outside=hit_outside), marks)


def _onecell(pkg):
    n = 65537
    s = _scene(pkg, n, 430, False)
    s.P[:] = (np.asarray((0.3, -0.2, 0.1)) + np.random.default_rng(431).uniform(0.001, 0.06, (n, 3))).astype(np.float32)
    s.alpha[:] = 0.5
    return Case("onecell", s, dict(cell=2.0 ** -4, origin=(-0.7, -0.7, -0.9), reach=1, count=FULL))


def _owncell(pkg):
    idx = np.asarray(list(itertools.product(range(7), range(7), range(11))), np.int64) * 6 + 3      # 6 cells apart: beyond 2 reach + 1 = 5
    s = _scene(pkg, idx.shape[0], 440, True)
    s.P[np.random.default_rng(441).permutation(idx.shape[0])] = _centre((-1.0, -1.0, -1.0), 2.0 ** -5, idx)
    s.alpha[:] = 0.5
    return Case("owncell", s, dict(cell=2.0 ** -5, origin=(-1.0, -1.0, -1.0), reach=2, count=(1, 1)))


ALPHA_MIN = np.float32(0.3)
ALPHA_EDGES = {"at_min": ALPHA_MIN, "ulp_below": np.nextafter(ALPHA_MIN, np.float32(-np.inf)), "nan": np.float32(np.nan),
               "negative": np.float32(-0.5), "minus_zero": np.float32(-0.0), "above_one": np.float32(1.5)}


def _alpha(pkg):
    n = 67
    s = _scene(pkg, n, 450, False)
    s.P[:] = (np.asarray((0.51, 0.52, 0.53)) + np.random.default_rng(451).uniform(0.0, 0.02, (n, 3))).astype(np.float32)   # one cell
    s.alpha[:] = np.where(np.arange(n) % 3 == 0, 0.2, 0.8).astype(np.float32)
    marks = {}
    for k, (label, v) in enumerate(ALPHA_EDGES.items()):
        s.alpha[5 + 9 * k] = v
        marks[label] = 5 + 9 * k
    return Case("alpha", s, dict(cell=2.0 ** -4, origin=(0.0, 0.0, 0.0), reach=1, count=FULL, alpha_min=float(ALPHA_MIN)), marks)


def _floaters(pkg):
    cell, origin = 2.0 ** -5, (-1.0, -1.0, -1.0)
    rng = np.random.default_rng(461)
    n_blob = 3000
    blob = (np.asarray(origin) + (20 + rng.uniform(0.0, 6.0, (n_blob, 3))) * cell).astype(np.float32)       # cells 20..25 on each axis
    # lone splats on a lattice 5 cells apart, all of it at least 4 cells away from the blob's block
    lattice = [(40 + 5 * a, 10 + 5 * b, 12 + 5 * c) for a in range(3) for b in range(3) for c in range(2)][:N_FLOATERS]
    assert len(lattice) == N_FLOATERS
    lone = _centre(origin, cell, np.asarray(lattice, np.int64))
    n = n_blob + N_FLOATERS
    s = _scene(pkg, n, 460, True)
    where = np.sort(rng.permutation(n)[:N_FLOATERS])
    is_lone = np.zeros(n, bool)
    is_lone[where] = True
    s.P[is_lone], s.P[~is_lone] = lone, blob
    s.alpha[:] = rng.uniform(0.3, 1.0, n).astype(np.float32)
    return Case("floaters", s, dict(cell=cell, origin=origin, reach=1, count=(1, 3)), {"lone": is_lone})


SPECIAL = {"faces_r1": lambda pkg: _faces(pkg, 1), "faces_r2": lambda pkg: _faces(pkg, 2), "bounds": lambda pkg: _bounds(pkg, False),
           "bounds_hit_outside": lambda pkg: _bounds(pkg, True), "onecell": _onecell, "owncell": _owncell, "alpha": _alpha,
           "floaters": _floaters}


def case_names():
    return [f"n{n}_{tag}" for n in SIZES for tag in ("sh", "nosh")] + list(SPECIAL)


def case(pkg, name):
    """one case of the table, built on first use and then kept (the clouds are never changed)"""
    if name not in _CACHE:
        if name in SPECIAL:
            _CACHE[name] = SPECIAL[name](pkg)
        else:
            n, tag = name[1:].split("_")
            _CACHE[name] = _sized(pkg, int(n), tag == "sh", 2 * SIZES.index(int(n)) + (tag == "nosh"))
    return _CACHE[name]


def variants():
    """rule overrides every medium case is also run under: each reach, an empty range, the full range, no alpha floor"""
    return [dict(reach=0), dict(reach=1), dict(reach=2), dict(count=(5, 2)), dict(count=FULL), dict(alpha_min=-np.inf, count=(2, 9)),
            dict(count=(0, 0)), dict(hit_outside=True, count=(3, 2))]
