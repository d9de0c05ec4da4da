"""The case table of the connected-selection tests (gsr_select_connected; include/gsplat_hip.h, "selection by connectivity"), shared by
test_select_connected.py (no GPU) and test_select_connected_gpu.py.  Everything expected comes from gsr_select_connected_eval -- the
rule on the host -- and the numpy restatement below (restate), never from the GPU path.  Nothing here has a tolerance.

restate() shares no code with the library: the cells come from np.float32 arithmetic in the stated order, as density_cases.restate
forms them (one subtraction, one multiplication by inv = float32(1) / float32(cell), a floor, the range test on the float); the
components from a plain breadth-first search over a dict of the occupied cells, looking at all (2 reach + 1)^3 - 1 neighbours of a cell
with a per-axis bounds test (no union-find, no forward half, no keys).

A case = a cloud and one rule:
  sizes      n in SIZES (density_cases.SIZES), each with SH and without: a random cloud over a grid in which about one cell in twelve
             is occupied (several components at every reach), some splats below the grid's low faces (outside), some below alpha_min;
             reach 0, 1, 2 by turns
  gap_r*     pairs of blobs whose nearest occupied cells are `reach` cells apart (ONE component) and reach + 1 cells apart (two), along
             x, y, z and the full diagonal
  faces_r*   density_cases' faces cloud: cells with indices in {0, 1, 1022, 1023}, and the seams (1023, y, z) | (0, y + 1, z),
             (x, 1023, z) | (x, 0, z + 1), which are consecutive keys and must NOT be joined
  snake_r*   a one-cell-wide serpentine of 4097 occupied cells, consecutive ones `reach` apart, its passes reach + 1 apart: ONE
             component (the longest parent chains); snake_r*_cut: its middle cell emptied: two, of 2048 each
  comb       a backbone row of 1000 cells with 1000 teeth (alternately up and down), and a second comb 10 cells beside it: two
             components (maximal contention on one root)
  onecell    density_cases' 65537 splats in one cell: one component of n
  owncell_r* every splat in a cell of its own at a stride of reach + 1 cells: n components of 1
  alpha      density_cases' alpha edges, all in one cell
  bounds*    density_cases' edges of the cell rule, with and without HIT_OUTSIDE
  clumps     density_cases' blob of 3000 splats and 17 clumps of 5 mutually adjacent floaters: reach 1, size (1, 8) hits exactly the 85"""
import itertools
from collections import deque

import numpy as np

import density_cases as DC

OPS = DC.OPS
SIZES = DC.SIZES
CELLS = 1024
BINS = 32
FULL = (1, 0xffffffff)
NO_LABEL = 0xffffffff
SKIP_HIDDEN, HIT_OUTSIDE = 1, 2
N_CLUMPS, CLUMP = 17, 5
SNAKE_CELLS = 4097
_CACHE = {}

apply_op = DC.apply_op
prior_words = DC.prior_words


def restate(P, alpha, cell, origin, reach=1, size=FULL, alpha_min=-np.inf, flags=0, hidden=None, seed=None):
    """the numpy restatement of the rule -> (hit bool (n,), labels uint32 (n,), sizes uint32 (n,), the result's fields as
    gsr_connect_result.fields() gives them)"""
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
        in_grid = ((f >= f32(0)) & (f < f32(CELLS))).all(axis=1)
        cand = alpha >= f32(alpha_min)
    if (flags & SKIP_HIDDEN) and hidden is not None:
        cand = cand & ~np.asarray(hidden, bool)
    pop, outside = cand & in_grid, cand & ~in_grid
    seeds = None if seed is None else np.asarray(seed, bool)
    cells = {}
    for i in np.flatnonzero(pop):
        cells.setdefault((int(f[i, 0]), int(f[i, 1]), int(f[i, 2])), []).append(int(i))
    around = [o for o in itertools.product(range(-reach, reach + 1), repeat=3) if o != (0, 0, 0)]
    labels, sizes, seeded = np.full(n, NO_LABEL, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    seen, comp_sizes, n_seeded = set(), [], 0
    for start in cells:
        if start in seen:
            continue
        seen.add(start)
        todo, members = deque([start]), []
        while todo:
            x, y, z = todo.popleft()
            members.extend(cells[(x, y, z)])
            for dx, dy, dz in around:
                q = (x + dx, y + dy, z + dz)
                if min(q) < 0 or max(q) >= CELLS or q in seen or q not in cells:   # a cell outside the grid does not exist
                    continue
                seen.add(q)
                todo.append(q)
        members = np.asarray(members, np.int64)
        labels[members], sizes[members] = members.min(), members.size
        comp_sizes.append(members.size)
        if seeds is not None and seeds[members].any():
            seeded[members] = True
            n_seeded += 1
    lo, hi = int(size[0]), int(size[1])
    hit = pop & (sizes >= lo) & (sizes <= hi)
    if seeds is not None:
        hit &= seeded
    hit |= outside & bool(flags & HIT_OUTSIDE)
    cs = np.asarray(comp_sizes, np.int64)
    bins = np.floor(np.log2(cs)).astype(np.int64) if cs.size else np.zeros(0, np.int64)
    assert ((1 << bins) <= cs).all() and (cs < (2 << bins)).all()
    comp_hist = np.bincount(bins, minlength=BINS)
    splat_hist = np.bincount(bins, weights=cs, minlength=BINS).astype(np.int64)
    fields = (int(pop.sum()), int(outside.sum()), len(cells), int(cs.size), n_seeded, int(cs.max()) if cs.size else 0,
              tuple(int(v) for v in comp_hist), tuple(int(v) for v in splat_hist))
    return hit, labels.astype(np.uint32), sizes.astype(np.uint32), fields


class Case:
    """a cloud and the keyword arguments of engine.connect_rule (all but op)"""

    def __init__(self, name, splats, params, marks=None):
        self.name, self.splats, self.params, self.n = name, splats, dict(params), splats.n
        self.marks = marks or {}
        self.sh = splats.shx is not None

    def rule(self, pkg, op=0, **over):
        return pkg.engine.connect_rule(**{**self.params, **over}, op=op)

    def eval(self, pkg, cloud=None, vis=None, seed=None, **over):
        """gsr_select_connected_eval of the rule over the cloud (or another one in read()'s layout) -> (hit, labels, sizes, fields)"""
        s = self.splats if cloud is None else cloud
        hit, lab, siz, res = pkg.engine.select_connected_eval(self.rule(pkg, **over), s.P, s.alpha, seed=seed, vis=vis, labels=True, sizes=True,
                                                              result=True)
        return hit, lab, siz, res.fields()

    def restate(self, cloud=None, hidden=None, seed=None, **over):
        s = self.splats if cloud is None else cloud
        return restate(s.P, s.alpha, hidden=hidden, seed=seed, **{**self.params, **over})

    def __repr__(self):
        return self.name


def _scene(pkg, n, seed, sh):
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-4.0, -2.5))


_centre = DC._centre
GRID = dict(cell=2.0 ** -6, origin=(-8.0, -8.0, -8.0))      # a dyadic grid whose every cell centre is a float32 number


def _at_cells(pkg, idx, seed, sh, shuffle=True):
    """a cloud with one splat at the centre of each cell of idx (m, 3) of GRID, in a random upload order -> (splats, where: where[k] =
    the upload index of idx[k])"""
    idx = np.asarray(idx, np.int64)
    s = _scene(pkg, idx.shape[0], seed, sh)
    where = np.random.default_rng(seed + 1).permutation(idx.shape[0]) if shuffle else np.arange(idx.shape[0])
    s.P[where] = _centre(GRID["origin"], GRID["cell"], idx)
    s.alpha[:] = 0.5
    return s, where


def _sized(pkg, n, sh, k):
    s = _scene(pkg, n, 500 + k, sh)
    rng = np.random.default_rng(1100 + k)
    per_axis = max(np.cbrt(12.0 * n), 2.0)
    cell = np.float32(2.0 ** -int(np.ceil(np.log2(per_axis)))) if sh else np.float32(1.0 / (1.03 * per_axis))
    s.P[:] = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    s.alpha[:] = rng.uniform(0.05, 1.0, n).astype(np.float32)
    params = dict(cell=cell, origin=(-0.47, -0.5, -0.44), reach=(k + 1) % 3, size=(2, 40), alpha_min=0.2)
    return Case(f"n{n}_{'sh' if sh else 'nosh'}", s, params)


GAP_DIRS = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "diag": (1, 1, 1)}


def _gap(pkg, reach):
    idx, marks = [], {}
    for k, ((axis, d), far) in enumerate(itertools.product(GAP_DIRS.items(), (0, 1))):
        a = np.array((100 + 40 * k, 200 + 30 * (k % 3), 300 + 50 * (k % 2)))
        b = a + (reach + far) * np.array(d)
        marks[f"{axis}_{'apart' if far else 'joined'}"] = (len(idx), 3, 2, not far)
        idx += [tuple(a)] * 3 + [tuple(b)] * 2
    s, where = _at_cells(pkg, idx, 610 + reach, reach == 1)
    marks = {k: (where[at:at + na], where[at + na:at + na + nb], joined) for k, (at, na, nb, joined) in marks.items()}
    return Case(f"gap_r{reach}", s, dict(**GRID, reach=reach, size=(4, 9)), marks)


def _faces(pkg, reach):
    c = DC.case(pkg, f"faces_r{reach}")
    return Case(f"faces_r{reach}", c.splats, dict(cell=c.params["cell"], origin=c.params["origin"], reach=reach, size=(1, 3)), c.marks)


def snake_path(reach, cells=SNAKE_CELLS, run=60):
    """the cells of the serpentine, in path order: passes along x of `run` cells `reach` apart; a turn is one cell that bulges out by one
    in x, `reach` up, and the next pass begins one further up: reach + 1 above the last"""
    path, x, y, step = [], 100, 100, 1
    while len(path) < cells:
        for _ in range(run):
            path.append((x, y, 500))
            x += step * reach
        x -= step * reach
        path.append((x + step, y + reach, 500))
        y += reach + 1
        step = -step
    return path[:cells]


def _snake(pkg, reach, cut):
    path = snake_path(reach)
    if cut:
        del path[SNAKE_CELLS // 2]
    s, where = _at_cells(pkg, path, 620 + reach, reach == 2)
    return Case(f"snake_r{reach}{'_cut' if cut else ''}", s, dict(**GRID, reach=reach, size=(1, 3000)), {"path": where})


COMB_TEETH = 1000


def _comb(pkg):
    idx, marks = [], {}
    for name, z in (("a", 400), ("b", 410)):
        first = len(idx)
        for k in range(COMB_TEETH):
            side = 1 if k % 2 == 0 else -1
            idx += [(10 + k, 500, z)] + [(10 + k, 500 + side * t, z) for t in (1, 2, 3)]
        marks[name] = (first, len(idx))
    s, where = _at_cells(pkg, idx, 630, False)
    marks = {k: where[a:b] for k, (a, b) in marks.items()}
    return Case("comb", s, dict(**GRID, reach=1, size=FULL), marks)


def _onecell(pkg):
    c = DC.case(pkg, "onecell")
    return Case("onecell", c.splats, dict(cell=c.params["cell"], origin=c.params["origin"], reach=1, size=FULL))


def _owncell(pkg, reach):
    idx = np.asarray(list(itertools.product(range(7), range(7), range(11))), np.int64) * (reach + 1) + 3
    s, where = _at_cells(pkg, idx, 640 + reach, True)
    return Case(f"owncell_r{reach}", s, dict(**GRID, reach=reach, size=(1, 1)))


def _alpha(pkg):
    c = DC.case(pkg, "alpha")
    return Case("alpha", c.splats, dict(cell=c.params["cell"], origin=c.params["origin"], reach=1, size=FULL, alpha_min=float(DC.ALPHA_MIN)), c.marks)


def _bounds(pkg, hit_outside):
    c = DC.case(pkg, "bounds_hit_outside" if hit_outside else "bounds")
    return Case(c.name, c.splats, dict(cell=c.params["cell"], origin=c.params["origin"], reach=1, size=(1, 4), flags=HIT_OUTSIDE if hit_outside else 0), c.marks)


def _clumps(pkg):
    """density_cases' blob (cells 20..25 of a grid of 2^-5 cells) and 17 clumps: 5 splats in 5 different cells of a 2 x 2 x 2 block
    (mutually adjacent at reach 1), the blocks 6 cells apart and at least 9 cells from the blob"""
    cell, origin = 2.0 ** -5, (-1.0, -1.0, -1.0)
    rng = np.random.default_rng(661)
    n_blob = 3000
    blob = (np.asarray(origin) + (20 + rng.uniform(0.0, 6.0, (n_blob, 3))) * cell).astype(np.float32)
    corners = [(40 + 6 * a, 10 + 6 * b, 12 + 6 * c) for a in range(3) for b in range(3) for c in range(2)][:N_CLUMPS]
    block = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
    idx = np.asarray([(x + dx, y + dy, z + dz) for (x, y, z) in corners for (dx, dy, dz) in block], np.int64)
    floaters = _centre(origin, cell, idx)
    n = n_blob + N_CLUMPS * CLUMP
    s = _scene(pkg, n, 660, True)
    where = rng.permutation(n)[:N_CLUMPS * CLUMP]
    is_floater = np.zeros(n, bool)
    is_floater[where] = True
    s.P[where], s.P[~is_floater] = floaters, blob
    s.alpha[:] = rng.uniform(0.3, 1.0, n).astype(np.float32)
    clump_of = np.full(n, -1, np.int64)
    clump_of[where] = np.arange(N_CLUMPS * CLUMP) // CLUMP
    return Case("clumps", s, dict(cell=cell, origin=origin, reach=1, size=(1, 8)), {"floater": is_floater, "clump_of": clump_of})


SPECIAL = {"gap_r0": lambda pkg: _gap(pkg, 0), "gap_r1": lambda pkg: _gap(pkg, 1), "gap_r2": lambda pkg: _gap(pkg, 2),
           "faces_r1": lambda pkg: _faces(pkg, 1), "faces_r2": lambda pkg: _faces(pkg, 2),
           "snake_r1": lambda pkg: _snake(pkg, 1, False), "snake_r1_cut": lambda pkg: _snake(pkg, 1, True),
           "snake_r2": lambda pkg: _snake(pkg, 2, False), "snake_r2_cut": lambda pkg: _snake(pkg, 2, True),
           "comb": _comb, "onecell": _onecell, "owncell_r0": lambda pkg: _owncell(pkg, 0), "owncell_r1": lambda pkg: _owncell(pkg, 1),
           "owncell_r2": lambda pkg: _owncell(pkg, 2), "alpha": _alpha, "bounds": lambda pkg: _bounds(pkg, False),
           "bounds_hit_outside": lambda pkg: _bounds(pkg, True), "clumps": _clumps}


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
    """rule overrides every medium case is also run under: each reach, an empty range, the full range, no alpha floor, HIT_OUTSIDE"""
    return [dict(reach=0), dict(reach=1), dict(reach=2), dict(size=(5, 2)), dict(size=FULL), dict(alpha_min=-np.inf, size=(2, 9)),
            dict(size=(0, 0)), dict(flags=HIT_OUTSIDE, size=(3, 2))]


def seed_of(c, k, count=3):
    """a reproducible random seed selection of case c: `count` splats (any class) -> bool (n,)"""
    seed = np.zeros(c.n, bool)
    seed[np.random.default_rng(7000 + k).permutation(c.n)[:min(count, c.n)]] = True
    return seed
