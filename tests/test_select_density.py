"""Selection by density without a GPU (include/gsplat_hip.h, "selection by density"): gsr_select_density_eval -- the rule the kernels
evaluate, on the host -- against the numpy restatement of density_cases.py for every case (hits, counts and every field of the result),
the case table's own conditions (the seams, the edges of the cell rule, the alpha edges, the floaters), SKIP_HIDDEN with and without
a visibility, every refusal of the rule, density_grid, the header's constants and structs, and the resources the compiler gives the
three kernels.  No tolerance anywhere."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import density_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
NAMES = DC.case_names()
NAN, INF = float("nan"), float("inf")


def _same(got, want, label):
    assert np.array_equal(got[0], want[0]), (label, "hit", np.flatnonzero(got[0] != want[0])[:10])
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), (label, "counts", np.flatnonzero(got[1] != want[1])[:10])
    assert got[2] == want[2], (label, "result", got[2][:3], want[2][:3])


# ---- (a) the eval against the numpy restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_eval_equals_the_restatement(pkg, name):
    c = DC.case(pkg, name)
    _same(c.eval(pkg), c.restate(), name)
    hit, cnt, (n_pop, n_out, n_cells, hist) = c.restate()
    assert sum(hist) == n_pop and n_cells <= n_pop and n_pop + n_out <= c.n and int((cnt > 0).sum()) == n_pop
    if c.n <= 4097:
        for over in DC.variants():
            _same(c.eval(pkg, **over), c.restate(**over), (name, over))


def test_the_case_table_covers_what_its_header_says(pkg):
    assert NAMES[:2 * len(DC.SIZES)] == [f"n{n}_{t}" for n in DC.SIZES for t in ("sh", "nosh")]
    assert pkg.engine.SELECT_BLOCK in DC.SIZES and pkg.engine.SELECT_BLOCK + 1 in DC.SIZES and 65537 in DC.SIZES
    for name in NAMES:
        c = DC.case(pkg, name)
        assert c.name == name and (not name.startswith("n") or c.sh == name.endswith("_sh"))
    for name in ("n4097_sh", "n65537_nosh", "n257_sh"):                  # the sized cases are not vacuous
        c = DC.case(pkg, name)
        hit, cnt, (n_pop, n_out, n_cells, hist) = c.restate(reach=1, count=(1, 2))
        assert 0 < hit.sum() < n_pop < c.n and n_out > 0 and n_pop + n_out < c.n, (name, int(hit.sum()), n_pop, n_out)
        assert sum(1 for v in hist if v) >= 3, (name, hist)
    assert {DC.case(pkg, n).params["reach"] for n in NAMES[:6]} == {0, 1, 2}


# ---- (b) what each special case is there for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", (1, 2))
def test_seams_do_not_count_each_other(pkg, reach):
    c = DC.case(pkg, f"faces_r{reach}")
    _, cnt, (n_pop, n_out, n_cells, _) = c.restate()
    assert n_pop == c.n and n_out == 0 and n_cells == 64 + len(c.marks)
    alone = ["x_seam_hi", "x_seam_lo", "x_seam2_hi", "x_seam2_lo", "yz_seam_hi", "yz_seam_lo", "yz_seam2_hi", "yz_seam2_lo", "xyz_seam_hi", "xyz_seam_lo"]
    for label in alone:                                                  # each sees its own cell only
        at, own = c.marks[label]
        assert (cnt[at] == own).all(), (label, cnt[at], own)
    for label in ("pair_a", "pair_b"):                                   # true neighbours see each other
        assert (cnt[c.marks[label][0]] == 5).all(), label
    for label in ("pair2_a", "pair2_b"):
        at, own = c.marks[label]
        assert (cnt[at] == (5 if reach == 2 else own)).all(), label
    # the corners: a cell of {0, 1, 1022, 1023}^3 sees the 2^3 cells of its own corner, never one across the grid
    got = c.eval(pkg)
    assert np.array_equal(got[1], cnt)
    lo_corner = sum(1 + k % 3 for k, cc in enumerate(itertools.product((0, 1, 1022, 1023), repeat=3)) if max(cc) <= 1)
    P = c.splats.P
    first = np.flatnonzero((P < -7.985).all(axis=1))                     # cell (0, 0, 0): its centre is -8 + 1 / 128
    assert first.size == 1 and cnt[first[0]] == lo_corner


@pytest.mark.parametrize("name", ("bounds", "bounds_hit_outside"))
def test_edges_of_the_cell_rule(pkg, name):
    c = DC.case(pkg, name)
    hit, cnt, (n_pop, n_out, _, _) = c.eval(pkg)
    _same((hit, cnt, c.eval(pkg)[2]), c.restate(), name)
    for label, (i, inside, where) in c.marks.items():
        assert (cnt[i] > 0) == inside, (label, cnt[i])
        if not inside:
            assert hit[i] == (name == "bounds_hit_outside"), label
    assert n_out == sum(1 for (_, inside, _) in c.marks.values() if not inside) and n_pop == c.n - n_out
    # the cell index itself, through a reach-0 rule whose grid is moved so that only that cell's row is counted: compare with a
    # single-splat cloud at the cell's centre
    E = pkg.engine
    for axis in range(3):
        for label, v, inside, where in DC.bounds_values(axis):
            if not inside:
                continue
            p = np.asarray(DC.BOUNDS_ORIGIN, np.float32) + np.float32(5.5 * DC.BOUNDS_CELL)
            q = p.copy()
            p[axis] = v
            q[axis] = np.float32(DC.BOUNDS_ORIGIN[axis] + (where + 0.5) * DC.BOUNDS_CELL)
            pair = np.stack([p, q])
            _, n2 = E.select_density_eval(E.density_rule(DC.BOUNDS_CELL, DC.BOUNDS_ORIGIN, reach=0), pair, counts=True)
            assert list(n2) == [2, 2], (axis, label, list(n2))


def test_one_cell_and_own_cells(pkg):
    c = DC.case(pkg, "onecell")
    hit, cnt, (n_pop, n_out, n_cells, hist) = c.eval(pkg)
    assert hit.all() and (cnt == c.n).all() and (n_pop, n_out, n_cells) == (c.n, 0, 1) and hist == (0,) * 63 + (c.n,)
    c = DC.case(pkg, "owncell")
    hit, cnt, (n_pop, n_out, n_cells, hist) = c.eval(pkg)
    assert hit.all() and (cnt == 1).all() and (n_pop, n_out, n_cells) == (c.n, 0, c.n) and hist == (c.n,) + (0,) * 63


def test_alpha_edges(pkg):
    c = DC.case(pkg, "alpha")
    hit, cnt, (n_pop, n_out, n_cells, _) = c.eval(pkg)
    s = c.splats
    with np.errstate(invalid="ignore"):
        pop = s.alpha >= DC.ALPHA_MIN
    assert n_cells == 1 and n_out == 0 and n_pop == int(pop.sum()) and np.array_equal(hit, pop) and np.array_equal(cnt, np.where(pop, n_pop, 0))
    m = c.marks
    assert hit[m["at_min"]] and hit[m["above_one"]] and not hit[m["ulp_below"]] and not hit[m["nan"]] and not hit[m["negative"]] and not hit[m["minus_zero"]]
    hit, cnt, (n_pop, _, _, _) = c.eval(pkg, alpha_min=-INF)            # no floor: everything but the NaN
    assert n_pop == c.n - 1 and not hit[m["nan"]] and hit[m["negative"]] and cnt[m["nan"]] == 0
    hit, _, (n_pop, _, _, _) = c.eval(pkg, alpha_min=0.0)               # -0.0f >= 0.0f
    assert hit[m["minus_zero"]] and not hit[m["negative"]]
    E = pkg.engine
    assert E.select_density_eval(c.rule(pkg, alpha_min=1.0), s.P).all(), "no alpha array: every alpha is 1"


def test_the_floaters_are_exactly_the_lone_splats(pkg):
    c = DC.case(pkg, "floaters")
    lone = c.marks["lone"]
    assert lone.sum() == DC.N_FLOATERS == 17 and c.params["reach"] == 1 and tuple(c.params["count"]) == (1, 3)
    hit, cnt, (n_pop, n_out, n_cells, hist) = c.restate()
    assert np.array_equal(hit, lone), "the restatement alone must hit exactly the 17"
    assert (cnt[lone] == 1).all() and cnt[~lone].min() >= 4 and hist[0] == 17 and n_out == 0 and n_pop == c.n
    assert np.array_equal(c.eval(pkg)[0], lone)


def test_ranges_and_reach(pkg):
    c = DC.case(pkg, "n4097_sh")
    n_pop = c.restate()[2][0]
    assert not c.eval(pkg, count=(5, 2))[0].any() and not c.eval(pkg, count=(0, 0))[0].any()
    assert c.eval(pkg, count=DC.FULL)[0].sum() == n_pop == c.eval(pkg, count=(0, 0xffffffff))[0].sum()
    n0, n1, n2 = (c.eval(pkg, reach=r)[1].astype(np.int64) for r in (0, 1, 2))
    assert (n0 <= n1).all() and (n1 <= n2).all() and (n0 < n1).any() and (n1 < n2).any()
    assert np.array_equal(c.eval(pkg, reach=1, op=3)[0], c.eval(pkg, reach=1)[0]), "the eval checks the op and does not apply it"


# ---- (c) SKIP_HIDDEN with and without a visibility ---------------------------------------------------------------------------------------
def test_skip_hidden(pkg):
    E = pkg.engine
    c = DC.case(pkg, "n257_sh")
    s = c.splats
    hide = np.arange(c.n) % 5 == 1
    vols = [E.crop_box((0.2, 0.0, 0.0), 0.4)]
    vis, keep = E.visibility_struct(vols, hide)
    visible = E.visibility_eval(vis, s.P)
    assert (~visible).sum() > 20 and visible.sum() > 20
    base = c.eval(pkg)
    _same(c.eval(pkg, vis=vis), base, "a visibility without the flag changes nothing")
    _same(c.eval(pkg, skip_hidden=True), base, "no visibility: nothing is hidden")
    skipped = c.eval(pkg, vis=vis, skip_hidden=True)
    _same(skipped, c.restate(hidden=~visible, skip_hidden=True), "skip hidden")
    assert (skipped[1][~visible] == 0).all() and skipped[2][0] < base[2][0] and (skipped[1] <= base[1]).all() and (skipped[1] < base[1]).any()


# ---- (d) refusals --------------------------------------------------------------------------------------------------------------------------
def _bad_rules(pkg):
    """every field value the library refuses: (label, rule)"""
    E = pkg.engine
    out = []

    def bad(label, **fields):
        r = E.density_rule(0.125, (0.0, 0.0, 0.0), count=(1, 3))
        for k, v in fields.items():
            if k.startswith("origin"):
                r.origin[int(k[-1])] = v
            else:
                setattr(r, k, v)
        out.append((label, r))

    for label, v in (("cell 0", 0.0), ("cell -1", -1.0), ("cell nan", NAN), ("cell inf", INF), ("cell denormal: 1 / cell overflows", 1e-45)):
        bad(label, cell=v)
    for k in range(3):
        bad(f"origin[{k}] nan", **{f"origin{k}": NAN})
        bad(f"origin[{k}] inf", **{f"origin{k}": -INF})
    bad("reach -1", reach=-1)
    bad("reach 3", reach=3)
    bad("flags 4", flags=4)
    bad("flags 1 << 30", flags=1 << 30)
    bad("op 5", op=5)
    bad("op -1", op=-1)
    bad("reserved_ 1", reserved_=1)
    bad("alpha_min nan", alpha_min=NAN)
    return out


def test_eval_refusals_write_nothing(pkg):
    L, E = pkg.load_library(), pkg.engine
    c = DC.case(pkg, "n65_sh")
    s = c.splats
    hit, cnt = np.full(c.n, 9, np.uint8), np.full(c.n, 0xdeadbeef, np.uint32)
    res = E.gsr_density_result()
    res.n_population = -7

    def call(rule, vis=None, n=c.n, P=s.P.ctypes.data, out=hit.ctypes.data):
        return L.gsr_select_density_eval(C.byref(rule) if rule is not None else None, C.byref(vis) if vis is not None else None, n, P,
                                         s.alpha.ctypes.data, out, cnt.ctypes.data, C.byref(res))

    for label, r in _bad_rules(pkg):
        assert call(r) == GSR_E_INVALID and b"gsr_select_density_eval" in L.gsr_last_error(), label
    ok = c.rule(pkg, skip_hidden=True)
    assert call(None) == GSR_E_INVALID
    assert call(ok, n=-1) == GSR_E_INVALID and call(ok, n=1 << 31) == GSR_E_INVALID
    assert call(ok, P=None) == GSR_E_INVALID and call(ok, out=None) == GSR_E_INVALID
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)], np.zeros(c.n - 1, bool))
    assert call(ok, vis=vis) == GSR_E_INVALID                                # the visibility's mask does not cover the splats
    vis.n_volumes = 7
    assert call(ok, vis=vis) == GSR_E_INVALID                                # a visibility gsr_set_visibility would refuse
    assert (hit == 9).all() and (cnt == 0xdeadbeef).all() and res.n_population == -7, "a refusal wrote something"
    assert call(ok, n=0, P=None, out=None) == 0 and res.fields() == (0, 0, 0, (0,) * 64)     # no splats: nothing is read, zeros
    # legal: an empty range, the largest cell whose reciprocal is finite, every pointer but the hits NULL
    assert L.gsr_select_density_eval(C.byref(c.rule(pkg, count=(9, 1))), None, c.n, s.P.ctypes.data, None, hit.ctypes.data, None, None) == 0
    assert not hit.any()


def test_context_refusals_without_a_gpu(pkg):
    L, E = pkg.load_library(), pkg.engine
    r = E.density_rule(0.125, (0, 0, 0))
    w = np.full(2, 0xdeadbeef, np.uint32)
    cnt = C.c_int64(-7)
    assert L.gsr_select_density(None, C.byref(r), w.ctypes.data, 0, None, 0, None, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_multi_select_density(None, C.byref(r), w.ctypes.data, None, None, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_get_select_density(None, None, None, None) == GSR_E_INVALID
    assert cnt.value == -7 and (w == 0xdeadbeef).all()


# ---- (e) the header and the Python door --------------------------------------------------------------------------------------------------
def _struct_names(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n) for n in re.findall(r"(\w+(?:\[\w+\])?)\s*[;,]", body)]


def test_header_constants_structs_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("SKIP_HIDDEN", 1), ("HIT_OUTSIDE", 2), ("CELLS", 1024), ("MAX_REACH", 2), ("HIST_BINS", 64)):
        assert int(re.search(r"#define GSR_DENSITY_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(E, "DENSITY_" + name)
    assert (DC.CELLS, DC.BINS) == (E.DENSITY_CELLS, E.DENSITY_HIST_BINS)
    assert _struct_names(hdr, "gsr_density_rule") == [n for n, _ in E.gsr_density_rule._fields_]
    assert _struct_names(hdr, "gsr_density_result") == [n for n, _ in E.gsr_density_result._fields_]
    R = E.gsr_density_rule
    assert C.sizeof(R) == 44 and (R.origin.offset, R.reach.offset, R.flags.offset, R.op.offset, R.reserved_.offset) == (4, 16, 20, 24, 28)
    assert (R.count_lo.offset, R.count_hi.offset, R.alpha_min.offset) == (32, 36, 40)
    S = E.gsr_density_result
    assert C.sizeof(S) == 8 * 67 and (S.n_population.offset, S.n_outside.offset, S.n_cells.offset, S.count_hist.offset) == (0, 8, 16, 24)
    for sym in ("gsr_select_density", "gsr_select_density_eval", "gsr_get_select_density", "gsr_multi_select_density"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)


def test_density_rule_builder(pkg):
    E = pkg.engine
    r = E.density_rule(0.5, (1, 2, 3))
    assert (r.cell, list(r.origin), r.reach, r.flags, r.op, r.reserved_, r.count_lo, r.count_hi) == (0.5, [1, 2, 3], 1, 0, 0, 0, 1, 0xffffffff)
    assert r.alpha_min == -INF
    r = E.density_rule(0.1, (0, 0, 0), reach=2, count=(1, 7), alpha_min=0.25, op=E.SELECT_TOGGLE, skip_hidden=True, hit_outside=True)
    assert (r.cell, r.reach, r.flags, r.op, r.count_lo, r.count_hi, r.alpha_min) == (np.float32(0.1), 2, 3, 4, 1, 7, 0.25)
    with pytest.raises(E.GsrError):
        E.select_density_eval(r, np.zeros((3, 3), np.float32), alpha=np.zeros(2, np.float32))
    hit, cnt, res = E.select_density_eval(E.density_rule(1.0, (0, 0, 0)), np.zeros((0, 3), np.float32), counts=True, result=True)
    assert hit.shape == cnt.shape == (0,) and res.fields() == (0, 0, 0, (0,) * 64) and res.hist().shape == (64,)


def test_density_grid(pkg):
    E = pkg.engine
    lo, hi = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 2.5, 1.5])
    origin, cell = E.density_grid(lo, hi, 0.125)
    assert origin.dtype == np.float32 and isinstance(cell, np.float32) and cell == np.float32(0.125)
    assert np.array_equal(origin, (lo - 0.125).astype(np.float32)), "the origin is one cell below lo"
    # every corner of the box lies in the grid with a whole cell around it, at any reach 1 rule
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    _, cnt, res = E.select_density_eval(E.density_rule(cell, origin), corners, counts=True, result=True)
    assert res.n_outside == 0 and res.n_population == 8 and (cnt == 1).all()
    t = np.floor((corners - origin) * (np.float32(1) / cell))
    assert t.min() >= 1 and t.max() <= 1022
    # the smallest cell that fits 1022 cells: accepted, and one float32 below it refused with the smallest named
    extent = 4.0
    with pytest.raises(ValueError) as err:
        E.density_grid(lo, hi, extent / 1022 * 0.999)
    named = np.float32(re.search(r"smallest cell that fits is (\S+)", str(err.value)).group(1))
    assert float(named) * 1022 > extent and float(np.nextafter(named, np.float32(0))) * 1022 <= extent
    origin, cell = E.density_grid(lo, hi, named)
    assert cell == named
    with pytest.raises(ValueError):
        E.density_grid(lo, hi, np.nextafter(named, np.float32(0)))
    _, _, res = E.select_density_eval(E.density_rule(cell, origin), corners, counts=True, result=True)
    assert res.n_outside == 0
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            E.density_grid(lo, hi, bad)
    with pytest.raises(ValueError):
        E.density_grid(hi, lo, 0.125)
    with pytest.raises(ValueError):
        E.density_grid((0, 0, NAN), hi, 0.125)
    origin, cell = E.density_grid((1, 1, 1), (1, 1, 1), 0.5)             # a point: any cell fits
    assert np.array_equal(origin, np.float32([0.5, 0.5, 0.5]))


# ---- (f) from the code object ----------------------------------------------------------------------------------------------------------
def test_kernels_exist_once_and_use_no_scratch():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): each of the three kernels is there, once,
    and uses no scratch; the sort the verb launches adds no instantiation (k_radix_* are counted before and after by their tests)"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for kernel in ("k_density_keys", "k_density_count", "k_density_hit"):
        mine = {k: v for k, v in rows.items() if re.match(r"_Z%d%s" % (len(kernel), kernel), k)}
        assert len(mine) == 1, (kernel, sorted(mine))
        (name, (vg, sg, lds, scratch)), = mine.items()
        print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0, (kernel, vg, sg, lds, scratch)
    assert rows[[k for k in rows if "k_density_hit" in k][0]][2] == 0, "k_density_hit is k_select's shape: no LDS"
