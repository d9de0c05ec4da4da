"""Selection by connectivity without a GPU (include/gsplat_hip.h, "selection by connectivity"): gsr_select_connected_eval -- the rule
the kernels evaluate, on the host -- against the breadth-first restatement of connect_cases.py for every case (hits, labels, sizes and
every field of the result), the case table's own conditions (the gap edge, the seams, the snake, the comb, the clumped floaters that no
density rule finds), seeds, size edges, SKIP_HIDDEN, every refusal, the header's constants and structs, and the resources the compiler
gives the kernels.  No tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import connect_cases as CC
import density_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
NAMES = CC.case_names()
NAN, INF = float("nan"), float("inf")
KERNELS = ("k_connect_mark", "k_connect_table", "k_connect_seed", "k_connect_link", "k_connect_flatten", "k_connect_stats",
           "k_connect_scatter", "k_connect_hit")


def _same(got, want, label):
    assert np.array_equal(got[0], want[0]), (label, "hit", np.flatnonzero(got[0] != want[0])[:10])
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), (label, "labels", np.flatnonzero(got[1] != want[1])[:10])
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), (label, "sizes", np.flatnonzero(got[2] != want[2])[:10])
    assert got[3] == want[3], (label, "result", got[3][:6], want[3][:6])


# ---- (a) the eval against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_eval_equals_the_restatement(pkg, name):
    c = CC.case(pkg, name)
    _same(c.eval(pkg), c.restate(), name)
    seed = CC.seed_of(c, 1, 4)
    _same(c.eval(pkg, seed=seed), c.restate(seed=seed), (name, "seeded"))
    hit, lab, siz, (n_pop, n_out, n_cells, n_comp, n_seeded, largest, chist, shist) = c.restate()
    assert sum(chist) == n_comp <= n_cells <= n_pop == sum(shist) and n_pop + n_out <= c.n and int((siz > 0).sum()) == n_pop
    pop = siz > 0
    assert (lab[~pop] == CC.NO_LABEL).all() and (lab[pop] <= np.flatnonzero(pop)).all() and len(set(lab[pop])) == n_comp
    if c.n <= 4097:
        for over in CC.variants():
            _same(c.eval(pkg, **over), c.restate(**over), (name, over))


def test_the_case_table_covers_what_its_header_says(pkg):
    assert NAMES[:2 * len(CC.SIZES)] == [f"n{n}_{t}" for n in CC.SIZES for t in ("sh", "nosh")] and CC.SIZES == DC.SIZES
    assert pkg.engine.SELECT_BLOCK in CC.SIZES and pkg.engine.SELECT_BLOCK + 1 in CC.SIZES and 65537 in CC.SIZES
    for name in NAMES:
        c = CC.case(pkg, name)
        assert c.name == name and (not name.startswith("n") or c.sh == name.endswith("_sh"))
    for name in ("n4097_sh", "n65537_nosh", "n257_sh", "n63_nosh"):      # the sized cases are not vacuous: several components at every reach
        c = CC.case(pkg, name)
        for reach in (0, 1, 2):
            hit, lab, siz, f = c.eval(pkg, reach=reach, size=(2, 40))
            assert f[3] > 1 and 0 < f[1] and f[0] + f[1] < c.n, (name, reach, f[:6])
        assert 0 < c.eval(pkg, reach=1, size=(2, 40))[0].sum() < f[0]
    assert {CC.case(pkg, n).params["reach"] for n in NAMES[:6]} == {0, 1, 2}


# ---- (b) what each special case is there for ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", (0, 1, 2))
def test_gap_edge(pkg, reach):
    """nearest occupied cells `reach` apart: one component; reach + 1 apart: two -- along each axis and the full diagonal"""
    c = CC.case(pkg, f"gap_r{reach}")
    hit, lab, siz, f = c.eval(pkg)
    _same((hit, lab, siz, f), c.restate(), c.name)
    assert len(c.marks) == 8
    for label, (a, b, joined) in c.marks.items():
        if joined:
            assert (siz[a] == 5).all() and (siz[b] == 5).all() and len(set(lab[a]) | set(lab[b])) == 1 and lab[a][0] == min(a.min(), b.min()), label
            assert hit[a].all() and hit[b].all(), label
        else:
            assert (siz[a] == 3).all() and (siz[b] == 2).all() and (lab[a] == a.min()).all() and (lab[b] == b.min()).all(), label
            assert not hit[a].any() and not hit[b].any(), label
    assert f[3] == 4 + 2 * 4 and f[5] == 5


@pytest.mark.parametrize("reach", (1, 2))
def test_seams_are_not_joined(pkg, reach):
    c = CC.case(pkg, f"faces_r{reach}")
    hit, lab, siz, f = c.eval(pkg)
    _same((hit, lab, siz, f), c.restate(), c.name)
    alone = ["x_seam_hi", "x_seam_lo", "x_seam2_hi", "x_seam2_lo", "yz_seam_hi", "yz_seam_lo", "yz_seam2_hi", "yz_seam2_lo", "xyz_seam_hi", "xyz_seam_lo"]
    for label in alone:                                                  # each is a component of its own cell
        at, own = c.marks[label]
        assert (siz[at] == own).all() and (lab[at] == at.min()).all(), (label, siz[at], own)
    a, b = c.marks["pair_a"][0], c.marks["pair_b"][0]                    # true neighbours, for contrast
    assert (siz[a] == 5).all() and (siz[b] == 5).all() and set(lab[a]) == set(lab[b])
    a, b = c.marks["pair2_a"][0], c.marks["pair2_b"][0]                  # two cells apart: joined at reach 2 only
    assert (set(lab[a]) == set(lab[b])) == (reach == 2)
    # the eight corners of the grid: the 2^3 cells of a corner form one component, never joined across the grid
    corner = sum(1 + k % 3 for k, cc in enumerate(__import__("itertools").product((0, 1, 1022, 1023), repeat=3)) if max(cc) <= 1)
    first = np.flatnonzero((c.splats.P < -7.985).all(axis=1))
    assert first.size == 1 and siz[first[0]] == corner
    assert f[3] == 8 + len(alone) + 1 + (1 if reach == 2 else 2)


@pytest.mark.parametrize("reach", (1, 2))
def test_snake(pkg, reach):
    c, cut = CC.case(pkg, f"snake_r{reach}"), CC.case(pkg, f"snake_r{reach}_cut")
    hit, lab, siz, f = c.restate(size=CC.FULL)
    assert c.n == 4097 and f[2:6] == (4097, 1, 0, 4097) and (lab == 0).all() and hit.all(), "the serpentine is one component"
    assert f[2:6] != c.restate(size=CC.FULL, reach=reach - 1)[3][2:6], "at a smaller reach it falls apart: the passes are that tight"
    _same(c.eval(pkg, size=CC.FULL), (hit, lab, siz, f), c.name)
    hit, lab, siz, f = cut.restate()
    path = cut.marks["path"]
    first, second = path[:2048], path[2048:]
    assert cut.n == 4096 and f[3:6] == (2, 0, 2048) and f[6][11] == 2 and f[7][11] == 4096
    assert (lab[first] == first.min()).all() and (lab[second] == second.min()).all() and (siz == 2048).all() and hit.all()
    _same(cut.eval(pkg), (hit, lab, siz, f), cut.name)
    seed = np.zeros(cut.n, bool)
    seed[second[77]] = True
    assert np.array_equal(np.flatnonzero(cut.eval(pkg, seed=seed)[0]), np.sort(second))


def test_comb(pkg):
    c = CC.case(pkg, "comb")
    hit, lab, siz, f = c.eval(pkg)
    _same((hit, lab, siz, f), c.restate(), "comb")
    a, b = c.marks["a"], c.marks["b"]
    assert f[2:6] == (8000, 2, 0, 4000) and (lab[a] == a.min()).all() and (lab[b] == b.min()).all() and (siz == 4000).all()
    assert c.restate(reach=0)[3][3] == 8000


def test_one_cell_and_own_cells(pkg):
    c = CC.case(pkg, "onecell")
    hit, lab, siz, f = c.eval(pkg)
    assert hit.all() and (siz == c.n).all() and (lab == 0).all() and f[:6] == (c.n, 0, 1, 1, 0, c.n) and f[6][16] == 1 and f[7][16] == c.n
    for reach in (0, 1, 2):
        c = CC.case(pkg, f"owncell_r{reach}")
        hit, lab, siz, f = c.eval(pkg)
        assert hit.all() and (siz == 1).all() and np.array_equal(lab, np.arange(c.n)) and f[:6] == (c.n, 0, c.n, c.n, 0, 1) and f[6][0] == c.n
        if reach < 2:
            assert c.restate(reach=reach + 1)[3][3] == 1, "one more cell of reach joins the whole lattice: the stride is the tightest"


def test_clumped_floaters_no_density_rule_finds(pkg):
    """the motivating case: 17 clumps of 5 mutually adjacent floaters.  gsr_select_density's rule, count (1, 3) at reach 1, hits none of
    them (each sees N = 5); size (1, 8) hits exactly the 85"""
    E = pkg.engine
    c = CC.case(pkg, "clumps")
    s, fl = c.splats, c.marks["floater"]
    assert fl.sum() == CC.N_CLUMPS * CC.CLUMP == 85 and c.params["reach"] == 1 and tuple(c.params["size"]) == (1, 8)
    dens, cnt = E.select_density_eval(E.density_rule(c.params["cell"], c.params["origin"], reach=1, count=(1, 3)), s.P, s.alpha, counts=True)
    assert not dens[fl].any() and (cnt[fl] == 5).all(), "the density rule would have found them: the case shows nothing"
    hit, lab, siz, f = c.restate()
    assert np.array_equal(hit, fl) and (siz[fl] == 5).all() and (siz[~fl] == 3000).all() and f[3:6] == (18, 0, 3000) and f[6][2] == 17
    _same(c.eval(pkg), (hit, lab, siz, f), "clumps")
    for k in range(CC.N_CLUMPS):
        members = np.flatnonzero(c.marks["clump_of"] == k)
        assert (lab[members] == members.min()).all()


# ---- (c) seeds and size edges -------------------------------------------------------------------------------------------------------
def test_seeds(pkg):
    E = pkg.engine
    c = CC.case(pkg, "clumps")
    clump_of, fl = c.marks["clump_of"], c.marks["floater"]
    seed = np.zeros(c.n, bool)
    seed[np.flatnonzero(clump_of == 3)[2]] = True
    hit, lab, siz, f = c.eval(pkg, seed=seed, size=CC.FULL)
    assert np.array_equal(hit, clump_of == 3) and f[4] == 1, "one seed bit selects exactly its clump"
    seed[np.flatnonzero(~fl)[5]] = True                                  # seed and size clauses together: the blob is seeded but too large
    assert np.array_equal(c.eval(pkg, seed=seed)[0], clump_of == 3) and c.eval(pkg, seed=seed)[3][4] == 2
    assert np.array_equal(c.eval(pkg, seed=seed, size=CC.FULL)[0], (clump_of == 3) | ~fl)
    assert not c.eval(pkg, seed=np.zeros(c.n, bool))[0].any(), "an empty seed hits nothing"
    # a seed on a splat that is not population seeds nothing: below alpha_min, outside, hidden under SKIP_HIDDEN
    c = CC.case(pkg, "n4097_sh")
    s = c.splats
    hit, lab, siz, f = c.eval(pkg, size=CC.FULL)
    below, outside = np.flatnonzero(s.alpha < np.float32(0.2)), np.flatnonzero((siz == 0) & (s.alpha >= np.float32(0.2)))
    assert below.size > 100 and outside.size > 100
    for label, at in (("below alpha_min", below[:7]), ("outside", outside[:7])):
        seed = np.zeros(c.n, bool)
        seed[at] = True
        got = c.eval(pkg, seed=seed, size=CC.FULL)
        assert not got[0].any() and got[3][4] == 0, label
        assert np.array_equal(c.eval(pkg, seed=seed, size=CC.FULL, flags=CC.HIT_OUTSIDE)[0], (siz == 0) & (s.alpha >= np.float32(0.2))), label
    hide = np.arange(c.n) % 5 == 1
    vis, keep = E.visibility_struct([], hide)
    seed = np.zeros(c.n, bool)
    seed[np.flatnonzero(hide & (siz > 0))[:9]] = True
    assert c.eval(pkg, seed=seed, size=CC.FULL, vis=vis)[0].any(), "without the flag a hidden splat is population and seeds"
    got = c.eval(pkg, seed=seed, size=CC.FULL, vis=vis, flags=CC.SKIP_HIDDEN)
    _same(got, c.restate(seed=seed, size=CC.FULL, hidden=hide, flags=CC.SKIP_HIDDEN), "skip hidden, seeded")
    assert not got[0].any() and got[3][4] == 0
    # seed bits behind n are never looked at
    c = CC.case(pkg, "n65_nosh")
    seed = CC.seed_of(c, 3, 6)
    words = E.pack_mask(seed)
    garbage = words.copy()
    garbage[-1] |= np.uint32(0xffffffff << (c.n % 32) & 0xffffffff)
    assert np.array_equal(E.select_connected_eval(c.rule(pkg), c.splats.P, c.splats.alpha, seed=garbage), c.eval(pkg, seed=seed)[0])


def test_size_edges(pkg):
    c = CC.case(pkg, "clumps")
    fl = c.marks["floater"]
    for lo, hi, want in ((5, 5, fl), (6, 3000, ~fl), (5, 2999, fl), (1, 4, fl & False), (5, 3000, fl | True), (3000, 3000, ~fl), (3001, CC.FULL[1], fl & False),
                         (0, 0, fl & False), (9, 4, fl & False)):
        got = c.eval(pkg, size=(lo, hi))[0]
        assert np.array_equal(got, want), (lo, hi, int(got.sum()))
        assert np.array_equal(got, c.restate(size=(lo, hi))[0]), (lo, hi)
    assert np.array_equal(c.eval(pkg, size=(0x80000000, 0xffffffff))[0], fl & False), "the range is compared as unsigned"
    assert np.array_equal(c.eval(pkg, op=3)[0], c.eval(pkg)[0]), "the eval checks the op and does not apply it"


def test_alpha_edges_and_outside(pkg):
    c = CC.case(pkg, "alpha")
    hit, lab, siz, f = c.eval(pkg)
    s, m = c.splats, c.marks
    with np.errstate(invalid="ignore"):
        pop = s.alpha >= DC.ALPHA_MIN
    assert f[:6] == (int(pop.sum()), 0, 1, 1, 0, int(pop.sum())) and np.array_equal(hit, pop) and (lab[pop] == np.flatnonzero(pop)[0]).all()
    assert hit[m["at_min"]] and hit[m["above_one"]] and not hit[m["ulp_below"]] and not hit[m["nan"]] and not hit[m["negative"]] and not hit[m["minus_zero"]]
    assert c.eval(pkg, alpha_min=-INF)[3][0] == c.n - 1 and c.eval(pkg, alpha_min=0.0)[0][m["minus_zero"]]
    assert pkg.engine.select_connected_eval(c.rule(pkg, alpha_min=1.0), s.P).all(), "no alpha array: every alpha is 1"
    for name in ("bounds", "bounds_hit_outside"):
        c = CC.case(pkg, name)
        hit, lab, siz, f = c.eval(pkg)
        _same((hit, lab, siz, f), c.restate(), name)
        for label, (i, inside, where) in c.marks.items():
            assert (siz[i] > 0) == inside and (lab[i] != CC.NO_LABEL) == inside, label
            if not inside:
                assert hit[i] == (name == "bounds_hit_outside"), label
        seed = np.zeros(c.n, bool)                                       # an outside splat is hit by the flag whatever the clauses
        assert np.array_equal(c.eval(pkg, seed=seed, size=(9, 1))[0], (siz == 0) if name == "bounds_hit_outside" else np.zeros(c.n, bool))


def test_skip_hidden(pkg):
    E = pkg.engine
    c = CC.case(pkg, "n257_sh")
    s = c.splats
    hide = np.arange(c.n) % 5 == 1
    vis, keep = E.visibility_struct([E.crop_box((0.2, 0.0, 0.0), 0.4)], hide)
    visible = E.visibility_eval(vis, s.P)
    assert (~visible).sum() > 20 and visible.sum() > 20
    for reach in (1, 2):
        base = c.eval(pkg, reach=reach)
        _same(c.eval(pkg, reach=reach, vis=vis), base, "a visibility without the flag changes nothing")
        _same(c.eval(pkg, reach=reach, flags=CC.SKIP_HIDDEN), base, "no visibility: nothing is hidden")
        skipped = c.eval(pkg, reach=reach, vis=vis, flags=CC.SKIP_HIDDEN)
        _same(skipped, c.restate(reach=reach, hidden=~visible, flags=CC.SKIP_HIDDEN), "skip hidden")
        assert (skipped[2][~visible] == 0).all() and skipped[3][0] < base[3][0]


# ---- (d) refusals --------------------------------------------------------------------------------------------------------------------------
def _bad_rules(pkg):
    """every field value the library refuses: (label, rule)"""
    E = pkg.engine
    out = []

    def bad(label, **fields):
        r = E.connect_rule(0.125, (0.0, 0.0, 0.0), size=(1, 8))
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
    c = CC.case(pkg, "n65_sh")
    s = c.splats
    hit, lab, siz = np.full(c.n, 9, np.uint8), np.full(c.n, 0xdeadbeef, np.uint32), np.full(c.n, 0xdeadbeef, np.uint32)
    res = E.gsr_connect_result()
    res.n_population = -7

    def call(rule, vis=None, n=c.n, P=s.P.ctypes.data, out=hit.ctypes.data):
        return L.gsr_select_connected_eval(C.byref(rule) if rule is not None else None, C.byref(vis) if vis is not None else None, n, P,
                                           s.alpha.ctypes.data, None, out, lab.ctypes.data, siz.ctypes.data, C.byref(res))

    for label, r in _bad_rules(pkg):
        assert call(r) == GSR_E_INVALID and b"gsr_select_connected_eval" in L.gsr_last_error(), label
    ok = c.rule(pkg, flags=CC.SKIP_HIDDEN)
    assert call(None) == GSR_E_INVALID
    assert call(ok, n=-1) == GSR_E_INVALID and call(ok, n=1 << 31) == GSR_E_INVALID
    assert call(ok, P=None) == GSR_E_INVALID and call(ok, out=None) == GSR_E_INVALID
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)], np.zeros(c.n - 1, bool))
    assert call(ok, vis=vis) == GSR_E_INVALID                                # the visibility's mask does not cover the splats
    assert (hit == 9).all() and (lab == 0xdeadbeef).all() and (siz == 0xdeadbeef).all() and res.n_population == -7, "a refusal wrote something"
    assert call(ok, n=0, P=None, out=None) == 0 and res.fields() == (0,) * 6 + ((0,) * 32,) * 2       # no splats: nothing is read, zeros
    assert L.gsr_select_connected_eval(C.byref(c.rule(pkg, size=(9, 1))), None, c.n, s.P.ctypes.data, None, None, hit.ctypes.data, None, None, None) == 0
    assert not hit.any()


def test_context_refusals_without_a_gpu(pkg):
    L, E = pkg.load_library(), pkg.engine
    r = E.connect_rule(0.125, (0, 0, 0))
    w = np.full(2, 0xdeadbeef, np.uint32)
    cnt = C.c_int64(-7)
    assert L.gsr_select_connected(None, C.byref(r), None, 0, w.ctypes.data, 0, None, None, 0, None, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_multi_select_connected(None, C.byref(r), None, w.ctypes.data, None, None, None, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_get_select_connected(None, None, None, None) == GSR_E_INVALID
    assert L.gsr_debug_select_connected_stages(None, None) == GSR_E_INVALID
    assert cnt.value == -7 and (w == 0xdeadbeef).all()


# ---- (e) the header and the Python door --------------------------------------------------------------------------------------------------
def _struct_names(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n) for n in re.findall(r"(\w+(?:\[\w+\])?)\s*[;,]", body)]


def test_header_constants_structs_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("SKIP_HIDDEN", 1), ("HIT_OUTSIDE", 2), ("CELLS", 1024), ("MAX_REACH", 2), ("HIST_BINS", 32)):
        assert int(re.search(r"#define GSR_CONNECT_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(E, "CONNECT_" + name)
        if name != "HIST_BINS":
            assert getattr(E, "DENSITY_" + name) == value, "the grid, the reach and the flags are the density rule's"
    assert int(re.search(r"#define GSR_CONNECT_NO_LABEL\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == E.CONNECT_NO_LABEL == CC.NO_LABEL
    assert (CC.CELLS, CC.BINS, CC.SKIP_HIDDEN, CC.HIT_OUTSIDE) == (E.CONNECT_CELLS, E.CONNECT_HIST_BINS, E.CONNECT_SKIP_HIDDEN, E.CONNECT_HIT_OUTSIDE)
    assert _struct_names(hdr, "gsr_connect_rule") == [n for n, _ in E.gsr_connect_rule._fields_]
    assert _struct_names(hdr, "gsr_connect_result") == [n for n, _ in E.gsr_connect_result._fields_]
    R, D = E.gsr_connect_rule, E.gsr_density_rule
    assert C.sizeof(R) == 44 == C.sizeof(D) and (R.origin.offset, R.reach.offset, R.flags.offset, R.op.offset, R.reserved_.offset) == (4, 16, 20, 24, 28)
    assert (R.size_lo.offset, R.size_hi.offset, R.alpha_min.offset) == (32, 36, 40) == (D.count_lo.offset, D.count_hi.offset, D.alpha_min.offset)
    S = E.gsr_connect_result
    assert C.sizeof(S) == 8 * 70 and (S.n_population.offset, S.n_outside.offset, S.n_cells.offset, S.n_components.offset, S.n_seeded.offset,
                                      S.largest.offset, S.comp_hist.offset, S.splat_hist.offset) == (0, 8, 16, 24, 32, 40, 48, 304)
    for sym in ("gsr_select_connected", "gsr_select_connected_eval", "gsr_get_select_connected", "gsr_multi_select_connected",
                "gsr_debug_select_connected_stages"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)


def test_connect_rule_builder(pkg):
    E = pkg.engine
    r = E.connect_rule(0.5, (1, 2, 3))
    assert (r.cell, list(r.origin), r.reach, r.flags, r.op, r.reserved_, r.size_lo, r.size_hi) == (0.5, [1, 2, 3], 1, 0, 0, 0, 1, 0xffffffff)
    assert r.alpha_min == -INF
    r = E.connect_rule(0.1, (0, 0, 0), reach=2, size=(1, 7), alpha_min=0.25, flags=3, op=E.SELECT_TOGGLE)
    assert (r.cell, r.reach, r.flags, r.op, r.size_lo, r.size_hi, r.alpha_min) == (np.float32(0.1), 2, 3, 4, 1, 7, 0.25)
    with pytest.raises(E.GsrError):
        E.select_connected_eval(r, np.zeros((3, 3), np.float32), alpha=np.zeros(2, np.float32))
    hit, lab, siz, res = E.select_connected_eval(E.connect_rule(1.0, (0, 0, 0)), np.zeros((0, 3), np.float32), labels=True, sizes=True, result=True)
    assert hit.shape == lab.shape == siz.shape == (0,) and res.fields()[:6] == (0,) * 6 and [h.shape for h in res.hists()] == [(32,), (32,)]
    origin, cell = E.density_grid((0, 0, 0), (1, 1, 1), 0.01)            # the grid is density_grid's
    assert E.select_connected_eval(E.connect_rule(cell, origin, size=(2, 2)), np.float32([[0, 0, 0], [0.005, 0, 0], [1, 1, 1]])).tolist() == [True, True, False]


# ---- (f) from the code object ----------------------------------------------------------------------------------------------------------
def test_kernels_exist_once_and_use_no_scratch():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): each of the eight kernels is there, once,
    and uses no scratch; the key kernel, the sort and the block scan the verb launches are the ones that were there"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for kernel in KERNELS + ("k_density_keys", "k_density_count", "k_remove_scan"):
        mine = {k: v for k, v in rows.items() if re.match(r"_Z%d%s" % (len(kernel), kernel), k)}
        assert len(mine) == 1, (kernel, sorted(mine))
        (name, (vg, sg, lds, scratch)), = mine.items()
        print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0, (kernel, vg, sg, lds, scratch)
    for kernel in ("k_connect_link", "k_connect_flatten", "k_connect_hit"):
        assert rows[[k for k in rows if kernel in k][0]][2] == 0, f"{kernel} uses no LDS"
