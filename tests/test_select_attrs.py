"""Selection by attribute without a GPU (include/gsplat_hip.h, "selection by attribute"): gsr_select_attrs_eval -- the rule the kernel
evaluates, on the host -- against the numpy restatement of attr_select_cases.py for every clause alone and all together, the case
table's own conditions, empty and NaN bounds, SKIP_HIDDEN with and without a visibility, every refusal of the rule, the header's
constants and struct, and the resources the compiler gives k_select_attrs.  No tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import attr_select_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
NAMES = AC.case_names()
NAN, INF = float("nan"), float("inf")


def test_the_case_table_covers_what_its_header_says(pkg):
    cs = AC.cases(pkg)
    assert [c.name for c in cs] == AC.case_names(pkg.engine.SELECT_BLOCK) == NAMES
    assert {c.n for c in cs} == set(AC.SIZES) and pkg.engine.SELECT_BLOCK + 1 in AC.SIZES
    for n in AC.SIZES:
        assert {c.sh for c in cs if c.n == n} == {True, False}
    for c in cs:
        if c.n >= 33:
            assert sorted(c.specials) == sorted(AC.SEEDS) and len(set(c.specials.values())) == len(AC.SEEDS)


# ---- (a) the eval against the numpy restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_eval_equals_the_restatement(pkg, name):
    c = AC.case(pkg, name)
    for only in [(k,) for k in AC.CLAUSES] + [AC.CLAUSES, ()]:
        got, want = c.eval(pkg, only=only), c.restate(pkg, only=only)
        assert np.array_equal(got, want), (name, only, np.flatnonzero(got != want)[:10])
    assert c.eval(pkg, only=()).all(), "no clause set: every splat is hit"


# ---- (b) the case table is not vacuous -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cases_are_not_vacuous(pkg, name):
    c = AC.case(pkg, name)
    full = c.eval(pkg)
    if c.n == 1:
        assert bool(full[0]) == name.endswith("_sh")
        return
    assert 0 < full.sum() < c.n, (name, int(full.sum()))
    for clause in AC.CLAUSES:
        alone = c.eval(pkg, drop=(clause,)) & ~full
        assert alone.any(), f"{name}: no splat fails on the {clause} clause alone"
    at, alone = c.specials, {k: c.eval(pkg, drop=(k,)) & ~full for k in AC.CLAUSES}
    for label in ("alpha_at_lo", "alpha_at_hi", "scale_negative", "cd_on_lo", "cd_on_hi", "on_box_face"):
        assert full[at[label]], (name, label)
    for label in ("alpha_below_lo", "alpha_above_hi", "alpha_nan", "alpha_pzero", "alpha_nzero", "alpha_above_1"):
        assert alone["alpha"][at[label]], (name, label)
    for label in ("scale_pinf", "scale_ninf"):
        assert alone["scale_max"][at[label]], (name, label)
    for label in ("scale_signed_zeros", "scale_denormal", "smin_zero"):
        assert alone["scale_min"][at[label]], (name, label)
    assert alone["anisotropy"][at["scale_isotropic"]], name
    assert alone["colour"][at["cd_nan"]] and alone["volumes"][at["in_inverted_ellipsoid"]] and alone["volumes"][at["pos_nan"]], name
    for label in ("scale_nan", "scale_all_zero"):
        assert not full[at[label]] and c.eval(pkg, drop=("scale_max", "scale_min", "anisotropy"))[at[label]], (name, label)


# ---- (c) empty and NaN bounds, no clause -----------------------------------------------------------------------------------------------
def test_empty_and_nan_bounds_hit_nothing(pkg):
    E = pkg.engine
    c = AC.case(pkg, "n357_sh")
    s = c.splats
    ev = lambda **kw: E.select_attrs_eval(E.attr_rule(**kw), s.P, s.alpha, s.scale, s.Cd)
    assert ev().all() and ev(alpha=(-INF, INF)).sum() == c.n - 1            # (only the NaN alpha is not in [-inf, inf])
    for kw in ({"alpha": (0.6, 0.4)}, {"alpha": (NAN, 1.0)}, {"alpha": (0.0, NAN)}, {"scale_max": (0.2, 0.1)}, {"scale_max": (NAN, INF)},
               {"scale_min": (INF, 0.0)}, {"scale_min": (0.0, NAN)}, {"anisotropy": NAN}, {"colour": ((0.0, 0.0, 0.9), (1.0, 1.0, 0.1))},
               {"colour": ((0.0, NAN, 0.0), (1.0, 1.0, 1.0))}, {"colour": (0.0, (1.0, 1.0, NAN))}):
        assert not ev(**kw).any(), kw
    # infinite bounds are allowed: they pass everything but NaN
    assert np.array_equal(ev(scale_max=(-INF, INF)), ev(scale_min=(0.0, INF))) and ev(scale_max=(-INF, INF)).sum() == c.n - 1
    # anisotropy: 0 passes every splat with smax > 0; infinity only where smin is 0 and smax finite... or inf * 0 = NaN: no hit
    sh = np.abs(s.scale.view(np.float16).astype(np.float32))
    assert np.array_equal(ev(anisotropy=0.0), ~np.isnan(sh).any(axis=1) & (sh.max(axis=1) > 0))
    assert not ev(anisotropy=INF)[c.specials["smin_zero"]]                   # (inf * 0 is NaN)


# ---- (d) SKIP_HIDDEN with and without a visibility ---------------------------------------------------------------------------------------
def test_skip_hidden(pkg):
    E = pkg.engine
    c = AC.case(pkg, "n257_nosh")
    s = c.splats
    hide = np.arange(c.n) % 5 == 1
    vols = [E.crop_box((0.2, 0.0, 0.0), 0.4)]
    vis, keep = E.visibility_struct(vols, hide)
    visible = E.visibility_eval(vis, s.P)
    assert (~visible).sum() > 20 and visible.sum() > 20
    for only in [("alpha",), AC.CLAUSES, ()]:
        base = E.select_attrs_eval(c.rule(pkg, only=only), s.P, s.alpha, s.scale, s.Cd)
        # without the flag a visibility changes nothing; with it the hidden splats drop out; with no visibility nothing is hidden
        assert np.array_equal(E.select_attrs_eval(c.rule(pkg, only=only), s.P, s.alpha, s.scale, s.Cd, vis=vis), base)
        assert np.array_equal(E.select_attrs_eval(c.rule(pkg, only=only, skip_hidden=True), s.P, s.alpha, s.scale, s.Cd, vis=vis), base & visible)
        assert np.array_equal(E.select_attrs_eval(c.rule(pkg, only=only, skip_hidden=True), s.P, s.alpha, s.scale, s.Cd), base)
        want = AC.restate(pkg, AC.rule_params(pkg, only=only), s.P, s.alpha, s.scale, s.Cd, hidden=~visible, skip_hidden=True)
        assert np.array_equal(want, base & visible)
    # a mask alone needs no positions
    vm, keep2 = E.visibility_struct((), hide)
    assert np.array_equal(E.select_attrs_eval(E.attr_rule(alpha=(0.0, 1.0), skip_hidden=True), alpha=s.alpha, vis=vm),
                          (s.alpha >= 0) & (s.alpha <= 1) & ~hide)


# ---- (e) refusals --------------------------------------------------------------------------------------------------------------------------
def _bad_rules(pkg):
    """every field value the library refuses: (label, rule)"""
    E = pkg.engine
    out = []

    def bad(label, **fields):
        r = E.attr_rule(alpha=(0.1, 0.9))
        for k, v in fields.items():
            setattr(r, k, v)
        out.append((label, r))

    bad("clause bit 64", clauses=1 | 64)
    bad("clause bit 1 << 30", clauses=1 << 30)
    bad("flags 2", flags=2)
    bad("reserved_ 1", reserved_=1)
    bad("op 5", op=5)
    bad("op -1", op=-1)
    bad("n_volumes 1 without VOLUME", n_volumes=1)
    for nv in (0, 5, -1):
        r = E.attr_rule(volumes=[E.crop_box((0, 0, 0), 1.0)])
        r.n_volumes = nv
        out.append((f"n_volumes {nv} with VOLUME", r))
    for k, v in (("kind", 0), ("kind", 3), ("invert", 2), ("invert", -1)):
        r = E.attr_rule(volumes=[E.crop_box((0, 0, 0), 1.0), E.crop_ellipsoid((0, 0, 0), 1.0)])
        setattr(r.volume[1], k, v)
        out.append((f"volume 1 {k} {v}", r))
    return out


def test_eval_refusals_write_nothing(pkg):
    L, E = pkg.load_library(), pkg.engine
    c = AC.case(pkg, "n33_sh")
    s = c.splats
    hit = np.full(c.n, 9, np.uint8)
    arrs = [s.P.ctypes.data, s.alpha.ctypes.data, s.scale.ctypes.data, s.Cd.ctypes.data]

    def call(rule, vis=None, n=c.n, a=arrs, out=hit.ctypes.data):
        return L.gsr_select_attrs_eval(C.byref(rule) if rule is not None else None, C.byref(vis) if vis is not None else None, n, *a, out)

    for label, r in _bad_rules(pkg):
        assert call(r) == GSR_E_INVALID and b"gsr_select_attrs_eval" in L.gsr_last_error(), label
    full = c.rule(pkg, skip_hidden=True)
    assert call(None) == GSR_E_INVALID
    assert call(full, n=-1) == GSR_E_INVALID
    assert call(full, out=None) == GSR_E_INVALID
    for k, name in enumerate(("P", "alpha", "scale", "Cd")):                 # an array a set clause needs
        a = list(arrs)
        a[k] = None
        assert call(full, a=a) == GSR_E_INVALID, name
        only = {"P": ("volumes",), "alpha": ("alpha",), "scale": ("scale_min",), "Cd": ("colour",)}[name]
        assert call(c.rule(pkg, only=only), a=a) == GSR_E_INVALID, name
        spare = np.zeros(c.n, np.uint8)
        assert call(c.rule(pkg, drop=only + (("scale_max", "anisotropy") if name == "scale" else ())), a=a, out=spare.ctypes.data) == 0, name
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)], np.zeros(c.n - 1, bool))
    assert call(full, vis=vis) == GSR_E_INVALID                              # the visibility's mask does not cover the splats
    vis.n_volumes = 7
    assert call(full, vis=vis) == GSR_E_INVALID                              # a visibility gsr_set_visibility would refuse
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)])
    a = list(arrs)
    a[0] = None
    assert call(c.rule(pkg, only=("alpha",), skip_hidden=True), vis=vis, a=a) == GSR_E_INVALID     # SKIP_HIDDEN by volumes needs P
    assert (hit == 9).all(), "a refusal wrote something"
    assert call(full, n=0, a=[None] * 4, out=None) == 0                      # no splats: nothing is read


def test_context_refusals_without_a_gpu(pkg):
    L, E = pkg.load_library(), pkg.engine
    r = E.attr_rule(alpha=(0.1, 0.9))
    w = np.full(2, 0xdeadbeef, np.uint32)
    cnt = C.c_int64(-7)
    assert L.gsr_select_attrs(None, C.byref(r), w.ctypes.data, 0, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_multi_select_attrs(None, C.byref(r), w.ctypes.data, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_get_select_attrs(None, None, None, None) == GSR_E_INVALID
    assert cnt.value == -7 and (w == 0xdeadbeef).all()


# ---- (f) the header and the Python door --------------------------------------------------------------------------------------------------
def test_header_constants_struct_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("ALPHA", 1), ("SCALE_MAX", 2), ("SCALE_MIN", 4), ("ANISOTROPY", 8), ("COLOUR", 16), ("VOLUME", 32), ("SKIP_HIDDEN", 1)):
        assert int(re.search(r"#define GSR_ATTR_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(E, "ATTR_" + name)
    body = hdr[hdr.index("typedef struct gsr_attr_rule {"):hdr.index("} gsr_attr_rule;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", n) for n in re.findall(r"(\w+(?:\[\w+\])?)\s*[;,]", body)]
    assert names == [n for n, _ in E.gsr_attr_rule._fields_], names
    assert C.sizeof(E.gsr_attr_rule) == 296 and E.gsr_attr_rule.alpha_lo.offset == 16 and E.gsr_attr_rule.colour_lo.offset == 44
    assert E.gsr_attr_rule.reserved_.offset == 68 and E.gsr_attr_rule.volume.offset == 72
    for sym in ("gsr_select_attrs", "gsr_select_attrs_eval", "gsr_get_select_attrs", "gsr_multi_select_attrs"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)


def test_attr_rule_builder(pkg):
    E = pkg.engine
    r = E.attr_rule()
    assert (r.clauses, r.flags, r.op, r.n_volumes, r.reserved_) == (0, 0, 0, 0, 0)
    box = E.crop_box((0.5, 0, 0), 0.25, invert=True)
    r = E.attr_rule(alpha=(0.1, 0.2), scale_max=(1, 2), scale_min=(3, 4), anisotropy=5, colour=(0.25, (0.5, 0.75, 1.0)), volumes=[box],
                    op=E.SELECT_TOGGLE, skip_hidden=True)
    assert r.clauses == 63 and r.flags == E.ATTR_SKIP_HIDDEN and r.op == 4 and r.n_volumes == 1
    assert (r.alpha_lo, r.alpha_hi, r.scale_max_lo, r.scale_max_hi, r.scale_min_lo, r.scale_min_hi, r.anisotropy) == \
        (np.float32(0.1), np.float32(0.2), 1, 2, 3, 4, 5)
    assert list(r.colour_lo) == [0.25] * 3 and list(r.colour_hi) == [0.5, 0.75, 1.0]
    assert (r.volume[0].kind, r.volume[0].invert) == (E.VOL_BOX, 1) and np.array_equal(np.asarray(r.volume[0].to_unit, np.float32), box[2])
    with pytest.raises(E.GsrError):
        E.select_attrs_eval(E.attr_rule(alpha=(0, 1)), alpha=np.zeros(3, np.float32), P=np.zeros((2, 3), np.float32))


# ---- (g) from the code object ----------------------------------------------------------------------------------------------------------
def test_kernel_exists_and_uses_no_scratch_or_lds():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): k_select_attrs is there, once, and uses
    neither scratch nor LDS"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    mine = {k: v for k, v in rows.items() if re.match(r"_Z14k_select_attrs", k)}
    assert len(mine) == 1, sorted(mine)
    (name, (vg, sg, lds, scratch)), = mine.items()
    print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
    assert scratch == 0 and lds == 0, (vg, sg, lds, scratch)
