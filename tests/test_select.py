"""Selection without a GPU (include/gsplat_hip.h, "selection"): gsr_select_eval -- the rule the kernel evaluates, on the host -- against
the oracle's records bit for bit, the case table's own conditions, the exact edges of the rect and the depth test, the refusals, the
header's constants and struct, and the resources the compiler gives k_select.  No tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import select_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
NAMES = SC.case_names()
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_case_table_covers_what_its_header_says(pkg):
    cs = SC.cases(pkg)
    assert [c.name for c in cs] == SC.case_names(pkg.engine.SELECT_BLOCK) == NAMES
    assert {c.n for c in cs} == {1, 33, 64, 65, 357, pkg.engine.SELECT_BLOCK + 1}
    assert {(c.cam.width, c.cam.height) for c in cs} == set(SC.FRAMES)
    assert {c.kind for c in cs} == {"persp", "ortho", "offcentre"}
    assert any(any(c.origin) for c in cs) and any(not any(c.origin) for c in cs)
    assert any(((c.n + 31) // 32) % 2 for c in cs)                      # an odd word count
    for c in cs:
        assert c.image.shape == c.depth.shape == (c.cam.height, c.cam.width)
    assert any(c.cam.width % 32 for c in cs)                            # image bits cross word boundaries inside a row


# ---- (a) the restated chain against the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_centres_equal_the_oracle_s_records(pkg, oracle, name):
    c = SC.case(pkg, name)
    rec = oracle.preprocess(c.splats, c.cam, c.origin)
    # (the oracle's `visible` has no opacity test -- its fragments are discarded one by one -- so the centres are taken without it too)
    hit, centre = c.eval(pkg, centres=True, rect=None, image=False, depth=False, any_opacity=True)
    vis = rec["visible"] != 0
    if c.n >= 33:
        assert vis.sum() >= c.n // 2, "the oracle sees too few splats for the comparison to mean anything"
    assert not np.isnan(centre[vis]).any(), "a record the oracle calls visible is not selectable"
    for k, field in enumerate(("cx", "cy", "zwin")):
        assert np.array_equal(_bits(centre[vis, k]), _bits(rec[field][vis])), (name, field)
    assert hit[vis].all()                                               # the everywhere-rect hits every visible record
    # what is not selectable carries three NaNs and is never hit
    off = np.isnan(centre).any(axis=1)
    assert np.isnan(centre[off]).all() and not hit[off].any() and not (off & vis).any()
    # with the opacity test: the same centres, bit for bit, on the splats at or above 1/255, and three NaNs below
    hit_d, centre_d = c.eval(pkg, centres=True, rect=None, image=False, depth=False)
    opaque = c.splats.alpha >= np.float32(1.0) / np.float32(255.0)
    assert np.array_equal(_bits(centre_d[opaque & ~off]), _bits(centre[opaque & ~off])) and np.isnan(centre_d[~opaque]).all()
    assert np.array_equal(hit_d, hit & opaque)


# ---- (b) the cases are not vacuous --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cases_are_not_vacuous(pkg, name):
    c = SC.case(pkg, name)
    full = c.eval(pkg)
    if c.n == 1:                                                        # (0 < hits < 1 has no solution: one case hits, the other does not)
        assert bool(full[0]) == (name == "n1_hit")
        return
    assert 0 < full.sum() < c.n, (name, int(full.sum()))
    alone = {"rect": c.eval(pkg, rect=None) & ~full, "image": c.eval(pkg, image=False) & ~full, "depth": c.eval(pkg, depth=False) & ~full,
             "opacity": c.eval(pkg, any_opacity=True) & ~full}
    _, centre = c.eval(pkg, centres=True, any_opacity=True)
    alone["clip"] = np.isnan(centre).any(axis=1) & (c.splats.alpha >= np.float32(1.0) / np.float32(255.0))
    for clause, m in alone.items():
        assert m.any(), f"{name}: no splat fails on the {clause} clause alone"
    # the seeded splats do what they were seeded for
    at = c.specials
    for label in ("behind", "beyond_far", "nan", "inf_x", "neg_inf_z"):
        assert alone["clip"][at[label]], (name, label)
    assert alone["opacity"][at["below_255"]] and alone["opacity"][at["zero_opacity"]] and full[at["exactly_255"]], name
    # ... and hits exist through each forced outcome: some splat inside the rect was hit, some was not
    assert (full & ~c.eval(pkg, rect=None, image=False, depth=False)).sum() == 0


# ---- (c) exact edges, from a host-evaluated centre -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n != "n1_behind"])
def test_exact_edges(pkg, name):
    E = pkg.engine
    c = SC.case(pkg, name)
    hit, centre = c.eval(pkg, centres=True, rect=None, image=False, depth=False)
    w, h = c.cam.width, c.cam.height
    inside = hit & (centre[:, 0] >= 0) & (centre[:, 0] < w) & (centre[:, 1] >= 0) & (centre[:, 1] < h)
    ks = np.flatnonzero(inside)[:5]
    assert ks.size
    ev = lambda region, k: bool(E.select_eval(c.cam, c.origin, region, c.splats.P[k:k + 1], c.splats.alpha[k:k + 1])[0])
    for k in ks:
        cx, cy, zw = (np.float32(v) for v in centre[k])
        assert ev(E.select_region((cx, -INF, INF, INF)), k), "x0 = cx hits"
        assert not ev(E.select_region((-INF, -INF, cx, INF)), k), "x1 = cx misses"
        assert ev(E.select_region((-INF, cy, INF, INF)), k), "y0 = cy hits"
        assert not ev(E.select_region((-INF, -INF, INF, cy)), k), "y1 = cy misses"
        assert ev(E.select_region((np.nextafter(cx, np.float32(-INF)), -INF, np.nextafter(cx, np.float32(INF)), INF)), k)
        depth = np.ones((h, w), np.float32)
        p = (int(cy), int(cx))
        depth[p] = zw
        assert ev(E.select_region(None, depth=depth, depth_bias=0.0), k), "depth[p] = zw, bias 0, hits"
        depth[p] = np.nextafter(zw, np.float32(-INF))
        assert not ev(E.select_region(None, depth=depth, depth_bias=0.0), k), "the next float below misses"
        depth[:] = 0.0
        depth[p] = zw                                                   # only its own texel is looked at
        assert ev(E.select_region(None, depth=depth), k)
        image = np.zeros((h, w), bool)
        image[p] = True
        assert ev(E.select_region(None, image=image), k), "its own bit, and no other"
        assert not ev(E.select_region(None, image=~image), k)


def test_pixel_clause_outside_the_image(pkg):
    """a centre outside the frame: hit by the everywhere-rect alone, never with an image or a depth buffer (no index is formed)"""
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    w, h = c.cam.width, c.cam.height
    wide = pkg.camera.make_camera(w, h, sh_order=3, frame=4, distance=1.6, near=0.01, far=50.0)
    hit, centre = E.select_eval(wide, c.origin, E.select_region(None), c.splats.P, c.splats.alpha, centres=True)
    out = hit & ~((centre[:, 0] >= 0) & (centre[:, 0] < w) & (centre[:, 1] >= 0) & (centre[:, 1] < h))
    assert out.sum() >= 10
    img = E.select_eval(wide, c.origin, E.select_region(None, image=np.ones((h, w), bool)), c.splats.P, c.splats.alpha)
    dep = E.select_eval(wide, c.origin, E.select_region(None, depth=np.ones((h, w), np.float32)), c.splats.P, c.splats.alpha)
    assert not img[out].any() and not dep[out].any()
    assert np.array_equal(img, hit & ~out) and np.array_equal(dep, hit & ~out)


# ---- (d) refusals, the header, a NaN rect --------------------------------------------------------------------------------------------
def test_null_handles_and_bad_structs(pkg):
    L, E = pkg.load_library(), pkg.engine
    c = SC.case(pkg, "n33_ortho_origin")
    cs = E.camera_struct(c.cam)
    r, _ = E.select_region(None)
    w = np.full(2, 0xdeadbeef, np.uint32)
    cnt = C.c_int64(-7)
    assert L.gsr_select(None, C.byref(cs), C.byref(r), w.ctypes.data, 0, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_multi_select(None, C.byref(cs), C.byref(r), w.ctypes.data, C.byref(cnt), C.byref(cnt)) == GSR_E_INVALID
    assert L.gsr_get_select(None, None, None, None) == GSR_E_INVALID
    assert cnt.value == -7 and (w == 0xdeadbeef).all()
    P, a = c.splats.P, c.splats.alpha
    hit = np.full(c.n, 9, np.uint8)
    o3 = (C.c_float * 3)(*c.origin)
    call = lambda cam, origin, reg, p=P: L.gsr_select_eval(cam, origin, reg, p.ctypes.data if p is not None else None, a.ctypes.data, c.n, hit.ctypes.data, None)
    assert call(C.byref(cs), o3, C.byref(r)) == 0 and set(hit.tolist()) <= {0, 1}
    hit[:] = 9
    assert call(None, o3, C.byref(r)) == GSR_E_INVALID and call(C.byref(cs), None, C.byref(r)) == GSR_E_INVALID
    assert call(C.byref(cs), o3, None) == GSR_E_INVALID and call(C.byref(cs), o3, C.byref(r), None) == GSR_E_INVALID
    for field, value in (("op", 5), ("op", -1), ("flags", 2), ("flags", 3), ("reserved_", 1)):
        bad, _ = E.select_region(None)
        setattr(bad, field, value)
        assert call(C.byref(cs), o3, C.byref(bad)) == GSR_E_INVALID, (field, value)
    for field, value in (("width", 0), ("height", 0), ("width", E.MAX_DIM + 1), ("height", -3)):
        cam = E.camera_struct(c.cam)
        setattr(cam, field, value)
        assert call(C.byref(cam), o3, C.byref(r)) == GSR_E_INVALID, (field, value)
    assert (hit == 9).all(), "a refusal wrote something"
    assert L.gsr_select_eval(C.byref(cs), o3, C.byref(r), None, None, 0, None, None) == 0      # no splats: nothing is read


def test_header_constants_struct_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("REPLACE", 0), ("ADD", 1), ("SUBTRACT", 2), ("INTERSECT", 3), ("TOGGLE", 4), ("ANY_OPACITY", 1), ("BLOCK", 256)):
        assert int(re.search(r"#define GSR_SELECT_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(E, "SELECT_" + name)
    assert SC.OPS == ("REPLACE", "ADD", "SUBTRACT", "INTERSECT", "TOGGLE")
    body = hdr[hdr.index("typedef struct gsr_select_region {"):hdr.index("} gsr_select_region;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == [n for n, _ in E.gsr_select_region._fields_]
    assert C.sizeof(E.gsr_select_region) == 64 and E.gsr_select_region.depth.offset == 32 and E.gsr_select_region.op.offset == 48
    for sym in ("gsr_select", "gsr_select_eval", "gsr_get_select", "gsr_multi_select"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr)
    assert "picking" not in hdr


def test_nan_and_empty_rects_hit_nothing(pkg):
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    everywhere = c.eval(pkg, rect=None, image=False, depth=False)
    assert everywhere.sum() > 300
    nan = float("nan")
    for rect in ((nan, -INF, INF, INF), (-INF, nan, INF, INF), (-INF, -INF, nan, INF), (-INF, -INF, INF, nan), (nan, nan, nan, nan),
                 (10.0, 10.0, 10.0, 50.0), (50.0, 10.0, 10.0, 50.0), (INF, -INF, INF, INF)):
        assert not c.eval(pkg, rect=rect, image=False, depth=False).any(), rect
    assert np.array_equal(c.eval(pkg, rect=(-INF, -INF, INF, INF), image=False, depth=False), everywhere)
    # a NaN depth texel or a NaN bias: no hit at that pixel
    _, centre = c.eval(pkg, centres=True, rect=None, image=False, depth=False)
    d = np.full((c.cam.height, c.cam.width), nan, np.float32)
    assert not E.select_eval(c.cam, c.origin, E.select_region(None, depth=d), c.splats.P, c.splats.alpha).any()
    d[:] = 1.0
    assert not E.select_eval(c.cam, c.origin, E.select_region(None, depth=d, depth_bias=nan), c.splats.P, c.splats.alpha).any()


def test_python_region_handling(pkg):
    E = pkg.engine
    img = np.random.default_rng(2).random((61, 97)) < 0.5
    words = E.pack_image(img)
    assert words.dtype == np.uint32 and words.size == (61 * 97 + 31) // 32
    p = 17 * 97 + 45
    assert bool((words[p >> 5] >> (p & 31)) & 1) == bool(img[17, 45])
    assert np.array_equal(E.unpack_mask(words, 61 * 97), img.reshape(-1))
    r, keep = E.select_region((1, 2, 3, 4), image=img, depth=np.ones((61, 97)), depth_bias=0.5, op=E.SELECT_TOGGLE, any_opacity=True)
    assert (r.x0, r.y0, r.x1, r.y1, r.depth_bias, r.op, r.flags, r.reserved_) == (1, 2, 3, 4, 0.5, 4, 1, 0)
    assert r.image == keep[0].ctypes.data and r.depth == keep[1].ctypes.data and not r.image_is_device and not r.depth_is_device
    r, keep = E.select_region(None, image_device=4096, depth_device=8192)
    assert (r.x0, r.x1, r.image, r.image_is_device, r.depth, r.depth_is_device, keep) == (-INF, INF, 4096, 1, 8192, 1, [])
    with pytest.raises(E.GsrError):
        E.select_region(None, image=img, image_device=4096)
    cam = pkg.camera.make_camera(97, 61)
    with pytest.raises(E.GsrError):                                     # an image of another frame's size: refused before the library reads it
        E.select_eval(cam, (0, 0, 0), E.select_region(None, image=img[:30]), np.zeros((1, 3), np.float32))
    with pytest.raises(E.GsrError):
        E.select_eval(cam, (0, 0, 0), E.select_region(None), np.zeros((2, 3), np.float32), np.ones(3, np.float32))


# ---- (e) from the code object ---------------------------------------------------------------------------------------------------------
def test_select_kernel_exists_and_uses_no_scratch():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): k_select is there, once, and uses neither
    scratch nor LDS"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    mine = {k: v for k, v in rows.items() if re.match(r"_Z8k_select", k)}
    assert len(mine) == 1, sorted(mine)
    (name, (vg, sg, lds, scratch)), = mine.items()
    print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
    assert scratch == 0 and lds == 0, (vg, sg, lds, scratch)
