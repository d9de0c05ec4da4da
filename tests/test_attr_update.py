"""Attribute updates without a GPU: the NULL-handle errors of gsr_update / gsr_multi_update, and the bookkeeping of
GSplatRenderer::updateAttributes on a dry instance -- which upload-order range of the resident plan a registered row is, and that the
row holds the new arrays for the next re-stage -- and the resources the compiler gives the update kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1


@pytest.fixture()
def R(pkg):
    r = pkg.GSplatRenderer(-1)
    yield r
    r.close()


def test_null_handles_are_invalid(pkg):
    L = pkg.load_library()
    u = pkg.engine.gsr_attr_update()
    assert L.gsr_update(None, 0, 0, C.byref(u)) == GSR_E_INVALID
    assert L.gsr_update(None, 0, 0, None) == GSR_E_INVALID
    assert L.gsr_multi_update(None, 0, 0, C.byref(u)) == GSR_E_INVALID
    assert L.gsr_debug_read_resident(None, 0, None, 0) == GSR_E_INVALID
    assert L.gsplat_renderer_update_attributes(None, b"x", *([None] * 7), None, None) == GSR_E_INVALID


def test_struct_matches_the_header(pkg):
    """seven pointers, in the header's order"""
    E = pkg.engine
    assert [n for n, _ in E.gsr_attr_update._fields_] == ["Cd", "alpha", "scale", "orient", "shx", "shy", "shz"]
    assert C.sizeof(E.gsr_attr_update) == 7 * C.sizeof(C.c_void_p)


def test_update_arrays_must_agree_in_length(pkg):
    E = pkg.engine
    u, n, keep = E.attr_update_struct(Cd=np.zeros((5, 3), np.uint16), alpha=np.ones(5, np.float32))
    assert n == 5 and u.Cd == keep[0].ctypes.data and u.alpha == keep[1].ctypes.data and not u.scale and not u.shx
    with pytest.raises(E.GsrError):
        E.attr_update_struct(Cd=np.zeros((5, 3), np.uint16), alpha=np.ones(4, np.float32))
    with pytest.raises(E.GsrError):
        E.attr_update_struct(orient=np.zeros(7, np.uint16))
    assert E.attr_update_struct()[1] == 0


def _redraw(pkg, R, ids):
    for i in ids:
        R.includeInRenderPass(i)
    r = pkg.GSplatRenderer.context(pkg.camera.make_camera(64, 48))
    R.generateRenderGeometry(r); R.render(r); R.postRender()


def test_dry_shim_addresses_a_resident_row(pkg, R):
    """three rows registered, two shown: the second shown row is the range behind the first one's splats; a row that is not shown is
    not resident; an unknown id and SH arrays for a row without SH are errors; the row keeps the new arrays for the next re-stage"""
    a, b, c = (pkg.scenes.make_scene(n, seed=3 + n, sh=True) for n in (100, 37, 64))
    ia, ib, ic = (R.registerUpdate(0x100 + k, (1, 0, 0, 0), 0, s) for k, s in enumerate((a, b, c)))
    assert ia < ib < ic                                                     # the plan packs rows in id order
    _redraw(pkg, R, (ia, ic))
    assert R.query(R.Q_STAGING_COUNT) == 1 and R.query(R.Q_SPLAT_COUNT) == 164
    cd = np.full((64, 3), 0x3c00, np.uint16)
    al = np.full(64, 0.25, np.float32)
    old_scale = R.rowArray(ic, 3)
    assert R.updateAttributes(ic, Cd=cd, alpha=al) == (1, 100, 64)
    assert R.updateAttributes(ia, alpha=np.zeros(100, np.float32)) == (1, 0, 100)
    assert R.query(R.Q_STAGING_COUNT) == 1                                  # in place: nothing was staged again
    # the row holds the arrays the binding keeps alive for it, and the attributes that were not given stay
    keep = R._updates[ic]
    assert R.rowArray(ic, 1) == keep["Cd"].ctypes.data and R.rowArray(ic, 2) == keep["alpha"].ctypes.data
    assert R.rowArray(ic, 3) == old_scale and R.rowArray(ic, 0) == R._keep[ic].P.ctypes.data
    # not shown, so not resident: staged when it is next shown
    new_b = np.zeros((37, 3), np.uint16)
    assert R.updateAttributes(ib, Cd=new_b) == (0, 0, 0)
    assert R.rowArray(ib, 1) == R._updates[ib]["Cd"].ctypes.data
    assert R.updateAttributes("0xdead__0__1_0_0_0", Cd=cd)[0] == GSR_E_INVALID
    # one of the three SH arrays; SH arrays for a row registered without SH
    sh = np.zeros((64, 16), np.uint16)
    assert R.updateAttributes(ic, shx=sh)[0] == GSR_E_INVALID
    d = pkg.scenes.make_scene(10, seed=9, sh=False)
    idd = R.registerUpdate(0x103, (1, 0, 0, 0), 0, d)
    sh10 = np.zeros((10, 16), np.uint16)
    assert R.updateAttributes(idd, shx=sh10, shy=sh10, shz=sh10)[0] == GSR_E_INVALID
    assert R.updateAttributes(ic, shx=sh, shy=sh, shz=sh) == (1, 100, 64)
    assert R.rowArray(ic, 5) == R._updates[ic]["shx"].ctypes.data
    # a forced re-stage (another row joins) plans the rows as they are now: b's new colours, c behind a and b
    _redraw(pkg, R, (ia, ib, ic))
    assert R.query(R.Q_STAGING_COUNT) == 2 and R.query(R.Q_SPLAT_COUNT) == 201
    assert R.rowArray(ib, 1) == R._updates[ib]["Cd"].ctypes.data
    assert R.updateAttributes(ic, alpha=al) == (1, 137, 64)
    assert R.updateAttributes(ib, alpha=np.ones(37, np.float32)) == (1, 100, 37)
    # the binding keeps ONE array per attribute of a row alive -- the one the row holds -- however many edits there were
    for _ in range(3):
        assert R.updateAttributes(ic, alpha=al.copy())[0] == 1
    assert sorted(R._updates[ic]) == ["Cd", "alpha", "shx", "shy", "shz"]
    assert R.rowArray(ic, 2) == R._updates[ic]["alpha"].ctypes.data
    assert R.registerUpdate(0x102, (2, 0, 0, 0), 0, c) != ic and ic not in R._updates      # a new cache version retires the row
    R.flushEntriesForMatchingDetail(ib)
    assert ib not in R._updates and ia in R._updates


def test_dry_shim_truncated_row_updates_what_is_resident(pkg):
    """the row that crosses the 2^23 - 1 budget is resident only up to the budget: n is the truncated count (NULL arrays: only the
    counts matter on a dry instance)"""
    L = pkg.load_library()
    h = L.gsplat_renderer_create(-1)
    try:
        ver = (C.c_int64 * 4)(1, 0, 0, 0)
        org = (C.c_float * 3)(0, 0, 0)
        ids = []
        for k, cnt in enumerate((5_000_000, 3_000_000, 2_000_000)):
            buf = C.create_string_buffer(128)
            L.gsplat_renderer_register_update(h, 0x100 + k, ver, 0, cnt, org, *([None] * 8), 0, buf, 128)
            ids.append(buf.value)
        for i in ids:
            L.gsplat_renderer_include_in_render_pass(h, i)
        r = pkg.engine.GSplatRenderContext()
        L.gsplat_renderer_generate_render_geometry(h, C.byref(r))
        alpha = np.zeros(8, np.float32)                                     # (never read: a dry instance only keeps the pointer)
        first, n = C.c_int64(-1), C.c_int64(-1)
        args = (None, alpha.ctypes.data, None, None, None, None, None, C.byref(first), C.byref(n))
        assert L.gsplat_renderer_update_attributes(h, ids[2], *args) == 1
        assert (first.value, n.value) == (8_000_000, (1 << 23) - 1 - 8_000_000)
        assert L.gsplat_renderer_update_attributes(h, ids[1], *args) == 1
        assert (first.value, n.value) == (5_000_000, 3_000_000)
        assert L.gsplat_renderer_row_array(h, ids[1], 2) == alpha.ctypes.data
    finally:
        L.gsplat_renderer_destroy(h)


def test_update_kernels_stay_within_k_packs_budget():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): both instantiations of k_update and of
    k_update_f32, and k_cluster_extents, exist, use no scratch, and no more vector registers or LDS than k_pack<true> -- the kernel
    whose shape (512 threads, eight lanes per splat, one LDS row per splat) the update kernels share"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])

    def find(prefix):
        hit = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, [k for k in rows if k.startswith(prefix)])
        return hit[0]

    pack = find("_Z6k_packILb1E")
    for name in ("_Z8k_updateILb0E", "_Z8k_updateILb1E", "_Z12k_update_f32ILb0E", "_Z12k_update_f32ILb1E", "_Z17k_cluster_extents"):
        vg, sg, lds, scratch = find(name)
        print(f"{name}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}; k_pack<true>: vgpr {pack[0]} lds {pack[2]}")
        assert scratch == 0 and vg <= pack[0] and lds <= pack[2], (name, (vg, sg, lds, scratch), pack)
