"""Position updates without a GPU: the NULL-handle errors of gsr_move / gsr_multi_move, the bookkeeping of GSplatRenderer::moveSplats on
a dry instance -- which upload-order range of the resident plan a registered row is, and that the row holds the new positions for the
next re-stage -- and the resources the compiler gives the new kernels."""
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
    P = np.zeros((1, 3), np.float32)
    assert L.gsr_move(None, 0, 1, P.ctypes.data, None, C.byref(u)) == GSR_E_INVALID
    assert L.gsr_move(None, 0, 0, None, None, None) == GSR_E_INVALID
    assert L.gsr_multi_move(None, 0, 1, P.ctypes.data, None, C.byref(u)) == GSR_E_INVALID
    assert L.gsr_multi_move(None, 0, 1, P.ctypes.data, None, None) == GSR_E_INVALID
    assert L.gsplat_renderer_move_splats(None, b"x", P.ctypes.data, None, *([None] * 7), None, None) == GSR_E_INVALID


def test_stats_carry_the_move_fields_last(pkg):
    """appended behind upload_ms, so a caller built against the shorter struct reads what it read before"""
    f = [n for n, _ in pkg.engine.gsr_stats._fields_]
    assert f[-4:] == ["uploads", "upload_ms", "moves", "move_ms"]
    assert C.sizeof(pkg.engine.gsr_stats) - pkg.engine.gsr_stats.moves.offset == 8 + 4 * 8
    assert C.sizeof(pkg.engine.gsr_attr_update) == 7 * C.sizeof(C.c_void_p)      # the update struct did not grow


def test_move_arrays_must_agree_in_length(pkg):
    E = pkg.engine
    P, n, u, keep = E.move_arrays(np.zeros((5, 3)), alpha=np.ones(5, np.float32))
    assert n == 5 and P.dtype == np.float32 and u.alpha == keep[0].ctypes.data and not u.Cd
    with pytest.raises(E.GsrError):
        E.move_arrays(np.zeros((5, 3), np.float32), alpha=np.ones(4, np.float32))
    with pytest.raises(E.GsrError):
        E.move_arrays(np.zeros(7, np.float32))


def _redraw(pkg, R, ids):
    for i in ids:
        R.includeInRenderPass(i)
    r = pkg.GSplatRenderer.context(pkg.camera.make_camera(64, 48))
    R.generateRenderGeometry(r); R.render(r); R.postRender()


def test_dry_shim_moves_a_resident_row(pkg, R):
    """three rows registered, two shown: the second shown row is the range behind the first one's splats; a row that is not shown is
    not resident; an unknown id and NULL positions are errors; the row holds the new positions for the next re-stage"""
    a, b, c = (pkg.scenes.make_scene(n, seed=3 + n, sh=True) for n in (100, 37, 64))
    ia, ib, ic = (R.registerUpdate(0x100 + k, (1, 0, 0, 0), 0, s) for k, s in enumerate((a, b, c)))
    assert ia < ib < ic
    _redraw(pkg, R, (ia, ic))
    assert R.query(R.Q_STAGING_COUNT) == 1 and R.query(R.Q_SPLAT_COUNT) == 164
    newc = np.ascontiguousarray(c.P[::-1])
    old_cd = R.rowArray(ic, 1)
    assert R.rowArray(ic, 0) == R._keep[ic].P.ctypes.data
    assert R.moveSplats(ic, newc) == (1, 100, 64)
    assert R.rowArray(ic, 0) == R._updates[ic]["P"].ctypes.data != R._keep[ic].P.ctypes.data
    assert np.array_equal(R._updates[ic]["P"], newc) and R.rowArray(ic, 1) == old_cd
    assert R.moveSplats(ia, a.P + 1.0, origin=(1.0, 2.0, 3.0), alpha=np.zeros(100, np.float32)) == (1, 0, 100)
    assert R.rowArray(ia, 2) == R._updates[ia]["alpha"].ctypes.data
    # the pass's origin: the mean over the two resident rows, as a re-stage forms it (c keeps its barycentre)
    want = (np.asarray((1.0, 2.0, 3.0), np.float32) + np.asarray(c.barycenter(), np.float32)) / np.float32(2)
    assert np.array_equal(R.origin(), want)
    assert R.query(R.Q_STAGING_COUNT) == 1                                  # nothing was staged again
    # not shown, so not resident: staged when it is next shown
    assert R.moveSplats(ib, b.P * 2.0) == (0, 0, 0)
    assert R.rowArray(ib, 0) == R._updates[ib]["P"].ctypes.data
    assert R.moveSplats("0xdead__0__1_0_0_0", newc)[0] == GSR_E_INVALID
    # NULL positions; one of the three SH arrays: refused, and the row keeps what it held
    L = pkg.load_library()
    held = R.rowArray(ic, 0)
    assert L.gsplat_renderer_move_splats(R.h, ic.encode(), None, None, *([None] * 7), None, None) == GSR_E_INVALID
    assert R.moveSplats(ic, c.P, shx=np.zeros((64, 16), np.uint16))[0] == GSR_E_INVALID
    assert R.rowArray(ic, 0) == held
    # a forced re-stage (another row joins) plans the rows as they are now
    _redraw(pkg, R, (ia, ib, ic))
    assert R.query(R.Q_STAGING_COUNT) == 2 and R.query(R.Q_SPLAT_COUNT) == 201
    assert R.rowArray(ib, 0) == R._updates[ib]["P"].ctypes.data
    assert R.moveSplats(ic, c.P) == (1, 137, 64)
    assert R.moveSplats(ib, b.P) == (1, 100, 37)


def test_dry_shim_move_while_another_resident_row_was_retired(pkg, R):
    """two rows resident; the first is registered again under a new cache version, so its old row leaves the registry while its splats
    are still resident; a move of the second with a new origin, in the same redraw and before the re-stage, counts as not resident --
    the resident pass's origin is not formed over a row that is gone -- and keeps the new positions and origin for the re-stage"""
    a, b = (pkg.scenes.make_scene(n, seed=3 + n, sh=True) for n in (100, 37))
    ia, ib = (R.registerUpdate(0x100 + k, (1, 0, 0, 0), 0, s) for k, s in enumerate((a, b)))
    _redraw(pkg, R, (ia, ib))
    assert R.query(R.Q_STAGING_COUNT) == 1 and R.query(R.Q_SPLAT_COUNT) == 137
    assert R.moveSplats(ib, b.P + 1.0, origin=(4.0, 5.0, 6.0)) == (1, 100, 37)      # both rows present: moved in place
    before = R.origin()
    ia2 = R.registerUpdate(0x100, (2, 0, 0, 0), 0, a, splatOrigin=(7.0, 8.0, 9.0))
    assert ia2 != ia and R.rowArray(ia, 0) == 0
    newb = np.ascontiguousarray(b.P[::-1])
    assert R.moveSplats(ib, newb, origin=(1.0, 2.0, 3.0)) == (0, 0, 0)
    assert np.array_equal(R.origin(), before)                                       # the stale plan's origin was left alone
    assert R.rowArray(ib, 0) == R._updates[ib]["P"].ctypes.data and np.array_equal(R._updates[ib]["P"], newb)
    assert R.moveSplats(ib, newb) == (0, 0, 0)                                      # and without an origin likewise
    assert R.query(R.Q_STAGING_COUNT) == 1
    # the redraw re-stages both rows as they are now, with the origin a re-stage forms: the mean of the two rows' origins
    _redraw(pkg, R, (ia2, ib))
    assert R.query(R.Q_STAGING_COUNT) == 2 and R.query(R.Q_SPLAT_COUNT) == 137
    assert np.array_equal(R.origin(), (np.asarray((7.0, 8.0, 9.0), np.float32) + np.asarray((1.0, 2.0, 3.0), np.float32)) / np.float32(2))
    assert R.moveSplats(ib, b.P, origin=(0.0, 0.0, 0.0)) == (1, 100, 37)
    # an attribute edit needs no row but its own: it is unchanged by a retired neighbour
    ia3 = R.registerUpdate(0x100, (3, 0, 0, 0), 0, a)
    assert ia3 != ia2 and R.updateAttributes(ib, alpha=np.zeros(37, np.float32)) == (1, 100, 37)


def test_new_kernels_stay_within_k_packs_budget():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): k_move_positions, both k_repack
    instantiations and k_cluster_bounds use no scratch, and no more vector registers or LDS than k_pack -- the kernel whose shape
    (512 threads per cluster) and occupancy they share"""
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

    for sh in ("Lb0E", "Lb1E"):
        pack = find("_Z6k_packI" + sh)
        for name in ("_Z8k_repackI" + sh, "_Z16k_move_positions", "_Z16k_cluster_bounds"):
            vg, sg, lds, scratch = find(name)
            print(f"{name}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}; k_pack<{sh}>: vgpr {pack[0]} lds {pack[2]}")
            assert scratch == 0 and vg <= pack[0] and lds <= pack[2], (name, (vg, sg, lds, scratch), pack)
