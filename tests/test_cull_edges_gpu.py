"""k_cluster_cull at its edges: the sweeps of tests/cull_edge_cases.py rendered by a context with the cluster cull on and by its twin
with GSR_OPT_CLUSTER_CULL = 0 and GSR_OPT_OCCLUSION_CULL = 0 (the context under test has no occlusion cull either: these sweeps hold
the cull's own geometric margins, the horizons are tested in test_horizons_gpu.py).

Per scene (one variant, one splat shape; in every clump the even splats are opaque and the odd ones have the smallest float32 opacity
>= 1/255, the edge of K1's opacity clause; two frames of the same camera):
  (a) soundness: every cluster that holds a splat with a sort entry in the twin (debug_cull rect != 0xffffffff) is in the culled
      context's kept list; the records and rects of the splats the culled context keeps equal the twin's; both frames are bit-identical;
  (b) per sweep, the twin keeps some clumps and drops others: the sweep crosses K1's own boundary;
  (c) per sweep, the cull drops the outermost clump: the sweep reaches past every margin of the cull; and of the coincident clumps it
      drops every one that lies further out than the innermost one it drops: what it keeps is an inner run of the sweep;
  and, where the scene's clumps are spread over boxes (cull_edge_cases.py; their probe splats sit on the boxes' inner faces), the twin
  keeps some of the spread clumps and drops others, and the cull drops some -- (a) then holds what the cull takes over a BOX;
  and the flagged clumps (a NaN position off screen, an infinite scale behind the eye) are kept.
Band scenes render rows [2, 4) of 6 tile rows as shard 1 of 3 (GSR_OPT_SHARD_LAYOUT 1) and rows [3, 5) by set_row_band, both contexts
alike; since K1's own early `far` test is active in the banded twin as well, they are also held to a FULL-frame twin:
  (d) every clump whose rect in the full frame reaches a tile row of the band has a sort entry in the banded, culled context, and the
      band image equals those rows of the full frame.
Depth scenes render against a depth buffer that holds one value d0 everywhere, across which the clumps' window depths step; the second
frame of the same buffer is the one compared, and the context under test must have culled it against the depth pyramid (the plan's
dcull).  The depth rules are on only with GSR_OPT_OCCLUSION_CULL != 0, so there both contexts run with it at 2 -- the twin then has
K1's own per-splat depth rule and no cluster cull -- and the frames are also held bit for bit to the context with both stages off.
Each sweep prints a GAP line: the boundary coordinate of the outermost clump the twin keeps and of the innermost one the cull drops,
and their difference, in the boundary's unit (pixels for the screen edges, world depth for the planes) -- the room the margins give
away (LAB_NOTES.md, "Cluster cull at its edges")."""
import numpy as np
import pytest

import cull_edge_cases as K

pytestmark = pytest.mark.gpu

NO_ENTRY = 0xffffffff


@pytest.fixture(scope="module")
def engines(pkg):
    """the context under test, its twin without either cull stage, and a second such twin that never gets a band"""
    E = pkg.engine
    dut, twin, full = pkg.Engine(0), pkg.Engine(0), pkg.Engine(0)
    for e, on in ((dut, 1), (twin, 0), (full, 0)):
        e.set_option(E.OPT_CLUSTER_CULL, on)
        e.set_option(E.OPT_OCCLUSION_CULL, 0)
    yield dut, twin, full
    for e in (dut, twin, full):
        e.close()


def _frames(pkg, eng, sc, frames=2, band=None, depth_rule=True):
    s, cam = sc["splats"], sc["cam"]
    E = pkg.engine
    eng.upload(s, origin=sc["origin"])
    depth_cull = sc["d0"] is not None and depth_rule
    if depth_cull:
        eng.set_option(E.OPT_OCCLUSION_CULL, 2)        # (what turns the depth rules on; no horizon forms under a covered tile)
    if band and band[0] == "shard":
        eng.set_option(E.OPT_SHARD_LAYOUT, 1)
        eng.set_row_shard(*band[1])
    elif band:
        eng.set_row_band(*band[1])
    try:
        if sc["d0"] is None:
            imgs = [eng.render(cam) for _ in range(frames)]
        else:
            depth = np.full((cam.height, cam.width), sc["d0"], np.float32)
            imgs = [eng.render_depth(cam, depth) for _ in range(frames)]
        plan = eng.debug_last_plan()
        rec = eng.debug_records(s.n)
        rect, clus = eng.debug_cull(s.n)
        perm = eng.debug_storage_order(s.n).astype(np.int64)
    finally:
        if band:
            eng.set_row_shard(0, 1)
            eng.set_option(E.OPT_SHARD_LAYOUT, 0)
        if depth_cull:
            eng.set_option(E.OPT_OCCLUSION_CULL, 0)
    return imgs, rec, rect, clus, perm, plan


def check_scene(sc, dut_out, twin_out, label):
    """the asserts (a)-(c) and the flagged clumps; returns [(boundary, twin's outermost kept coord, cull's innermost dropped coord)]"""
    imgs, rec, rect, clus, perm = dut_out[:5]
    imgs0, rec0, rect0, clus0, perm0 = twin_out[:5]
    n = sc["splats"].n
    assert np.array_equal(perm, perm0), label
    slot = np.empty(n, np.int64)
    slot[perm] = np.arange(n)
    cluster = slot // 64
    nc = sc["clumps"]
    cl_of_clump = cluster.reshape(nc, K.CLUMP)
    assert (cl_of_clump == cl_of_clump[:, :1]).all(), f"{label}: a clump spans two clusters"
    cl_of_clump = cl_of_clump[:, 0]
    kept = np.zeros((n + 63) // 64, bool)
    kept[clus] = True
    assert len(clus0) == kept.size, f"{label}: the twin culled clusters"
    # (a) soundness
    need = np.unique(cluster[rect0 != NO_ENTRY])
    miss = need[~kept[need]]
    if miss.size:
        who = [int(np.nonzero(cl_of_clump == c)[0][0]) for c in miss]
        where = [(sw.boundary, float(sw.coord[sw.clumps.index(k)]), sw.kind[sw.clumps.index(k)]) for k in who for sw in sc["sweeps"] if k in sw.clumps]
        raise AssertionError(f"{label}: the cull dropped {miss.size} clusters the twin draws from: clumps {who} at {where}")
    vis = rec["visible"] == 1
    assert np.array_equal(rec[vis], rec0[vis]) and np.array_equal(rect[vis], rect0[vis]), f"{label}: records / rects of kept splats"
    assert np.array_equal(rect != NO_ENTRY, rect0 != NO_ENTRY), f"{label}: a splat lost its sort entry"
    for k, (a, b) in enumerate(zip(imgs, imgs0)):
        assert np.array_equal(a, b, equal_nan=True), f"{label}: frame {k} differs from the twin's"
    for name, k in sc["flagged"].items():
        assert kept[cl_of_clump[k]], f"{label}: the flagged clump ({name}) was culled"
    # (b), (c) per sweep
    entry = (rect0 != NO_ENTRY).reshape(nc, K.CLUMP).any(axis=1)
    out = []
    for sw in sc["sweeps"]:
        idx = np.array(sw.clumps)
        tw = entry[idx]
        cu = kept[cl_of_clump[idx]]
        assert tw.any() and not tw.all(), f"{label} {sw.boundary}: the twin keeps {int(tw.sum())} of {tw.size} clumps"
        assert not cu[-1], f"{label} {sw.boundary}: the cull kept the outermost clump (coordinate {sw.coord[-1]:.6g})"
        c_keep = float(sw.coord[tw].min())
        beyond = sw.coord < c_keep              # (not an inside clump that left the screen sideways)
        c_drop = float(sw.coord[~cu & beyond].max())
        # ... and every coincident clump past the innermost one it drops: what the cull keeps of them is an inner run, with no kept
        # clump out among the dropped ones (the sweep is ordered from inside to outside; a spread clump's box is its own, and a corner
        # of it may project further in than its probe, so those are not held to the order)
        point = ~sc["spread"][idx]
        if (~cu & beyond & point).any():
            p_drop = float(sw.coord[~cu & beyond & point].max())
            stray = cu & beyond & point & (sw.coord < p_drop)
            assert not stray.any(), (f"{label} {sw.boundary}: the cull drops the clump at {p_drop:.7g} but keeps "
                                     f"{int(stray.sum())} further out, at {sw.coord[stray].tolist()}")
        sp = ~point
        if sp.any():
            assert (tw & sp).any() and (~tw & sp).any() and (~cu & beyond & sp).any(), \
                f"{label} {sw.boundary}: of {int(sp.sum())} spread clumps the twin keeps {int((tw & sp).sum())}, the cull {int((cu & sp).sum())}"
            s_keep, s_drop = float(sw.coord[tw & sp].min()), float(sw.coord[~cu & beyond & sp].max())
            print(f"GAP {label} {sw.boundary} (spread clumps, by their probes): twin keeps to {s_keep:.7g}, cull drops from {s_drop:.7g}, "
                  f"gap {s_keep - s_drop:.7g} ({int((tw & sp).sum())} kept by the twin, {int((cu & sp).sum())} by the cull, of {int(sp.sum())})")
        print(f"GAP {label} {sw.boundary}: twin keeps to {c_keep:.7g}, cull drops from {c_drop:.7g}, gap {c_keep - c_drop:.7g} "
              f"({int(tw.sum())} kept by the twin, {int(cu.sum())} by the cull, of {tw.size})")
        out.append((sw.boundary, c_keep, c_drop))
    return out


def check_band(sc, dut_out, full_out, label):
    """(d): the banded, culled context against the full-frame twin"""
    lo, hi = sc["band"][2]
    img_full, rect_full = full_out[0][-1], full_out[2]
    rect = dut_out[2]
    j0, j1 = (rect_full >> 8) & 255, rect_full >> 24
    reach = (rect_full != NO_ENTRY) & (j1 >= lo) & (j0 < hi)
    nc = sc["clumps"]
    need = reach.reshape(nc, K.CLUMP).any(axis=1)
    got = (rect != NO_ENTRY).reshape(nc, K.CLUMP).any(axis=1)
    assert need.any(), f"{label}: no clump reaches the band"
    assert not (need & ~got).any(), f"{label}: clumps {np.nonzero(need & ~got)[0].tolist()} reach the band but have no entry"
    assert (reach <= (rect != NO_ENTRY)).all(), f"{label}: a splat that reaches the band has no entry"
    band_img = dut_out[0][-1]
    assert np.array_equal(band_img, img_full[16 * lo:16 * hi], equal_nan=True), f"{label}: the band differs from the full frame's rows"


@pytest.mark.parametrize("case", K.all_scenes(), ids=K.scene_id)
def test_sweeps_across_cull_boundaries(pkg, engines, case):
    dut, twin, full = engines
    sc = K.scene(pkg, *case)
    label = K.scene_id(case)
    band = sc["band"]
    got = _frames(pkg, dut, sc, band=band)
    check_scene(sc, got, _frames(pkg, twin, sc, band=band), label)
    if band:
        check_band(sc, got, _frames(pkg, full, sc), label)
    if sc["d0"] is not None:
        off = _frames(pkg, full, sc, depth_rule=False)
        for k, (a, b) in enumerate(zip(got[0], off[0])):
            assert np.array_equal(a, b, equal_nan=True), f"{label}: frame {k} differs from the frame with both cull stages off"
        assert got[5]["dcull"] == 1, f"{label}: the second frame of the buffer was not culled against its depth pyramid: {got[5]}"
