"""K1 (the four k_preprocess instantiations) and k_cluster_cull read the frame constants from the kernel's argument segment, phase by phase
(csrc/gsr_device.h: gsr_frame_fetch), instead of holding the whole GsrFrame in registers.  A wrong offset or a stale field in ANY part of
the frame must show up here, on the smallest inputs that reach every field:

  * the cloud: 5 x 64 + 1 splats.  64 of them sit behind the camera and fill storage cluster 0 (k_cluster_cull must drop it), the 257
    others fill clusters 1..4 and leave ONE splat in the partial cluster 5;
  * an object transform with rotation, non-uniform scale and translation (ov, ob, io, sigma_vo2), a non-zero origin;
  * SH orders 0..3; the shading and the colour-pending K1 (GSR_OPT_LAZY_COLOUR 0 / 2);
  * a perspective, an off-centre and an orthographic camera on 100 x 70 pixels (limx != limy), and a frame 4112 pixels wide and three
    tiles high: 257 tiles a side, so rects are packed in pairs of tiles (rect_shift = 1);
  * a band shard (shard_rpb, sigma_vo2 and the extent bound of gsr_k1_front);
  * eight big opaque splats on the camera's side of the ball, which close every tile of the small perspective frames.  The culled
    frames of this cloud read the horizon pyramid through the frame's level offsets, tile counts and dilation, but every horizon in it is
    +inf: k_tile_pass places a horizon 1024 list entries behind the point where a tile went opaque, and no list here is that long.  The
    second test renders a cloud of 60 000 splats for finite ones;
  * front-slab frames with a slab key picked on the device (phase 1 and phase 2), culled second and third frames (the horizon pyramid's
    level offsets, cull_dilate), and the depth-tested twins under a depth buffer that holds a sphere.

THE REFERENCE IS THE CPU ORACLE, as in test_gpu_parity.py::test_records_bit_exact: for every splat a frame keeps, its record and its sort
key equal the oracle's bit for bit, and the oracle keeps it too.  The oracle forms no tile rects and no cluster list, so those are held
to the rules themselves: a kept splat's rect is the pixel box of its own record (centre -+ half extent, clamped to the frame, in rect
units) restated here in float32, and the cluster list is ascending, inside the cloud, holds the cluster of every splat the frame keeps --
and, where nothing is culled by occlusion, of every splat the frame with both cull stages off keeps -- and does not hold cluster 0.
Every frame of every case is also bit-identical, pixels, records, keys and rects, to the same context with GSR_OPT_CLUSTER_CULL = 0 and
GSR_OPT_OCCLUSION_CULL = 0.
"""
import os

import numpy as np
import pytest

from helpers import OBJECT_MATRIX

pytestmark = pytest.mark.gpu

REC_FIELDS = ("cx", "cy", "a1x", "a1y", "b1x", "b1y", "r", "g", "b", "la")
ORIGIN = (0.25, -0.5, 0.125)
N_FAR, N_WALL, N = 64, 8, 5 * 64 + 1


OBJ = OBJECT_MATRIX


def _cameras(pkg, kind, sh_order, frames=3):
    """three frames of a slow orbit (the view moves between a frame and the culled one behind it)"""
    C = pkg.camera
    kw = dict(sh_order=sh_order, object_matrix=OBJ, step_deg=1.0)
    if kind == "persp":
        return [C.make_camera(100, 70, frame=180 + k, **kw) for k in range(frames)]
    if kind == "offcentre":
        return [C.make_camera(100, 70, frame=180 + k, proj_matrix=C.frustum(-0.003, 0.005, -0.002, 0.0035, 0.01, 1.0e3), **kw) for k in range(frames)]
    if kind == "ortho":
        return [C.make_camera(100, 70, frame=180 + k, proj_matrix=C.orthographic(-1.7, 1.3, -1.0, 1.2, 0.01, 100.0), **kw) for k in range(frames)]
    if kind == "wide":
        return [C.make_camera(4112, 40, frame=180 + k, p00=0.6, **kw) for k in range(frames)]
    raise KeyError(kind)


@pytest.fixture(scope="module")
def cloud(pkg, oracle):
    """the splats (object space) and what the storage order makes of them"""
    s = pkg.scenes.make_scene(N, seed=77, sh=True, log_scale_range=(-2.6, -1.8))
    rng = np.random.default_rng(78)
    s.alpha[:] = np.where(rng.uniform(size=N) < 0.75, 0.97, s.alpha).astype(np.float32)
    s.alpha[N_FAR + 5] = 0.003               # below 1 / 255: the opacity clause of the clip test
    cam = _cameras(pkg, "persp", 3)[0]
    # a WALL of N_WALL big opaque splats on the camera's side of the ball: the tiles in the middle of the frame go opaque at its depth,
    # leave depth horizons, and the splats behind it are what the culled frames drop
    to_cam = np.linalg.inv(OBJ) @ np.append(0.55 * cam.cam_pos.astype(np.float64) / np.linalg.norm(cam.cam_pos), 1.0)
    wall = slice(N_FAR + 10, N_FAR + 10 + N_WALL)
    s.P[wall] = (to_cam[:3] + 0.04 * rng.standard_normal((N_WALL, 3))).astype(np.float32)
    s.scale[wall] = pkg.scenes.f16bits(np.full((N_WALL, 3), 3.0))
    s.alpha[wall] = 1.0
    behind = np.linalg.inv(OBJ) @ np.append(2.0 * cam.cam_pos.astype(np.float64), 1.0)     # twice as far out as the camera, in object space
    s.P[:N_FAR] = (behind[:3] + 0.05 * rng.standard_normal((N_FAR, 3))).astype(np.float32)
    order = oracle.storage_order(s.P)        # order[j] = upload index of the splat in storage slot j
    slot = np.empty(N, np.int64)
    slot[order] = np.arange(N)
    assert sorted(order[:64].tolist()) == list(range(N_FAR)), "the 64 splats behind the camera are storage cluster 0"
    ref = oracle.preprocess(s, cam, origin=ORIGIN)
    assert ref["visible"][:N_FAR].sum() == 0 and ref["visible"][N_FAR:].sum() > 200
    assert ref["visible"][order[N - 1]] == 1, "the one splat of the partial cluster is in view"
    return s, slot // 64


@pytest.fixture(scope="module")
def engines(pkg):
    """the context under test and the same with both cull stages off; slabs of one cluster so that BOTH front-slab phases draw (the
    library reads the A/B hooks when a context is created)"""
    E = pkg.engine
    old = {k: os.environ.get(k) for k in ("GSR_SLAB_MIN", "GSR_SLAB_MAX")}
    os.environ["GSR_SLAB_MIN"], os.environ["GSR_SLAB_MAX"] = "1", "2"
    try:
        dut, plain = pkg.Engine(0), pkg.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    plain.set_option(E.OPT_CLUSTER_CULL, 0)
    plain.set_option(E.OPT_OCCLUSION_CULL, 0)
    yield dut, plain
    dut.close()
    plain.close()


def _rects_from_records(rec, width, height):
    """gsr_k1_back's rule in float32: the pixels whose centres lie inside centre -+ half extent, clamped to the frame, in rect units"""
    f = np.float32
    g4 = 4 + (0 if max((width + 15) // 16, (height + 15) // 16) <= 256 else 1)
    cx, cy, hx, hy = rec["cx"], rec["cy"], rec["hx"], rec["hy"]
    xlo, xhi = (cx - hx) - f(0.5), (cx + hx) - f(0.5)
    ylo, yhi = (cy - hy) - f(0.5), (cy + hy) - f(0.5)
    i0 = np.ceil(np.maximum(xlo, f(0))).astype(np.int64) >> g4
    i1 = np.floor(np.minimum(xhi, f(width - 1))).astype(np.int64) >> g4
    j0 = np.ceil(np.maximum(ylo, f(0))).astype(np.int64) >> g4
    j1 = np.floor(np.minimum(yhi, f(height - 1))).astype(np.int64) >> g4
    return (i0 | (j0 << 8) | (i1 << 16) | (j1 << 24)).astype(np.uint32)


def _run(pkg, eng, splats, cams, opts, shard, depth):
    """upload, set the case's options, render the frames; -> images, the last frame's records, rects, cluster list and the stats"""
    E = pkg.engine
    eng.upload(splats, origin=ORIGIN)
    eng.stats_reset()
    for k, v in opts.items():
        eng.set_option(k, v)
    if shard:
        eng.set_option(E.OPT_SHARD_LAYOUT, 1)
        eng.set_row_shard(*shard)
    try:
        imgs = [eng.render(c) if depth is None else eng.render_depth(c, depth) for c in cams]
        rec = eng.debug_records(splats.n)
        rect, clus = eng.debug_cull(splats.n)
        st = eng.stats()
    finally:
        if shard:
            eng.set_row_shard(0, 1)
            eng.set_option(E.OPT_SHARD_LAYOUT, 0)
    return imgs, rec, rect, clus, st


def _check_against_oracle(oracle, splats, cam, rec, rect, clus, cluster_of, cluster_cull):
    ref = oracle.preprocess(splats, cam, origin=ORIGIN)
    vis = rec["visible"] == 1
    assert (ref["visible"][vis] == 1).all(), "the frame keeps a splat the oracle drops"
    assert np.array_equal(rec["key"][vis].view(np.uint32), ref["key"][vis].view(np.uint32))
    for f in REC_FIELDS:
        a, b = rec[f][vis].view(np.uint32), ref[f][vis].view(np.uint32)
        assert np.array_equal(a, b), f"field {f}: {np.count_nonzero(a != b)} mismatches"
    for f in ("hx", "hy"):                   # (not parity-relevant: shrunk to where alpha can reach 1 / 255)
        assert (rec[f][vis] <= ref[f][vis]).all() and (rec[f][vis] > 0).all()
    assert np.array_equal(rect[vis], _rects_from_records(rec[vis], cam.width, cam.height))
    assert (rect[~vis] == 0xffffffff).all()
    nclus = (splats.n + 63) // 64
    assert (np.diff(clus.astype(np.int64)) > 0).all() and (clus < nclus).all(), clus
    assert set(cluster_of[vis].tolist()) <= set(clus.tolist()), "a kept splat outside the surviving clusters"
    if cluster_cull:
        assert 0 not in clus, "the cluster behind the camera survived"
    return vis


# name: (camera kind, SH order, lazy colour, occlusion cull of the context under test, band shard, depth buffer)
CASES = {
    "persp sh0": ("persp", 0, 0, 2, None, False),
    "persp sh1": ("persp", 1, 0, 2, None, False),
    "persp sh2": ("persp", 2, 0, 2, None, False),
    "persp sh3": ("persp", 3, 0, 2, None, False),
    "persp sh3 pending": ("persp", 3, 2, 2, None, False),
    "persp sh3 cluster cull alone": ("persp", 3, 0, 0, None, False),
    "offcentre": ("offcentre", 3, 0, 2, None, False),
    "ortho": ("ortho", 2, 0, 2, None, False),
    "wide": ("wide", 3, 0, 2, None, False),
    "band": ("persp", 3, 0, 2, (1, 3), False),
    "band pending": ("persp", 1, 2, 0, (0, 2), False),
    "slab": ("persp", 3, 0, 3, None, False),
    "slab pending": ("offcentre", 2, 2, 3, None, False),
    "depth": ("persp", 3, 0, 2, None, True),
    "depth pending": ("persp", 3, 2, 2, None, True),
    "depth slab": ("persp", 2, 0, 3, None, True),
    "depth band": ("persp", 3, 0, 0, (0, 2), True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_frame_fields_reach_k1_and_cluster_cull(pkg, oracle, engines, cloud, case):
    kind, order, lazy, cull, shard, with_depth = CASES[case]
    E = pkg.engine
    dut, plain = engines
    splats, cluster_of = cloud
    cams = _cameras(pkg, kind, order)
    depth = pkg.scenes.sphere_occluder_depth(cams[0], 4.45, 0.45) if with_depth else None
    if with_depth:
        assert (depth < 1.0).mean() > 0.02, "the depth buffer holds geometry"
    common = {E.OPT_LAZY_COLOUR: lazy}
    imgs, rec, rect, clus, st = _run(pkg, dut, splats, cams, {**common, E.OPT_OCCLUSION_CULL: cull, E.OPT_CLUSTER_CULL: 1}, shard, depth)
    imgs0, rec0, rect0, clus0, st0 = _run(pkg, plain, splats, cams, common, shard, depth)
    print(f"{case}: kept {int((rec['visible'] == 1).sum())} of {int((rec0['visible'] == 1).sum())} splats, clusters {clus.tolist()}, culled {st['frames_culled']} "
          f"slab {st['frames_slab']} repaired {st['frames_repaired']} lazy {st['frames_lazy']}")
    assert st0["frames_culled"] == 0 and st0["frames_slab"] == 0 and clus0.tolist() == list(range(6))
    if cull == 2:
        assert st["frames_culled"] >= 1, st
    if cull == 3:
        assert st["frames_slab"] >= len(cams) and st["frames_culled"] == 0, st
    if lazy == 2:        # (front-slab phases shade in K1 whatever the option says)
        assert st0["frames_lazy"] >= len(cams) and (cull == 3 or st["frames_lazy"] >= len(cams)), (st, st0)
    else:
        assert st["frames_lazy"] == 0 and st0["frames_lazy"] == 0
    for k, (a, b) in enumerate(zip(imgs, imgs0)):
        assert a[..., 3].max() > 0.5, "an empty frame checks nothing"
        assert np.array_equal(a, b, equal_nan=True), f"frame {k} differs from the frame with both cull stages off"
    # the last frame against the oracle, in both contexts
    vis0 = _check_against_oracle(oracle, splats, cams[-1], rec0, rect0, clus0, cluster_of, False)
    vis = _check_against_oracle(oracle, splats, cams[-1], rec, rect, clus, cluster_of, True)
    assert vis0.sum() > 50 and vis.sum() > 0
    assert not (vis & ~vis0).any(), "culling ADDED a splat"
    assert np.array_equal(rec[vis], rec0[vis]) and np.array_equal(rect[vis], rect0[vis])
    if cull == 0:
        # nothing is culled by occlusion: the cluster stage alone may drop nothing the per-splat rules keep
        assert np.array_equal(rec, rec0) and np.array_equal(rect, rect0)
        assert set(cluster_of[vis0].tolist()) <= set(clus.tolist())


def test_culled_frames_against_finite_horizons(pkg, oracle, engines):
    """the same checks on a dense cloud whose tile lists are thousands of entries long, so that the second and third frame are culled
    against FINITE horizons (level offsets, tile counts and dilation of the frame decide which cell a splat is compared with)"""
    E = pkg.engine
    dut, plain = engines
    splats = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    splats.alpha[:] = 0.97
    order = oracle.storage_order(splats.P)
    slot = np.empty(splats.n, np.int64)
    slot[order] = np.arange(splats.n)
    # (from 2.2 units the ball fills the frame: the oracle's image has 94 of its 104 tiles opaque, under lists of some ten thousand entries)
    cams = [pkg.camera.make_camera(200, 120, sh_order=3, frame=180 + k, object_matrix=OBJ, step_deg=1.0, distance=2.2) for k in range(3)]
    imgs, rec, rect, clus, st = _run(pkg, dut, splats, cams, {E.OPT_LAZY_COLOUR: 0, E.OPT_OCCLUSION_CULL: 2, E.OPT_CLUSTER_CULL: 1}, None, None)
    imgs0, rec0, rect0, clus0, st0 = _run(pkg, plain, splats, cams, {E.OPT_LAZY_COLOUR: 0}, None, None)
    hz = dut.debug_horizons(st["tiles_x"], st["tiles_y"])[0]
    print(f"kept {int((rec['visible'] == 1).sum())} of {int((rec0['visible'] == 1).sum())} splats, {len(clus)} of {len(clus0)} clusters, culled {st['frames_culled']} "
          f"repaired {st['frames_repaired']}, finite horizons on {int((hz < 3.0e38).sum())} of {hz.size} tiles")
    assert st["frames_culled"] >= 1 and st0["frames_culled"] == 0, (st, st0)
    assert (hz < 3.0e38).sum() >= 10, "no finite horizons: the culled frames compared nothing"
    for k, (a, b) in enumerate(zip(imgs, imgs0)):
        assert np.array_equal(a, b, equal_nan=True), f"frame {k} differs from the frame with both cull stages off"
    vis0 = _check_against_oracle(oracle, splats, cams[-1], rec0, rect0, clus0, slot // 64, False)
    vis = _check_against_oracle(oracle, splats, cams[-1], rec, rect, clus, slot // 64, False)
    assert vis.sum() > 1000 and not (vis & ~vis0).any()
    assert vis.sum() < vis0.sum(), "the far side of the ball lies behind the horizons: the culled frame drops some of it"
    assert np.array_equal(rec[vis], rec0[vis]) and np.array_equal(rect[vis], rect0[vis])
