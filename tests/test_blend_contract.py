"""GPU frames against the blend contract, on scenes aimed at where k_blend and the binning go wrong.

Every frame goes through helpers.check_contract: within the per-pixel bound of the oracle's early-out frame, not
just within 1e-3.  Each scene is rendered by the default context and by a "plain" one that culls and classifies nothing; both
must hold the bound on their own (comparing them with each other cannot see a mistake they share).
"""
import os

import numpy as np
import pytest

from helpers import camera_axes, check_contract, make_splats, stop_scene, unproject, veil_scene, world_sigma

pytestmark = pytest.mark.gpu

LADDER = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


def _label(extra=""):
    return os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0] + extra


@pytest.fixture(scope="module")
def engines(pkg):
    E = pkg.engine
    default = pkg.Engine(0)
    plain = pkg.Engine(0)
    plain.set_option(E.OPT_OCCLUSION_CULL, 0)
    plain.set_option(E.OPT_CLUSTER_CULL, 0)
    plain.set_option(E.OPT_DEBUG_FLAGS, 32)
    yield {"default": default, "plain": plain}
    default.close()
    plain.close()


def _both(engines, oracle, splats, cam, depth=None, origin=(0.0, 0.0, 0.0), cam_o=None):
    """render on both contexts, check both against the contract; returns the default context's frame"""
    out = None
    for name, eng in engines.items():
        eng.upload(splats, origin=origin)
        img = eng.render(cam) if depth is None else eng.render_depth(cam, depth)
        check_contract(img, oracle, splats, cam if cam_o is None else cam_o, origin=origin, depth=depth, label=_label(" " + name))
        out = img if out is None else out
    return out


def _ladder(pkg, cam, n, tile, decoys_in=0, seed=0):
    """n small isotropic splats on one view ray through the centre of tile `tile`, at distinct depths, opacity ~3/n (pixels stay
    unsaturated); decoys_in = S > 0: as many decoys in the other tiles of the tile's S x S super-tile, interleaved in depth"""
    rng = np.random.default_rng(seed + n)
    tx, ty = tile
    D = np.linspace(2.5, 5.0, n)
    X = np.full(n, tx * 16 + 8.0)
    Y = np.full(n, ty * 16 + 8.0)
    op = np.full(n, min(max(3.0 / n, 1.0 / 255.0 + 2e-3), 0.9))
    sig = world_sigma(cam, 1.6, D)
    Cd = rng.uniform(0.0, 1.0, (n, 3))
    if decoys_in:
        S = decoys_in
        sx, sy = (tx // S) * S, (ty // S) * S
        others = [(sx + i, sy + j) for j in range(S) for i in range(S) if (sx + i, sy + j) != (tx, ty)]
        pick = [others[k % len(others)] for k in range(n)]
        Dd = D + 0.5 * (D[1] - D[0] if n > 1 else 0.1)
        X = np.concatenate([X, [p[0] * 16 + 8.0 for p in pick]])
        Y = np.concatenate([Y, [p[1] * 16 + 8.0 for p in pick]])
        D = np.concatenate([D, Dd])
        op = np.concatenate([op, np.full(n, 0.3)])
        sig = np.concatenate([sig, world_sigma(cam, 1.6, Dd)])
        Cd = np.concatenate([Cd, rng.uniform(0.0, 1.0, (n, 3))])
    return make_splats(pkg, unproject(cam, X, Y, D), sig, op, Cd)


def _super_list_length(eng, tile):
    st = eng.stats()
    S = st["super_tile"]
    ls, le, _ = eng.debug_tile_lists()
    k = (tile[1] // S) * st["stiles_x"] + tile[0] // S
    return int(le[k] - ls[k]), S


@pytest.mark.parametrize("n", LADDER)
def test_list_length_ladder(pkg, oracle, engines, n):
    """one tile's list at the boundaries of BL_ROUND, BL_BATCH, the 1024-entry scan step and BL_QCAP"""
    cam = pkg.camera.make_camera(256, 256, sh_order=0, frame=0)
    tile = (5, 6)
    s = _ladder(pkg, cam, n, tile)
    img = _both(engines, oracle, s, cam)
    assert img[tile[1] * 16 + 8, tile[0] * 16 + 8, 3] > 0.5 * (1.0 - np.exp(-3.0)) if n > 1 else img[..., 3].max() > 0.5
    for name, eng in engines.items():
        length, _ = _super_list_length(eng, tile)
        assert length == n, (name, length, n)
        assert eng.stats()["pairs_total"] == n, name


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("n", [65, 257, 1025, 2049, 4097])
def test_list_length_ladder_in_a_shared_super_tile(pkg, oracle, engines, S, n):
    """the ladder deep inside an S x S super-tile whose other tiles hold as many decoys, interleaved in depth: the ladder's hits
    are every other entry of the shared list"""
    E = pkg.engine
    cam = pkg.camera.make_camera(256, 256, sh_order=0, frame=0)
    tile = (S + S // 2 + 1, S + S // 2)
    s = _ladder(pkg, cam, n, tile, decoys_in=S)
    for eng in engines.values():
        eng.set_option(E.OPT_SUPER_TILE, S)
    try:
        _both(engines, oracle, s, cam)
        for name, eng in engines.items():
            length, got = _super_list_length(eng, tile)
            assert got == S and length == 2 * n, (name, got, length, n)
    finally:
        for eng in engines.values():
            eng.set_option(E.OPT_SUPER_TILE, 0)


def test_ladder_in_row_shards_and_frames_in_flight(pkg, oracle, engines):
    E = pkg.engine
    cam = pkg.camera.make_camera(256, 256, sh_order=0, frame=0)
    s = _ladder(pkg, cam, 1025, (5, 6), decoys_in=4)
    eng = engines["default"]
    eng.upload(s)
    full = eng.render(cam)
    check_contract(full, oracle, s, cam, label=_label(" full"))
    for layout in (0, 1):
        eng.set_option(E.OPT_SHARD_LAYOUT, layout)
        eng.set_row_shard(1, 3)
        try:
            band = eng.render(cam)
        finally:
            eng.set_row_shard(0, 1)
            eng.set_option(E.OPT_SHARD_LAYOUT, 0)
        assert np.array_equal(band, pkg.multigpu.extract_band(full, 1, 3, layout)), layout
    for fif in (1, 2):
        eng.set_option(E.OPT_FRAMES_IN_FLIGHT, fif)
        try:
            for _ in range(3):
                check_contract(eng.render(cam), oracle, s, cam, label=_label(f" fif{fif}"))
        finally:
            eng.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)


def _quat_rows(M):
    """(x, y, z, w) of the rotation whose matrix (column-vector maths) is M"""
    w = np.sqrt(max(1.0 + M[0, 0] + M[1, 1] + M[2, 2], 1e-12)) / 2.0
    return np.array([(M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w), (M[1, 0] - M[0, 1]) / (4 * w), w])


def _border_scene(pkg, cam, seed):
    """centres on tile corners, quadrant edges, super-tile edges, pixel centres and pixel edges, the last row and column; sizes
    from sub-pixel to the axis cap; thin splats at 45 degrees across quadrant corners with their 1/255 edge near the boundary"""
    rng = np.random.default_rng(seed)
    W, H = cam.width, cam.height
    xs = sorted({0.0, 0.5, W - 0.5, float(W), W / 2.0} | {float(v) for v in range(0, W + 1, 8)} | {v + 0.5 for v in range(0, W, 16)})
    ys = sorted({0.0, 0.5, H - 0.5, float(H), H / 2.0} | {float(v) for v in range(0, H + 1, 8)} | {v + 0.5 for v in range(0, H, 16)})
    pts = [(x, y) for x in xs for y in ys]
    if len(pts) > 3000:
        pts = [pts[i] for i in rng.choice(len(pts), 3000, replace=False)]
    X = np.array([p[0] for p in pts])
    Y = np.array([p[1] for p in pts])
    n = len(X)
    D = rng.uniform(2.0, 5.0, n)
    s_px = np.exp(rng.uniform(np.log(0.2), np.log(6000.0), n))
    op = np.where(s_px > 50.0, rng.uniform(0.004, 0.03, n), rng.uniform(0.004, 1.0, n))
    sig = world_sigma(cam, s_px, D)
    # thin 45-degree splats across quadrant corners: long axis along (x + y) / sqrt 2 in the image plane
    cx = np.array([v for v in range(8, W, 16)] or [W / 2.0])[: 40]
    cy = np.array([v for v in range(8, H, 16)] or [H / 2.0])[: 40]
    m = min(len(cx), len(cy))
    Xt, Yt = cx[:m].astype(float), cy[:m].astype(float)
    Dt = rng.uniform(2.0, 5.0, m)
    _, R = camera_axes(cam)
    u = (R[0] + R[1]) / np.sqrt(2.0)
    v = (R[1] - R[0]) / np.sqrt(2.0)
    q = _quat_rows(np.stack([u, v, R[2]], axis=1))
    sig_t = np.stack([world_sigma(cam, rng.uniform(4.0, 12.0, m), Dt), world_sigma(cam, 0.3, Dt), world_sigma(cam, 0.3, Dt)], axis=1)
    P = np.concatenate([unproject(cam, X, Y, D), unproject(cam, Xt, Yt, Dt)])
    sig_all = np.concatenate([np.repeat(sig[:, None], 3, axis=1), sig_t])
    op_all = np.concatenate([op, rng.uniform(1.0 / 255.0, 0.02, m)])
    orient = np.concatenate([np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)), np.tile(q, (m, 1))])
    return make_splats(pkg, P, sig_all, op_all, rng.uniform(0.0, 1.0, (n + m, 3)), orient=orient)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (31, 33), (1001, 517)])
def test_borders_and_sizes(pkg, oracle, engines, w, h):
    cam = pkg.camera.make_camera(w, h, sh_order=0, frame=0)
    s = _border_scene(pkg, cam, seed=w * 1000 + h)
    _both(engines, oracle, s, cam)


def test_colours_beyond_one(pkg, oracle, engines):
    """Cd in [-2, 6] without SH; SH order 3 with large coefficients: the bound scales with the colours, and the early-out's residual
    exceeds 2^-14"""
    cam0 = pkg.camera.make_camera(240, 180, sh_order=0, frame=2)
    _both(engines, oracle, veil_scene(pkg, cam0, n=2500, seed=11, colours=(-2.0, 6.0)), cam0)
    s = pkg.scenes.make_scene(20000, seed=12, sh=False)
    s.Cd[:] = pkg.scenes.f16bits(np.random.default_rng(12).uniform(-2.0, 6.0, (s.n, 3)))
    _both(engines, oracle, s, cam0)
    s3 = pkg.scenes.make_scene(20000, seed=13, sh=True)
    rng = np.random.default_rng(13)
    for a in (s3.shx, s3.shy, s3.shz):
        a[:, :15] = pkg.scenes.f16bits(rng.normal(0.0, 2.0, (s3.n, 15)))
    cam3 = pkg.camera.make_camera(240, 180, sh_order=3, frame=2)
    _both(engines, oracle, s3, cam3)


def _kth_zwin_depth(oracle, splats, cam, k):
    """per pixel, the zwin of the k-th (in depth order) visible record whose bbox covers the pixel centre; 1 where there is none"""
    rec = oracle.preprocess(splats, cam)
    perm = oracle.argsort(rec, oracle.storage_order(splats.P))
    W, H = cam.width, cam.height
    depth = np.ones((H, W), np.float32)
    count = np.zeros((H, W), np.int32)
    for r in perm:
        o = rec[r]
        if o["visible"] != 1:
            continue
        i0, i1 = max(int(np.ceil(o["cx"] - o["hx"] - 0.5)), 0), min(int(np.floor(o["cx"] + o["hx"] - 0.5)), W - 1)
        j0, j1 = max(int(np.ceil(o["cy"] - o["hy"] - 0.5)), 0), min(int(np.floor(o["cy"] + o["hy"] - 0.5)), H - 1)
        if i1 < i0 or j1 < j0:
            continue
        c = count[j0:j1 + 1, i0:i1 + 1]
        d = depth[j0:j1 + 1, i0:i1 + 1]
        d[c == k] = o["zwin"]
        c += 1
    return depth


def test_depth_equality_on_an_orbit(pkg, oracle, engines):
    """depth buffers holding exactly the zwin of a pixel's k-th fragment (k = 0, 3, 10), then the same one ulp nearer: LEQUAL, the
    tile-max culling, per-quadrant classification and the 9-bit depth codes all decide at equality; a 4-frame orbit under the
    default policy with the buffer recomputed every frame"""
    s = pkg.scenes.make_scene(6000, seed=21, sh=True)
    for frame in range(4):
        cam = pkg.camera.make_camera(192, 144, sh_order=3, frame=frame)
        for k in (0, 3, 10):
            depth = _kth_zwin_depth(oracle, s, cam, k)
            assert (depth < 1.0).mean() > 0.2
            _both(engines, oracle, s, cam, depth=depth)
            nearer = np.where(depth < 1.0, np.nextafter(depth, np.float32(0.0)), depth).astype(np.float32)
            _both(engines, oracle, s, cam, depth=nearer)


def test_stop_ambiguity_on_hardware(pkg, oracle, engines):
    """the scene of the CPU soundness test whose pixels' T lands next to 2^-14: the ambiguity term is needed and enough"""
    cam = pkg.camera.make_camera(200, 150, sh_order=0, frame=3)
    s = stop_scene(pkg, cam, seed=8)
    _, _, _, st = oracle.render_contract(s, cam)
    assert st["ambiguous"] >= 20
    _both(engines, oracle, s, cam)


def test_c4_through_the_renderer_verbs_is_the_unculled_frame(pkg, oracle):
    """the bench's boundary leg at the headline config: C4 as three registry entries behind the verbs, the default policy, the
    leg's 25 cameras; each frame bit-identical to a direct context that culls nothing and is given the position the shim derived"""
    E = pkg.engine
    L = pkg.load_library()
    splats, cfg = pkg.scenes.make_config("C4")
    W, H, order = cfg["width"], cfg["height"], cfg["sh_order"]
    cuts = [0, splats.n // 3, 2 * (splats.n // 3), splats.n]
    parts = [splats.subset(slice(cuts[k], cuts[k + 1])) for k in range(3)]
    R = pkg.GSplatRenderer(0)
    direct = pkg.Engine(0)
    try:
        R_eng = L.gsplat_renderer_engine(R.h)
        for opt, val in ((E.OPT_OCCLUSION_CULL, 1), (E.OPT_FRONT_SLAB, 1)):
            E._check(L.gsr_set_option(R_eng, opt, val))
        R.setSphericalHarmonicsOrder(order)
        origin0 = np.zeros(3, np.float32)
        ids = [R.registerUpdate(0x1000 + 16 * k, (1, 0, 0, 0), 0, parts[k], splatOrigin=origin0) for k in range(3)]
        for opt, val in ((E.OPT_OCCLUSION_CULL, 0), (E.OPT_CLUSTER_CULL, 0), (E.OPT_DEBUG_FLAGS, 32)):
            direct.set_option(opt, val)
        img = cam = None
        for i in range(25):
            cam = pkg.scenes.config_camera("C4", pkg.camera, W, H, order, i)
            img = R.frame(cam, ids)
            if i == 0:
                assert R.query(R.Q_SPLAT_COUNT) == splats.n
                direct.upload(splats, origin=R.origin())
            cam.cam_pos = R.lastCameraPos()
            want = direct.render(cam)
            assert np.array_equal(img, want), f"frame {i}: {int((img != want).any(axis=2).sum())} pixels differ, max {np.abs(img - want).max()}"
        assert R.query(R.Q_STAGING_COUNT) == 1
        check_contract(img, oracle, splats, cam, origin=R.origin(), label=_label())
    finally:
        direct.close()
        R.close()
