"""Balanced bands on the GPU: a context that renders an EXPLICIT band of tile rows (gsr_set_row_band), the per-tile-row work sums
(GSR_OPT_ROW_WORK, k_row_work) and gsr_multi's layout 2 over the COPY transport on the one GPU.

Everything is held to frames of a single unsharded context, bit for bit: a band is the same tiles with the same lists, so its pixels are
the full frame's rows.  The conditions on the balancer take the row work of the SINGLE context as their reference, never the ranks'."""
import numpy as np
import pytest

from helpers import HipBuffers

pytestmark = pytest.mark.gpu

W, H = 200, 150                      # 10 tile rows; the last one holds 6 pixel rows
BANDS = [(0, 1), (1, 6), (7, 3), (4, 0), (9, 3)]    # ... an empty band and one that reaches beyond the image among them


@pytest.fixture(scope="module")
def cloud(pkg):
    splats = pkg.scenes.make_scene(20000, seed=411, sh=True, log_scale_range=(-4.5, -3.0))
    cam = pkg.camera.make_camera(W, H, sh_order=3, frame=7, distance=2.6)      # (the ball reaches every tile row)
    return splats, cam


@pytest.fixture(scope="module")
def pair(pkg, cloud):
    """the context under test and the unsharded one, both holding the 20 k cloud"""
    dut, full = pkg.Engine(0), pkg.Engine(0)
    dut.upload(cloud[0])
    full.upload(cloud[0])
    yield dut, full
    dut.close()
    full.close()


def _reset(pkg, eng):
    eng.set_row_shard(0, 1)
    eng.set_target_format(pkg.engine.TARGET_RGBA32F)


@pytest.mark.parametrize("fmt", ["RGBA32F", "RGBA8"])
def test_explicit_bands_are_the_full_frames_rows(pkg, cloud, pair, fmt):
    E, mg = pkg.engine, pkg.multigpu
    splats, cam = cloud
    dut, full = pair
    f = getattr(E, "TARGET_" + fmt)
    try:
        dut.set_target_format(f)
        full.set_target_format(f)
        want = full.render(cam)
        assert want[..., 3].max() > 0 and want[: 16].any() and want[144:].any(), "the first and the last tile row hold something"
        hb = HipBuffers()
        try:
            for band in BANDS:
                dut.set_row_band(*band)
                got = dut.render(cam)                                   # host target: padding rows read as zeros
                assert got.shape == (band[1] * 16, W, 4)
                assert np.array_equal(got, mg.extract_band(want, band=band)), f"band {band} ({fmt}, host target)"
                # device target: pixel rows beyond the image are never written
                nbytes = max(got.nbytes, 16)
                canary = np.full(nbytes, 0xCD, np.uint8)
                dev = hb.upload(canary)
                dut.render_to_device(cam, dev)
                dut.synchronize()
                raw = hb.download(dev, (nbytes,), np.uint8)[: got.nbytes].view(got.dtype).reshape(got.shape)
                live = max(min((band[0] + band[1]) * 16, H) - band[0] * 16, 0)
                assert np.array_equal(raw[:live], want[band[0] * 16: band[0] * 16 + live]), f"band {band} ({fmt}, device target)"
                assert (raw[live:].view(np.uint8) == 0xCD).all(), f"band {band}: padding rows of a device target were written"
        finally:
            hb.free()
    finally:
        _reset(pkg, dut)
        _reset(pkg, full)


def test_set_row_band_refusals_and_cancelling(pkg, cloud, pair):
    E = pkg.engine
    splats, cam = cloud
    dut, full = pair
    try:
        for bad in [(-1, 2), (0, -1), (1000, 25), (1025, 0)]:
            with pytest.raises(E.GsrError):
                dut.set_row_band(*bad)
        dut.set_row_band(1024, 0)                                       # the limit itself
        dut.set_row_band(2, 3)
        assert dut.render(cam).shape[0] == 48
        dut.set_row_shard(0, 1)                                         # cancels the band
        assert np.array_equal(dut.render(cam), full.render(cam))
        dut.set_option(E.OPT_SHARD_LAYOUT, 1)
        dut.set_row_shard(1, 2)
        dut.set_row_band(2, 3)                                          # cancels the shard
        assert np.array_equal(dut.render(cam), full.render(cam)[32:80])
    finally:
        dut.set_option(E.OPT_SHARD_LAYOUT, 0)
        _reset(pkg, dut)


def test_depth_aov_and_background_in_a_band(pkg, cloud, pair):
    """inputs are the FULL image (depth buffer, background), outputs the band: each verb's band equals the full verb's rows"""
    splats, cam = cloud
    dut, full = pair
    band = (1, 6)
    rows = slice(16, 112)
    depth = pkg.scenes.sphere_occluder_depth(cam, 2.6, 0.45)            # a sphere in the middle of the ball
    assert 0.02 < (depth < 1.0).mean() < 0.9 and (depth[rows] < 1.0).any(), "the band holds part of the sphere"
    rng = np.random.default_rng(5)
    bg = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    bg[..., :3] *= bg[..., 3:]                                           # premultiplied
    try:
        dut.set_row_band(*band)
        want = full.render_depth(cam, depth)
        assert not np.array_equal(want, full.render(cam)), "the sphere hides something"
        assert np.array_equal(dut.render_depth(cam, depth), want[rows])
        w_img, w_plane = full.render_aov(cam, depth)
        g_img, g_plane = dut.render_aov(cam, depth)
        assert np.array_equal(g_img, w_img[rows]) and np.array_equal(g_plane, w_plane[rows]) and w_plane[rows].any()
        assert np.array_equal(dut.render_over(cam, bg), full.render_over(cam, bg)[rows])
    finally:
        _reset(pkg, dut)


@pytest.fixture(scope="module")
def ball(pkg):
    """a dense opaque ball that fills the frame: its tiles go opaque, so culled frames have finite horizons and front slabs close tiles"""
    splats = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    splats.alpha[:] = 0.97
    cams = [pkg.camera.make_camera(W, H, sh_order=3, frame=180 + k, step_deg=1.0, distance=2.2) for k in range(16)]
    return splats, cams


def test_temporal_regimes_in_a_band_that_changes(pkg, ball):
    """an orbit under GSR_OPT_OCCLUSION_CULL = 2 (every frame culled against the previous frame's horizons), then 3 (front-slab frames):
    the band moves from [2, 8) to [3, 6) mid-orbit -- a new tile geometry, so the horizons of the old band must be dropped -- and every
    frame equals the rows of a context that culls nothing"""
    E = pkg.engine
    splats, cams = ball
    with pkg.Engine(0) as plain, pkg.Engine(0) as dut:
        plain.set_option(E.OPT_OCCLUSION_CULL, 0)
        plain.upload(splats)
        want = [plain.render(c) for c in cams]
        dut.upload(splats)
        for mode in (2, 3):
            dut.set_option(E.OPT_OCCLUSION_CULL, mode)
            dut.stats_reset()
            for k, c in enumerate(cams):
                first, rows = (2, 6) if k < 9 else (3, 3)
                dut.set_row_band(first, rows)
                got = dut.render(c)
                assert np.array_equal(got, want[k][first * 16: (first + rows) * 16]), f"cull mode {mode}, frame {k}, band [{first}, {first + rows})"
            st = dut.stats()
            print(f"cull mode {mode}: culled {st['frames_culled']} slab {st['frames_slab']} repaired {st['frames_repaired']}")
            if mode == 2:
                assert st["frames_culled"] >= 8, st
            else:
                assert st["frames_slab"] >= 8, st


def _row_sums(tw):
    w = tw.astype(np.uint64)
    return np.minimum((w[..., 2] * 32 + w[..., 1] * 8 + (w[..., 0] >> 1)).sum(axis=1), 0xFFFFFFFF)


def test_row_work_is_the_tile_work(pkg, cloud):
    E = pkg.engine
    splats, cam = cloud
    with pkg.Engine(0) as eng:
        eng.upload(splats)
        eng.render(cam)
        with pytest.raises(E.GsrError):
            eng.read_row_work(H)                                        # the option is off
        eng.set_option(E.OPT_ROW_WORK, 1)
        with pytest.raises(E.GsrError):
            eng.read_row_work(H)                                        # no frame has run with it
        for band in (None, (1, 6)):
            if band:
                eng.set_row_band(*band)
            eng.render(cam)
            rows, frame = eng.read_row_work(H)
            tw = eng.debug_tile_work()
            first, n = band if band else (0, 10)
            assert tw.shape[0] == n
            want = np.zeros(10, np.uint64)
            want[first: first + n] = _row_sums(tw)
            print("row work", rows.tolist(), "frame", frame)
            assert want.max() > 0
            assert np.array_equal(rows.astype(np.uint64), want), (rows.tolist(), want.tolist())
            assert frame == eng.stats()["frames"] == (4 if band else 2), "frame_out names the last frame"
            eng.render(pkg.camera.make_camera(W, H, sh_order=3, frame=9, distance=2.6))
            rows2, frame2 = eng.read_row_work(H)
            assert frame2 == frame + 1 and not np.array_equal(rows2, rows)
            with pytest.raises(E.GsrError):
                eng.read_row_work(H + 16)                               # another image's rows
        eng.set_option(E.OPT_ROW_WORK, 0)
        with pytest.raises(E.GsrError):
            eng.read_row_work(H)


# ---- gsr_multi, layout 2 -------------------------------------------------------------------------
TW, TH = 320, 240                    # 15 tile rows


@pytest.fixture(scope="module")
def terrain(pkg, oracle):
    """the landscape under sky, its frames from a single context, the single context's row work of the last frame -- and the check,
    on the CPU, that this camera really leaves layout 1's bands unequal"""
    E = pkg.engine
    splats = pkg.scenes.make_terrain(30000, seed=23)
    moving = [pkg.scenes.terrain_camera(pkg.camera, TW, TH, frame=k) for k in range(24)]
    cams = moving + [moving[-1]] * 12
    rec = oracle.preprocess(splats, cams[-1])
    vis = rec["visible"] == 1
    trow = np.clip(rec["cy"][vis].astype(np.int64) // 16, 0, 14)
    per_row = np.bincount(trow, minlength=15)
    for ranks in (2, 3):
        rpb = -(-15 // ranks)
        per_band = [int(per_row[g * rpb: (g + 1) * rpb].sum()) for g in range(ranks)]
        print(f"{ranks} ranks: splat centres per equal band {per_band}")
        assert max(per_band) > 2 * min(per_band), "the sky leaves the equal split's bands unequal"
    with pkg.Engine(0) as eng:
        eng.set_option(E.OPT_ROW_WORK, 1)
        eng.upload(splats)
        want = []
        for k, c in enumerate(cams):
            if k < 24 or k == len(cams) - 1:
                want.append(eng.render(c))
            else:
                want.append(want[23])
        assert np.array_equal(want[-1], want[23]), "a still camera renders the same frame"
        work, _ = eng.read_row_work(TH)
    assert work.sum() > 0
    return splats, cams, want, work


def _equal_split(tiles_y, count):
    rpb = -(-tiles_y // count)
    return [min(g * rpb, tiles_y) for g in range(count)] + [tiles_y]


def _largest(work, first):
    return max(int(work[first[g]: first[g + 1]].astype(np.uint64).sum()) for g in range(len(first) - 1))


@pytest.mark.parametrize("ranks,period", [(2, None), (3, 8)])
def test_multi_gpu_balanced_bands_match_single_gpu(pkg, terrain, ranks, period):
    """period None: the library's own (one evaluation within these 36 frames, in front of the first still frame); 8 (the A/B hook, read when
    gsr_multi is created): evaluations in front of frames 8, 16, 24 and 32 -- the last one inside the still frames, where nothing may move"""
    import os
    E = pkg.engine
    splats, cams, want, ref_work = terrain
    hb = HipBuffers()
    old = os.environ.get("GSR_BALANCE_PERIOD")
    if period:
        os.environ["GSR_BALANCE_PERIOD"] = str(period)
    try:
        M = pkg.MultiEngine([0] * ranks, E.TRANSPORT_COPY)
    finally:
        if old is None:
            os.environ.pop("GSR_BALANCE_PERIOD", None)
        else:
            os.environ["GSR_BALANCE_PERIOD"] = old
    try:
        with M:
            M.set_option(E.OPT_SHARD_LAYOUT, 2)
            M.upload(splats)
            # the moving frames: device target, no synchronisation in between (frame f's gather overlaps frame f + 1, whose bands may differ)
            outs = [hb.alloc(TW * TH * 16) for _ in range(24)]
            for k in range(24):
                M.render_struct_to_device(E.camera_struct(cams[k]), outs[k], 0)
            M.synchronize()
            for k in range(24):
                assert np.array_equal(hb.download(outs[k], (TH, TW, 4)), want[k]), f"moving frame {k} differs"
            history = []
            for k in range(24, 36):                                      # the camera stands still: host target
                assert np.array_equal(M.render(cams[k]), want[k]), f"still frame {k} differs"
                history.append(M.get_bands()[1])
            first, rebalances = M.get_bands()
            first = first.tolist()
            eq = _equal_split(15, ranks)
            print(f"{ranks} ranks: bands {first} (equal split {eq}), rebalances {history}, largest band {_largest(ref_work, first)} "
                  f"against {_largest(ref_work, eq)}")
            assert first != eq and rebalances >= 1, "(a) the balancer moved the boundaries"
            assert _largest(ref_work, first) <= _largest(ref_work, eq), "(b) the heaviest band is no heavier than the equal split's"
            assert first[0] == 0 and first[-1] == 15 and all(b >= a for a, b in zip(first, first[1:])), "(c) monotone, covering the image"
            assert len(set(history[-8:])) == 1, "(d) a still camera does not rebalance again"
    finally:
        hb.free()


def test_multi_gpu_layouts_0_and_1_beside_layout_2(pkg, terrain):
    """the gather is shared code: interleaved rows and equal bands through the same gsr_multi, before and after a balanced run"""
    E = pkg.engine
    splats, cams, want, _ = terrain
    with pkg.MultiEngine([0] * 3, E.TRANSPORT_COPY) as M:
        M.upload(splats)
        with pytest.raises(E.GsrError):
            M.set_option(E.OPT_SHARD_LAYOUT, 0)
            M.get_bands()                                                # interleaved rows have no boundaries
        for layout in (1, 2, 0, 1, 2):
            M.set_option(E.OPT_SHARD_LAYOUT, layout)
            for k in (0, 5, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 23):
                assert np.array_equal(M.render(cams[k]), want[k]), f"layout {layout}, frame {k}"
            if layout == 1:
                assert M.get_bands()[0].tolist() == _equal_split(15, 3)
