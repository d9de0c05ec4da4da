"""A background on the GPU (gsr_render_over): the frame composited over a colour or an image in the blend kernel's epilogue.

Everything is held, BIT FOR BIT, to gsr_composite_over (the rule on the host, test_background.py) applied to the RGBA32F frame of
gsr_render_depth -- in every target format, image format, on host and device targets with host and device images -- and to itself
across every regime a frame can take (every regime renders the same frame)."""
import ctypes as C

import numpy as np
import pytest

import depth_aov_ref as ref
from helpers import HipBuffers, stop_scene
from test_depth_aov_gpu import ORBIT, REGIMES, RH, RW

W, H = 72, 40                      # the AOV tests' frame: 5 x 3 tiles, the last column and row cut
COLOUR = (0.1, 0.2, 0.3, 0.5)
FMTS = (0, 1, 2)


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _image(w, h, seed=21):
    """float32 [h, w, 4], premultiplied: alpha 1 under one disc, 0.4 under a second, 0 elsewhere; random colour times alpha"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    alpha = np.zeros((h, w), np.float32)
    alpha[(x - 0.30 * w) ** 2 + (y - 0.45 * h) ** 2 < (0.28 * h) ** 2] = 1.0
    alpha[(x - 0.70 * w) ** 2 + (y - 0.55 * h) ** 2 < (0.30 * h) ** 2] = np.float32(0.4)
    rgb = np.random.default_rng(seed).random((h, w, 3)).astype(np.float32) * alpha[..., None]
    return np.concatenate([rgb, alpha[..., None]], -1).astype(np.float32)


def _images(w, h, seed=21):
    """the image in the three formats (each holds ITS OWN nearest values: what the kernel decodes is what the host rule decodes)"""
    f = _image(w, h, seed)
    return {"f32": f, "f16": f.astype(np.float16), "u8": np.clip(np.rint(f.astype(np.float64) * 255), 0, 255).astype(np.uint8)}


def _decoded(img):
    return img.astype(np.float32) / np.float32(255.0) if img.dtype == np.uint8 else img.astype(np.float32)


def _device_bg(E, hb, img):
    b, _ = E.background_struct(img)
    b.image, b.image_is_device = hb.upload(img), 1
    return b


def _stock(pkg):
    return pkg.scenes.make_scene(4000, seed=197, sh=True), ref.tight_camera(pkg, W, H, sh_order=3, frame=1)


def _depth(seed=11, w=W, h=H, z=0.5):
    return np.where(np.random.default_rng(seed).random((h, w)) < 0.5, np.float32(z), np.float32(1.0)).astype(np.float32)


@pytest.fixture(scope="module")
def small(pkg):
    """the stock scene, its camera, a half-covered depth buffer and the RGBA32F frames of gsr_render / gsr_render_depth, once"""
    s, cam = _stock(pkg)
    depth = _depth()
    eng = pkg.Engine(0)
    try:
        eng.upload(s)
        f32 = {None: eng.render(cam).copy(), "d": eng.render_depth(cam, depth).copy()}
    finally:
        eng.close()
    assert not np.array_equal(f32[None], f32["d"])
    return s, cam, depth, f32


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_the_rule_everywhere(pkg, small, fmt):
    """target format x {colour, image in three formats} x {no depth, half-covered depth}, host and device targets, host and device
    images: the bytes of composite_over(the RGBA32F frame, bg, fmt)"""
    E = pkg.engine
    s, cam, depth, f32 = small
    imgs = _images(W, H)
    hb = HipBuffers()
    eng = pkg.Engine(0)
    scanned, opaque = 0, False
    try:
        eng.upload(s)
        eng.set_target_format(fmt)
        dt = E.target_dtype(fmt)
        d_img, d_depth = hb.alloc(W * H * dt.itemsize * 4), hb.upload(depth)
        cs = E.camera_struct(cam)
        for key, d in ((None, None), ("d", depth)):
            plain = E.convert_pixels(f32[key], fmt)
            for name, bg in [("colour", COLOUR)] + list(imgs.items()):
                want = E.composite_over(f32[key], bg, fmt)
                label = (fmt, key, name)
                # teeth: the background shows, and where it is absent or opaque the frame is what the rule says it is
                assert not np.array_equal(_u8(want), _u8(plain)), label
                if name != "colour":
                    B = _decoded(bg)
                    one, none = B[..., 3] == 1, B[..., 3] == 0
                    assert one.sum() > 100 and none.sum() > 100 and ((B[..., 3] > 0.39) & (B[..., 3] < 0.41)).sum() > 100
                    assert np.array_equal(_u8(want[one]), _u8(E.convert_pixels(B, fmt)[one])), label
                    assert np.array_equal(_u8(want[none]), _u8(plain[none])), label
                    assert (f32[key][one][:, 3] > 0).any() and (f32[key][none][:, 3] > 0).any()      # (splats cover both regions)
                # host target, host background
                got = eng.render_over(cam, bg, d)
                tw = eng.debug_tile_work()
                scanned, opaque = max(scanned, int(tw[..., 0].max())), opaque or bool((tw[..., 3] & 1).any())
                assert got.dtype == dt and np.array_equal(_u8(got), _u8(want)), label
                # device target: host background, then (an image) the device copy of it; host target with the device image
                b_host, keep = E.background_struct(bg)
                variants = [b_host] + ([_device_bg(E, hb, bg)] if name != "colour" else [])
                for b in variants:
                    eng.render_over_struct_to_device(cs, b, d_img, d_depth if d is not None else 0)
                    eng.synchronize()
                    assert np.array_equal(_u8(hb.download(d_img, (H, W, 4), dt)), _u8(want)), label + (b.image_is_device,)
                if name != "colour":
                    out = np.empty((H, W, 4), dt)
                    assert eng.L.gsr_render_over(eng.h, C.byref(cs), None if d is None else d.ctypes.data, 0, C.byref(variants[1]), out.ctypes.data, 0) == 0
                    assert np.array_equal(_u8(out), _u8(want)), label
        # a scene that stops (opaque tiles) beside the stock one: the epilogue behind an early exit
        cam2 = pkg.camera.make_camera(W, H, sh_order=0, frame=3)
        eng.upload(stop_scene(pkg, cam2, n=500, seed=8))
        eng.set_target_format(0)
        raw = eng.render(cam2).copy()
        eng.set_target_format(fmt)
        got = eng.render_over(cam2, imgs["f16"])
        tw = eng.debug_tile_work()
        scanned, opaque = max(scanned, int(tw[..., 0].max())), opaque or bool((tw[..., 3] & 1).any())
        assert np.array_equal(_u8(got), _u8(E.composite_over(raw, imgs["f16"], fmt)))
        assert scanned > 1024 and opaque, (scanned, opaque)            # more than one scan step, an opaque stop somewhere
    finally:
        eng.close()
        hb.free()


# ---- regime independence: the AOV tests' 400 k splats at 960 x 540 on their orbit, under their regimes ----
RFMTS = (0, 2)


@pytest.fixture(scope="module")
def big(pkg):
    """the scene, the orbit, a half-covered depth buffer, a background image and the over-frames of an engine without occlusion
    culling (RGBA32F and RGBA8), computed once; they are the rule applied to that engine's plain frames"""
    E = pkg.engine
    s = pkg.scenes.make_scene(400000, seed=197, sh=True, radius=1.0)
    cams = [pkg.camera.make_camera(RW, RH, sh_order=3, frame=i, near=3.3, far=6.2) for i in ORBIT]
    depth = _depth(11, RW, RH, 0.55)
    bg = _images(RW, RH, 5)["f16"]
    eng = pkg.Engine(0)
    want = {}
    try:
        eng.set_option(E.OPT_OCCLUSION_CULL, 0)
        eng.upload(s)
        plain = [eng.render(c).copy() for c in cams]
        plain_d = [eng.render_depth(c, depth).copy() for c in cams[:3]]
        for fmt in RFMTS:
            eng.set_target_format(fmt)
            want[fmt] = ([eng.render_over(c, bg).copy() for c in cams], [eng.render_over(c, bg, depth).copy() for c in cams[:3]])
            for got, p in zip(want[fmt][0] + want[fmt][1], plain + plain_d):
                assert np.array_equal(_u8(got), _u8(E.composite_over(p, bg, fmt)))
    finally:
        eng.close()
    a = plain[0][..., 3]
    assert (a > 0.99).mean() > 0.2 and (a == 0).mean() > 0.05
    assert not np.array_equal(want[0][0][0], plain[0]) and not np.array_equal(want[0][1][0], want[0][0][0])
    return s, cams, depth, bg, want


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_over_frame_does_not_depend_on_the_regime(pkg, big, regime):
    """every regime's over-frame, with and without depth, in RGBA32F and RGBA8, is the frame of an engine without occlusion culling.
    The front-slab row is the one that catches a composited pixel fed back into phase 2."""
    E = pkg.engine
    s, cams, depth, bg, want = big
    opts, stat = REGIMES[regime]
    for fmt in RFMTS:
        eng = pkg.Engine(0)
        try:
            for k, v in opts.items():
                eng.set_option(getattr(E, k), v)
            eng.set_target_format(fmt)
            eng.upload(s)
            for k, (c, w) in enumerate(zip(cams, want[fmt][0])):
                assert np.array_equal(_u8(eng.render_over(c, bg)), _u8(w)), f"{regime}, format {fmt}: frame {k} differs"
            for k, (c, w) in enumerate(zip(cams[:3], want[fmt][1])):
                assert np.array_equal(_u8(eng.render_over(c, bg, depth)), _u8(w)), f"{regime}, format {fmt}: the depth-tested frame {k} differs"
            st = eng.stats()
            print(f"{regime} fmt {fmt}: culled {st['frames_culled']} slab {st['frames_slab']} lazy {st['frames_lazy']} repaired {st['frames_repaired']}")
            if stat:
                assert st[stat] >= 2, (regime, stat, st[stat])
        finally:
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1])
def test_bands_stitch_to_the_over_frame(pkg, big, layout):
    """two row shards: each composites its band over ITS rows of the full image; the bands put back are the unsharded over-frame"""
    E = pkg.engine
    s, cams, depth, bg, want = big
    eng = pkg.Engine(0)
    try:
        eng.set_option(E.OPT_SHARD_LAYOUT, layout)
        eng.upload(s)
        for fmt in RFMTS:
            eng.set_target_format(fmt)
            for c, d, w in ((cams[0], None, want[fmt][0][0]), (cams[4], None, want[fmt][0][4]), (cams[1], depth, want[fmt][1][1])):
                bands = []
                for idx in range(2):
                    eng.set_row_shard(idx, 2)
                    band = eng.render_over(c, bg, d)
                    assert band.shape == (eng.band_rows(RH), RW, 4)
                    bands.append(band)
                eng.set_row_shard(0, 1)
                assert np.array_equal(_u8(pkg.multigpu.stitch_bands_host(np.stack(bands), RH, layout)), _u8(w)), (layout, fmt)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["frames in flight 2", "deferred check"])
def test_a_background_that_changes_every_frame(pkg, small, mode):
    """device targets, a different background every frame -- host images (staged per slot), device images, colours -- queued back to
    back: each frame is the rule for ITS background"""
    E = pkg.engine
    s, cam, depth, f32 = small
    hb = HipBuffers()
    eng = pkg.Engine(0)
    try:
        eng.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
        if mode == "deferred check":
            eng.set_option(E.OPT_DEFERRED_CHECK, 1)
        eng.upload(s)
        cs = E.camera_struct(cam)
        d_depth = hb.upload(depth)
        for fmt in FMTS:
            eng.set_target_format(fmt)
            dt = E.target_dtype(fmt)
            bgs, keep = [], []
            for k in range(8):
                img = _images(W, H, 100 + k)[("f32", "f16", "u8")[k % 3]]
                bgs.append((0.05 * k, 0.1, 0.02 * k, 0.1 * k) if k % 4 == 3 else img)
            targets = [hb.alloc(W * H * dt.itemsize * 4) for _ in bgs]
            for k, (bg, t) in enumerate(zip(bgs, targets)):
                b, arr = E.background_struct(bg)
                if arr is not None and k % 2 == 0:
                    b = _device_bg(E, hb, arr)
                keep.append((b, arr))
                eng.render_over_struct_to_device(cs, b, t, d_depth if k % 2 else 0)
            eng.synchronize()
            for k, (bg, t) in enumerate(zip(bgs, targets)):
                want = E.composite_over(f32["d" if k % 2 else None], bg, fmt)
                assert np.array_equal(_u8(hb.download(t, (H, W, 4), dt)), _u8(want)), (mode, fmt, k)
        assert eng.stats()["frames_truncated"] == 0
    finally:
        eng.close()
        hb.free()


@pytest.mark.gpu
def test_no_leakage_into_the_other_verbs(pkg, small):
    """gsr_render, gsr_render_depth and gsr_render_aov return after over-frames the bytes they returned before; kind 0 and bg = NULL
    are gsr_render_depth"""
    E = pkg.engine
    s, cam, depth, f32 = small
    img = _images(W, H)["u8"]
    eng = pkg.Engine(0)
    try:
        eng.upload(s)
        cs = E.camera_struct(cam)
        for fmt in FMTS:
            eng.set_target_format(fmt)
            before = (eng.render(cam).copy(), eng.render_depth(cam, depth).copy(), eng.render_aov(cam, depth))
            assert np.array_equal(_u8(before[1]), _u8(E.convert_pixels(f32["d"], fmt)))
            for bg, d in ((COLOUR, None), (img, depth), (img, None), (COLOUR, depth)):
                eng.render_over(cam, bg, d)
            after = (eng.render(cam), eng.render_depth(cam, depth), eng.render_aov(cam, depth))
            assert np.array_equal(_u8(before[0]), _u8(after[0])) and np.array_equal(_u8(before[1]), _u8(after[1])), fmt
            assert np.array_equal(_u8(before[2][0]), _u8(after[2][0])) and np.array_equal(_u8(before[2][1]), _u8(after[2][1])), fmt
            # nothing to composite over: the plain verb
            assert np.array_equal(_u8(eng.render_over(cam, None, depth)), _u8(before[1])) and np.array_equal(_u8(eng.render_over(cam, None)), _u8(before[0]))
            out = np.empty_like(before[1])
            assert eng.L.gsr_render_over(eng.h, C.byref(cs), depth.ctypes.data, 0, None, out.ctypes.data, 0) == 0
            assert np.array_equal(_u8(out), _u8(before[1])), fmt
    finally:
        eng.close()


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_the_next_frame_is_right(pkg, small):
    E = pkg.engine
    s, cam, depth, f32 = small
    img = _images(W, H)["f16"]
    hb = HipBuffers()
    eng = pkg.Engine(0)
    try:
        eng.upload(s)
        cs = E.camera_struct(cam)
        L = eng.L
        npx = W * H
        base = hb.alloc(npx * 16 * 3)               # room for a target and an image side by side
        hb.hip.hipMemcpy(C.c_void_p(base + npx * 16), C.c_void_p(img.ctypes.data), C.c_size_t(img.nbytes), 1)
        out = np.empty((H, W, 4), np.float32)

        def over(b, target=None, is_dev=0):
            return L.gsr_render_over(eng.h, C.byref(cs), None, 0, C.byref(b), C.c_void_p(target) if is_dev else out.ctypes.data, is_dev)

        def good():
            b, _ = E.background_struct(img)
            b.image, b.image_is_device = base + npx * 16, 1
            return b

        def check_next():
            assert np.array_equal(_u8(eng.render_over(cam, img)), _u8(E.composite_over(f32[None], img, 0)))

        assert over(good()) == 0 and np.array_equal(_u8(out), _u8(E.composite_over(f32[None], img, 0)))
        cases = []
        b = good(); b.kind = 3; cases.append(("unknown kind", b, None, 0))
        b = good(); b.kind = -1; cases.append(("negative kind", b, None, 0))
        b = good(); b.format = 3; cases.append(("unknown image format", b, None, 0))
        b = good(); b.image = None; cases.append(("NULL image", b, None, 0))
        b = good(); b.image = base + npx * 16 + 4; cases.append(("device image off its 8-byte pixel", b, None, 0))
        b = good(); b.image = base + npx * 16 + 2; cases.append(("device image off its 8-byte pixel by 2", b, None, 0))
        # a device image whose bytes overlap the device target: the same start, the target's last pixel, the image's last pixel
        b = good(); cases.append(("image == target", b, base + npx * 16, 1))
        b = good(); cases.append(("image begins inside the target", b, base + 16, 1))
        b = good(); cases.append(("target begins inside the image", b, base + npx * 16 + npx * 8 - 16, 1))
        for label, b, target, is_dev in cases:
            assert over(b, target, is_dev) == -1, label
            assert b"gsr_render_over" in L.gsr_last_error(), label
            check_next()
        # (touching ranges do not overlap)
        assert over(good(), base, 1) == 0 and over(good(), base + npx * 16 + npx * 8, 1) == 0
        eng.synchronize()
        assert np.array_equal(_u8(hb.download(base, (H, W, 4))), _u8(E.composite_over(f32[None], img, 0)))
        # a misaligned device target, as for every render verb
        assert over(good(), base + 4, 1) == -1
        check_next()
    finally:
        eng.close()
        hb.free()


@pytest.mark.gpu
def test_shim_redraw_over_a_background(pkg):
    """GSplatRenderer::setBackground: a redraw through the nine verbs is the direct call; clearing it restores the plain frame; a
    multi-GPU renderer refuses"""
    E = pkg.engine
    a = pkg.scenes.make_scene(20000, seed=141, sh=True)
    cam = pkg.camera.make_camera(322, 241, sh_order=3, frame=1)
    img = _images(322, 241)["u8"]
    R = pkg.GSplatRenderer(0)
    eng = pkg.Engine(0)
    try:
        rid = R.registerUpdate(0x1, (1, 0, 0, 0), 0, a)
        first = R.frame(cam, [rid]).copy()
        cam.cam_pos = R.lastCameraPos()
        eng.upload(a, origin=a.barycenter())
        assert np.array_equal(eng.render(cam), first)
        for fmt in FMTS:
            assert R.setTargetFormat(fmt) == 0
            eng.set_target_format(fmt)
            for bg in (COLOUR, img):
                b, keep = E.background_struct(bg)
                assert R.setBackground(b) == 0
                out = np.zeros((cam.height, cam.width, 4), E.target_dtype(fmt))
                R.redraw([rid], R.context(cam, out.ctypes.data, False))
                assert np.array_equal(_u8(out), _u8(eng.render_over(cam, bg))), (fmt, type(bg))
                assert np.array_equal(_u8(out), _u8(E.composite_over(first, bg, fmt))), (fmt, type(bg))
            assert R.setBackground(None) == 0
            out = np.zeros((cam.height, cam.width, 4), E.target_dtype(fmt))
            R.redraw([rid], R.context(cam, out.ctypes.data, False))
            assert np.array_equal(_u8(out), _u8(E.convert_pixels(first, fmt))), fmt
    finally:
        R.close()
        eng.close()
    M = pkg.GSplatRenderer([0, 0], E.TRANSPORT_COPY)
    try:
        b, _ = E.background_struct(COLOUR)
        assert M.setBackground(b) == -1 and M.setBackground(None) == 0
    finally:
        M.close()
