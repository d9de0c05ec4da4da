"""Target formats on the GPU (gsr_set_target_format): every frame a context renders into an RGBA16F or RGBA8 target must be,
bit for bit, gsr_convert_pixels of the f32 frame of a context that was never given a format -- whatever path produced it:
plain, depth-tested, lazy colour, front-slab, sharded, gathered by gsr_multi, banded host copies, the wire overlay, the shim.
The expected image is always the conversion of an f32 frame, never the packed output of another path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import HipBuffers, load_golden

pytestmark = pytest.mark.gpu

F16, U8 = 1, 2
PACKED = (F16, U8)
BPP = {0: 16, 1: 8, 2: 4}


def _bits(a):
    """an image as integers: the comparison is on bits (float16 NaN payloads and signed zeros included)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _same(got, f32_frame, fmt, pkg):
    want = pkg.engine.convert_pixels(f32_frame, fmt)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _device_frame(pkg, hb, eng, cam, fmt, depth=None):
    """a frame rendered into a DEVICE target (cleared first: band padding is never written there)"""
    rows = eng.band_rows(cam.height)
    nbytes = rows * cam.width * BPP[fmt]
    ptr = hb.upload(np.zeros(nbytes, np.uint8))
    if depth is None:
        eng.render_to_device(cam, ptr)
    else:
        eng.render_struct_depth_to_device(pkg.engine.camera_struct(cam), hb.upload(depth), ptr)
    eng.synchronize()
    return hb.download(ptr, (rows, cam.width, 4), pkg.engine.target_dtype(fmt))


@pytest.fixture()
def plain(pkg):
    """the context that is never given a format"""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture()
def eng(pkg):
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("order", [0, 3])
def test_plain_frames_host_and_device(pkg, plain, eng, order):
    """SH 0 and SH 3, a framebuffer whose width and height are no multiples of 16, host and device targets, both packed formats"""
    splats = pkg.scenes.make_scene(60000, seed=301, sh=order > 0)
    hb = HipBuffers()
    try:
        for e in (plain, eng):
            e.upload(splats)
        for (w, h) in ((333, 217), (640, 360)):
            for frame in (0, 7):
                cam = pkg.camera.make_camera(w, h, sh_order=order, frame=frame)
                ref = plain.render(cam)
                assert ref.dtype == np.float32 and np.count_nonzero(ref) > 0
                for fmt in PACKED:
                    eng.set_target_format(fmt)
                    assert eng.L.gsr_get_target_format(eng.h) == fmt
                    got = eng.render(cam)
                    assert got.dtype == pkg.engine.target_dtype(fmt)
                    assert _same(got, ref, fmt, pkg), f"{w}x{h} frame {frame} format {fmt}: host target differs"
                    assert _same(_device_frame(pkg, hb, eng, cam, fmt), ref, fmt, pkg), f"{w}x{h} frame {frame} format {fmt}: device target differs"
    finally:
        hb.free()


def test_depth_tested_frames(pkg, oracle, plain, eng):
    """gsr_render_depth with an occluder through the middle of the cloud (and a cleared buffer: the guarded plain kernel)"""
    splats = pkg.scenes.make_scene(60000, seed=95, sh=True)
    cam = pkg.camera.make_camera(481, 303, sh_order=3, frame=4)
    rec = oracle.preprocess(splats, cam)
    zmid = float(np.median(rec["zwin"][rec["visible"] == 1]))
    yy, xx = np.mgrid[0:cam.height, 0:cam.width]
    depth = np.full((cam.height, cam.width), 1.0, np.float32)
    depth[(xx // 40 + yy // 40) % 2 == 0] = zmid
    depth[:20] = 0.0
    far = np.ones_like(depth)
    hb = HipBuffers()
    try:
        for e in (plain, eng):
            e.upload(splats)
        for d in (depth, far, depth):
            ref = plain.render_depth(cam, d)
            for fmt in PACKED:
                eng.set_target_format(fmt)
                assert _same(eng.render_depth(cam, d), ref, fmt, pkg), f"format {fmt}: depth-tested host frame differs"
                assert _same(_device_frame(pkg, hb, eng, cam, fmt, d), ref, fmt, pkg), f"format {fmt}: depth-tested device frame differs"
        assert not np.array_equal(plain.render_depth(cam, depth), plain.render(cam))
    finally:
        hb.free()


def test_lazy_colour_frames(pkg, plain, eng):
    """GSR_OPT_LAZY_COLOUR = 2: the plain kernel and the on-demand fallback (k_blend_lazy) share the store"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(200000, seed=303, sh=True)
    for e in (plain, eng):
        e.upload(splats)
    eng.set_option(E.OPT_LAZY_COLOUR, 2)
    for fmt in PACKED:
        eng.set_target_format(fmt)
        for flags in (0, 8):                      # 8 = no ahead-of-time pass: every tile takes the fallback kernel
            eng.set_option(E.OPT_DEBUG_FLAGS, flags)
            for frame in (0, 1, 30):
                cam = pkg.camera.make_camera(700, 413, sh_order=3, frame=frame)
                assert _same(eng.render(cam), plain.render(cam), fmt, pkg), f"format {fmt} flags {flags} frame {frame}"
    assert eng.stats()["frames_lazy"] > 0


@pytest.mark.parametrize("fmt", PACKED)
def test_front_slab_frames_and_the_default_culling_policy(pkg, plain, fmt):
    """GSR_OPT_OCCLUSION_CULL = 3 (every frame in two phases; phase 2 continues from f32 pixels kept beside the packed target) with a
    device target, then an orbit under the default policy (temporal culling, repairs, front-slab frames where a horizon broke)"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(400000, seed=197, sh=True, radius=1.0)
    w, h = 950, 531
    cams = [pkg.camera.make_camera(w, h, sh_order=3, frame=i) for i in (0, 1, 40, 41, 77)]
    cams += [pkg.camera.make_camera(w, h, sh_order=3, frame=43, distance=d) for d in (0.5, 2.2, 9.0)]
    plain.upload(splats)
    plain.set_option(E.OPT_OCCLUSION_CULL, 0)
    want = [plain.render(c).copy() for c in cams]
    hb = HipBuffers()
    slab, dflt = pkg.Engine(0), pkg.Engine(0)
    try:
        slab.set_target_format(fmt)
        slab.set_option(E.OPT_OCCLUSION_CULL, 3)
        slab.upload(splats)
        for k, (c, ref) in enumerate(zip(cams, want)):
            assert _same(_device_frame(pkg, hb, slab, c, fmt), ref, fmt, pkg), f"front-slab frame {k} (device target) differs"
            assert _same(slab.render(c), ref, fmt, pkg), f"front-slab frame {k} (host target) differs"
        st = slab.stats()
        assert st["frames_slab"] >= 2 * len(cams) and st["frames_culled"] == 0, st
        dflt.set_target_format(fmt)
        dflt.upload(splats)
        orbit = [pkg.camera.make_camera(w, h, sh_order=3, frame=i) for i in (0, 1, 2, 3, 4, 5, 50, 51, 52, 110, 111, 112)]
        for k, c in enumerate(orbit):
            assert _same(_device_frame(pkg, hb, dflt, c, fmt), plain.render(c), fmt, pkg), f"default policy: frame {k} differs"
        print("default policy:", {q: dflt.stats()[q] for q in ("frames_culled", "frames_slab", "frames_repaired", "frames_jumped")})
    finally:
        slab.close(); dflt.close(); hb.free()


@pytest.mark.parametrize("layout", [0, 1])
def test_row_shards_stitch_to_the_unsharded_frame(pkg, plain, eng, layout):
    """band images are in the target format (host bands: padding reads as zeros); gsr_stitch_bands moves pixels of that size"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(40000, seed=31, sh=True)
    splats.scale[:300] = pkg.scenes.f16bits(np.random.default_rng(3).uniform(0.2, 2.0, size=(300, 3)))
    cam = pkg.camera.make_camera(301, 203, sh_order=3, frame=2)
    for e in (plain, eng):
        e.upload(splats)
    full = plain.render(cam)
    eng.set_option(E.OPT_SHARD_LAYOUT, layout)
    hb = HipBuffers()
    try:
        for fmt in PACKED:
            eng.set_target_format(fmt)
            want = E.convert_pixels(full, fmt)
            for count in (2, 3, 8):
                bands, dev_bands = [], []
                for idx in range(count):
                    eng.set_row_shard(idx, count)
                    band = eng.render(cam)
                    assert band.shape[0] == eng.band_rows(cam.height) and band.dtype == want.dtype
                    bands.append(band)
                    dev_bands.append(_device_frame(pkg, hb, eng, cam, fmt))
                    assert np.array_equal(_bits(band), _bits(dev_bands[-1]))      # (the device target was cleared: same zeros in the padding)
                eng.set_row_shard(0, 1)
                out = pkg.multigpu.stitch_bands_host(np.stack(bands), cam.height, layout)
                assert np.array_equal(_bits(out), _bits(want)), f"layout {layout}, format {fmt}, {count} shards: stitched image differs"
                # the stitch kernel on the gathered device bands
                g = hb.upload(np.stack(dev_bands))
                o = hb.upload(np.zeros(cam.height * cam.width * BPP[fmt], np.uint8))
                eng.stitch_bands(g, count, cam.width, cam.height, o)
                eng.synchronize()
                got = hb.download(o, (cam.height, cam.width, 4), want.dtype)
                assert np.array_equal(_bits(got), _bits(want)), f"layout {layout}, format {fmt}, {count} shards: gsr_stitch_bands differs"
    finally:
        eng.set_row_shard(0, 1)
        hb.free()


@pytest.mark.parametrize("ranks,layout", [(2, 0), (3, 1), (3, 0), (2, 1)])
def test_multi_gpu_copy_transport(pkg, plain, ranks, layout):
    """gsr_multi over the COPY transport on the one GPU: host frames, and device frames queued back to back"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(60000, seed=131, sh=True)
    w, h = 500, 333
    cams = [pkg.camera.make_camera(w, h, sh_order=3, frame=20 + f) for f in range(5)]
    plain.upload(splats)
    want = [plain.render(c).copy() for c in cams]
    hb = HipBuffers()
    try:
        with pkg.MultiEngine([0] * ranks, E.TRANSPORT_COPY) as M:
            M.set_option(E.OPT_SHARD_LAYOUT, layout)
            M.upload(splats)
            for fmt in PACKED + (0,):
                M.set_target_format(fmt)
                for k, c in enumerate(cams[:2]):
                    assert _same(M.render(c), want[k], fmt, pkg), f"{ranks} ranks layout {layout} format {fmt}: host frame {k} differs"
                outs = [hb.upload(np.zeros(w * h * BPP[fmt], np.uint8)) for _ in cams]
                for c, o in zip(cams, outs):
                    M.render_struct_to_device(E.camera_struct(c), o, 0)          # (no synchronisation in between)
                M.synchronize()
                for k, o in enumerate(outs):
                    got = hb.download(o, (h, w, 4), E.target_dtype(fmt))
                    assert _same(got, want[k], fmt, pkg), f"{ranks} ranks layout {layout} format {fmt}: device frame {k} differs"
    finally:
        hb.free()


def test_banded_host_copies(pkg, plain, eng):
    """host-target frames with the band-by-band copy-back active (4 bands by default: a height of at least 16 tile rows)"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(250000, seed=5, sh=True)
    for e in (plain, eng):
        e.upload(splats)
    for (w, h) in ((1001, 517), (640, 1100)):
        assert (h + 15) // 16 >= 4 * 4
        cams = [pkg.camera.make_camera(w, h, sh_order=3, frame=i) for i in (0, 1, 2, 40)]
        sphere = pkg.scenes.sphere_occluder_depth(cams[0], 3.42, 0.645)
        for mode in ((1, 1), (3, 2), (0, 0)):
            eng.set_option(E.OPT_OCCLUSION_CULL, mode[0]); eng.set_option(E.OPT_FRONT_SLAB, mode[1])
            for fmt in PACKED:
                eng.set_target_format(fmt)
                for k, c in enumerate(cams):
                    assert _same(eng.render(c), plain.render(c), fmt, pkg), f"{w}x{h} mode {mode} format {fmt} frame {k}"
                assert _same(eng.render_depth(cams[0], sphere), plain.render_depth(cams[0], sphere), fmt, pkg), f"{w}x{h} mode {mode} format {fmt} depth"


def test_wire_overlay(pkg, plain, eng):
    """gsr_render_wire writes (Cd, 1) / 0 in the target format (RGBA16F: Cd's own half bits); gsr_render_wire_over writes the covered
    pixels into a frame of the same format, host and device"""
    E = pkg.engine
    d, s, c = load_golden("w1_wire")
    for e in (plain, eng):
        e.upload(s)
    wire = plain.render_wire(c)
    beauty = plain.render(c)
    covered = wire[..., 3] > 0
    assert covered.any() and (~covered).any()
    hb = HipBuffers()
    try:
        for fmt in PACKED:
            eng.set_target_format(fmt)
            got = eng.render_wire(c)
            assert _same(got, wire, fmt, pkg), f"format {fmt}: wire overlay differs"
            ptr = hb.upload(np.full(c.height * c.width * BPP[fmt], 0xff, np.uint8))
            cs = E.camera_struct(c)
            assert eng.L.gsr_render_wire(eng.h, C.byref(cs), C.c_void_p(ptr), 1) == 0
            assert _same(hb.download(ptr, got.shape, got.dtype), wire, fmt, pkg), f"format {fmt}: wire overlay (device target) differs"
            under = eng.render(c)
            assert _same(under, beauty, fmt, pkg)
            want = E.convert_pixels(np.where(covered[..., None], wire, beauty), fmt)
            both = eng.render_wire_over(c, under)
            assert np.array_equal(_bits(both), _bits(want)), f"format {fmt}: wire-over (host) differs"
            ptr = hb.upload(under)
            eng.render_wire_over_device(c, ptr)
            assert np.array_equal(_bits(hb.download(ptr, under.shape, under.dtype)), _bits(want)), f"format {fmt}: wire-over (device) differs"
        eng.set_target_format(F16)      # RGBA16F carries Cd unchanged
        w16 = eng.render_wire(c)
        assert np.array_equal(w16[covered][:, :3].astype(np.float32), wire[covered][:, :3])
    finally:
        hb.free()


def test_switching_formats_between_frames(pkg, plain, eng):
    """one context, the format switched back and forth (host and device targets, a front-slab frame in between): every frame is right
    and the last f32 frame is the first one, bit for bit"""
    E = pkg.engine
    splats = pkg.scenes.make_scene(120000, seed=307, sh=True)
    for e in (plain, eng):
        e.upload(splats)
    cams = [pkg.camera.make_camera(515, 389, sh_order=3, frame=i) for i in range(4)]
    first = eng.render(cams[0]).copy()
    assert first.dtype == np.float32 and np.array_equal(first, plain.render(cams[0]))
    hb = HipBuffers()
    try:
        for k, fmt in enumerate((F16, U8, 0, U8, F16, F16, 0, F16, U8, 0)):
            eng.set_target_format(fmt)
            eng.set_option(E.OPT_OCCLUSION_CULL, 3 if k % 3 == 1 else 1)
            c = cams[k % len(cams)]
            ref = plain.render(c)
            assert _same(eng.render(c), ref, fmt, pkg), f"step {k} format {fmt}: host frame differs"
            assert _same(_device_frame(pkg, hb, eng, c, fmt), ref, fmt, pkg), f"step {k} format {fmt}: device frame differs"
        eng.set_option(E.OPT_OCCLUSION_CULL, 1)
        last = eng.render(cams[0])
        assert last.dtype == np.float32 and np.array_equal(_bits(last), _bits(first))
    finally:
        hb.free()


def test_misaligned_device_target_is_rejected(pkg, eng):
    E = pkg.engine
    splats = pkg.scenes.make_scene(2000, seed=311, sh=False)
    eng.upload(splats)
    cam = pkg.camera.make_camera(64, 48, sh_order=0, frame=0)
    cs = E.camera_struct(cam)
    hb = HipBuffers()
    try:
        base = hb.alloc(64 * 48 * 16 + 64)
        for fmt, off in ((0, 4), (0, 8), (F16, 4), (F16, 2), (U8, 2), (U8, 1)):
            eng.set_target_format(fmt)
            assert eng.L.gsr_render(eng.h, C.byref(cs), C.c_void_p(base + off), 1) == -1, (fmt, off)
            assert eng.L.gsr_render_wire(eng.h, C.byref(cs), C.c_void_p(base + off), 1) == -1, (fmt, off)
        for fmt, off in ((F16, 8), (U8, 4), (0, 16)):       # aligned to the pixel: accepted
            eng.set_target_format(fmt)
            assert eng.L.gsr_render(eng.h, C.byref(cs), C.c_void_p(base + off), 1) == 0, (fmt, off)
        eng.synchronize()
        assert eng.L.gsr_set_target_format(eng.h, 3) == -1 and eng.L.gsr_get_target_format(eng.h) == 0
    finally:
        hb.free()


def test_shim_redraw_in_rgba16f(pkg, plain):
    """GSplatRenderer::setTargetFormat(1): redraw() hands back the pixels the direct door gives -- one GPU and gsr_multi behind the verbs"""
    E = pkg.engine
    a = pkg.scenes.make_scene(20000, seed=141, sh=True)
    cam = pkg.camera.make_camera(322, 241, sh_order=3, frame=1)
    for dev in (0, [0, 0]):
        R = pkg.GSplatRenderer(dev, E.TRANSPORT_COPY) if isinstance(dev, list) else pkg.GSplatRenderer(dev)
        try:
            rid = R.registerUpdate(0x1, (1, 0, 0, 0), 0, a)
            first = R.frame(cam, [rid]).copy()
            assert first.dtype == np.float32
            # the direct door, with the camera position the shim derived and the origin it staged with
            cam.cam_pos = R.lastCameraPos()
            plain.upload(a, origin=a.barycenter())
            ref32 = plain.render(cam)
            assert np.array_equal(ref32, first)
            for fmt in (F16, U8, 0):
                assert R.setTargetFormat(fmt) == 0 and R.targetFormat() == fmt
                out = np.zeros((cam.height, cam.width, 4), E.target_dtype(fmt))
                R.redraw([rid], R.context(cam, out.ctypes.data, False))
                assert _same(out, ref32, fmt, pkg), f"shim on {dev}, format {fmt}"
            assert R.setTargetFormat(5) == -1 and R.targetFormat() == 0
        finally:
            R.close()


def test_fuzz_with_formats(pkg):
    """tools/fuzz_parity.py --formats, a short run: fresh contexts, then one long-lived context whose format flips between iterations"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for args in (["24", "21", "--formats"], ["16", "22", "0", "2", "--formats"], ["8", "23", "0", "3", "--formats"]):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py")] + args, capture_output=True, text=True, timeout=900, cwd=root)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
        assert "frames bit-identical" in res.stdout and "'format': " in res.stdout
