"""The depth AOV on the GPU (gsr_render_aov): per pixel {zsum, cov} = the alpha-weighted sum of window depths over exactly the
fragments the colour frame composites, and the coverage 1 - T.

The plane is held to the oracle's contract pass (depth_aov_ref.py: zwin in the records' red channel), the colour beside it to the
frame without the AOV bit for bit, and the plane to itself across every regime a frame can take (every regime
renders the same frame)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import depth_aov_ref as ref
from helpers import HipBuffers, check_contract, make_splats, stop_scene, unproject, veil_scene, world_sigma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 72, 40                      # neither a multiple of the 16-pixel tile: 5 x 3 tiles, the last column and row cut


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(pkg, name):
    if name == "stock":
        cam = ref.tight_camera(pkg, W, H, sh_order=3, frame=1)
        return pkg.scenes.make_scene(4000, seed=197, sh=True), cam
    cam = pkg.camera.make_camera(W, H, sh_order=0, frame=3)      # (the stock planes: stop_scene stands 2 to 3.5 in front of the camera)
    return (veil_scene(pkg, cam, n=3000, seed=5), cam) if name == "veil" else (stop_scene(pkg, cam, n=500, seed=8), cam)


def _check_plane(plane, want, label):
    """|zsum - eo.r| <= bound.r and |cov - eo.a| <= bound.a on every pixel; prints the worst err / bound like check_contract"""
    zsum, cov, bz, bc = want
    assert plane.shape == zsum.shape + (2,) and plane.dtype == np.float32 and np.isfinite(plane).all()
    worst = []
    for name, got, eo, bound in (("zsum", plane[..., 0], zsum, bz), ("cov", plane[..., 1], cov, bc)):
        err = np.abs(got.astype(np.float64) - eo.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        worst.append(float(ratio.max(initial=0.0)))
        covered = cov > 0
        print(f"AOV CONTRACT {label} {name}: worst err/bound = {worst[-1]:.4f}, max|err| = {float(err.max()):.3e}, "
              f"median bound = {float(np.median(bound[covered])) if covered.any() else 0.0:.3e}")
        if not worst[-1] <= 1.0:
            y, x = np.unravel_index(int(ratio.argmax()), ratio.shape)
            raise AssertionError(f"{label}: {int((err > bound).sum())} pixels of {name} outside the contract bound; worst at (x, y) = ({x}, {y}): "
                                 f"got {got[y, x]!r}, eo {eo[y, x]!r}, |err| = {err[y, x]:.4e}, bound = {bound[y, x]:.4e}")
    assert (plane[cov == 0] == 0).all()            # nothing covers the pixel: {0, 0}
    return max(worst)


@pytest.mark.gpu
def test_plane_meets_the_oracle_contract(pkg, oracle, engine):
    """three scenes at 72 x 40, each with and without a random half-covered depth buffer; the tiles' bookkeeping shows that the
    paths the kernel can take were taken: more than one scan step, more than one batch of gathered records, an opaque stop"""
    scanned = gathered = 0
    opaque = False
    for name in ("stock", "veil", "stop"):
        s, cam = _scene(pkg, name)
        rec, perm = ref.records(oracle, s, cam)
        z = rec["zwin"][rec["visible"] == 1]
        if name == "stock":
            assert z.min() <= 0.2 and z.max() >= 0.8, (z.min(), z.max())          # (the planes spread the depths: the reference has teeth)
        # half of the pixels covered at a depth in the middle of the cloud's: fragments on either side of it everywhere
        depth = np.where(np.random.default_rng(11).random((H, W)) < 0.5, np.float32(np.median(z)), np.float32(1.0)).astype(np.float32)
        engine.upload(s)
        for d in (None, depth):
            label = f"{name}{' + depth' if d is not None else ''}"
            rgba, plane = engine.render_aov(cam, d)
            tw = engine.debug_tile_work()
            scanned, gathered, opaque = max(scanned, int(tw[..., 0].max())), max(gathered, int(tw[..., 1].max())), opaque or bool((tw[..., 3] & 1).any())
            want = ref.reference(oracle, rec, perm, cam, depth=d)
            _check_plane(plane, want, label)
            check_contract(rgba, oracle, s, cam, depth=d, label=label)
            if d is not None:
                assert not np.array_equal(plane, engine.render_aov(cam)[1])            # (the depth buffer really cut fragments)
    assert scanned > 1024 and gathered > 256 and opaque, (scanned, gathered, opaque)


@pytest.mark.gpu
def test_one_splat_resolves_to_its_window_depth(pkg, oracle, engine):
    """one splat alone: zsum / cov within 2 ulp of its zwin.  Held where the fragment's weight w is at least 1/2: there T = 1 - w and
    cov = 1 - T are exact (Sterbenz), so zsum / cov = fl(fl(w * zwin) / w) -- two roundings, at most 2 ulp.  (Below 1/2, T = fl(1 - w)
    rounds at 2^-25 ABSOLUTE, which is many ulp of a small w: no such bound exists there.)"""
    cam = ref.tight_camera(pkg, W, H, sh_order=0, frame=0)
    P = unproject(cam, [W * 0.5 + 3.0], [H * 0.5 - 2.0], [4.3])
    s = make_splats(pkg, P, world_sigma(cam, [6.0], [4.3]), [0.9], [[0.2, 0.5, 0.8]])
    rec, perm = ref.records(oracle, s, cam)
    assert rec["visible"][0] == 1
    zwin = np.float32(rec["zwin"][0])
    assert 0.2 < zwin < 0.8
    engine.upload(s)
    rgba, plane = engine.render_aov(cam)
    _check_plane(plane, ref.reference(oracle, rec, perm, cam), "one splat")
    heavy = plane[..., 1] >= 0.5
    assert heavy.sum() >= 8 and (plane[..., 1] > 0).sum() > heavy.sum()
    q = plane[..., 0][heavy] / plane[..., 1][heavy]
    assert q.dtype == np.float32
    ulps = np.abs(q.astype(np.float64) - float(zwin)) / float(np.spacing(zwin))
    print(f"one splat: zwin = {zwin!r}, {int(heavy.sum())} pixels with cov >= 1/2, worst |zsum / cov - zwin| = {ulps.max():.2f} ulp")
    assert ulps.max() <= 2.0
    assert np.array_equal(pkg.engine.resolve_depth(plane, 0.5)[heavy], np.minimum(q, np.float32(1.0)))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_colour_is_untouched_and_cov_is_the_f32_alpha(pkg, fmt):
    """in every target format the image of gsr_render_aov is gsr_render's / gsr_render_depth's bit for bit, and the plane's cov the
    RGBA32F frame's alpha -- the plane itself does not depend on the format -- on host and on device targets"""
    E = pkg.engine
    s, cam = _scene(pkg, "stock")
    depth = np.where(np.random.default_rng(3).random((H, W)) < 0.5, np.float32(0.5), np.float32(1.0)).astype(np.float32)
    hb = HipBuffers()
    eng = pkg.Engine(0)
    try:
        eng.upload(s)
        f32 = {None: eng.render(cam).copy(), "d": eng.render_depth(cam, depth).copy()}
        planes = {None: eng.render_aov(cam)[1].copy(), "d": eng.render_aov(cam, depth)[1].copy()}
        eng.set_target_format(fmt)
        bpp = E.target_dtype(fmt).itemsize * 4
        d_img, d_plane, d_depth = hb.alloc(W * H * bpp), hb.alloc(W * H * 8), hb.upload(depth)
        cs = E.camera_struct(cam)
        for key, d in ((None, None), ("d", depth)):
            want = eng.render(cam) if d is None else eng.render_depth(cam, d)
            rgba, plane = eng.render_aov(cam, d)
            assert rgba.dtype == want.dtype and np.array_equal(rgba.view(np.uint8), want.view(np.uint8)), (fmt, key)
            assert np.array_equal(_bits(plane[..., 1]), _bits(f32[key][..., 3])), (fmt, key)
            assert np.array_equal(_bits(plane), _bits(planes[key])), (fmt, key)
            assert (plane[..., 1] > 0).mean() > 0.2
            # device targets (aov = 0 or no plane: the plain frame)
            eng.render_aov_struct_to_device(cs, d_img, d_plane, d_depth if d is not None else 0)
            eng.synchronize()
            assert np.array_equal(hb.download(d_img, (H, W, 4), want.dtype).view(np.uint8), want.view(np.uint8)), (fmt, key)
            assert np.array_equal(_bits(hb.download(d_plane, (H, W, 2))), _bits(plane)), (fmt, key)
            eng.render_aov_struct_to_device(cs, d_img, 0, d_depth if d is not None else 0)
            eng.synchronize()
            assert np.array_equal(hb.download(d_img, (H, W, 4), want.dtype).view(np.uint8), want.view(np.uint8)), (fmt, key)
        # the verb's own argument checks: an unknown AOV, a misaligned device plane
        L = eng.L
        import ctypes as C
        assert L.gsr_render_aov(eng.h, C.byref(cs), None, 0, C.c_void_p(d_img), 1, 7, C.c_void_p(d_plane)) == -1
        assert L.gsr_render_aov(eng.h, C.byref(cs), None, 0, C.c_void_p(d_img), 1, E.AOV_DEPTH, C.c_void_p(d_plane + 4)) == -1
    finally:
        eng.close()
        hb.free()


# ---- regime independence: 400 k splats at 960 x 540 (the size at which the regimes engage) on an orbit with one jump ----
RW, RH = 960, 540
ORBIT = (0, 1, 2, 3, 50, 51)


@pytest.fixture(scope="module")
def big(pkg):
    """the scene, the orbit, a half-covered depth buffer and the planes of an engine without occlusion culling, computed once"""
    E = pkg.engine
    s = pkg.scenes.make_scene(400000, seed=197, sh=True, radius=1.0)
    cams = [pkg.camera.make_camera(RW, RH, sh_order=3, frame=i, near=3.3, far=6.2) for i in ORBIT]
    depth = np.where(np.random.default_rng(11).random((RH, RW)) < 0.5, np.float32(0.55), np.float32(1.0)).astype(np.float32)
    eng = pkg.Engine(0)
    try:
        eng.set_option(E.OPT_OCCLUSION_CULL, 0)
        eng.upload(s)
        want = [eng.render_aov(c) for c in cams]
        want_d = [eng.render_aov(c, depth) for c in cams[:3]]
        # (the colour beside the plane is the frame without it)
        assert np.array_equal(want[0][0], eng.render(cams[0])) and np.array_equal(want_d[0][0], eng.render_depth(cams[0], depth))
    finally:
        eng.close()
    cov = want[0][1][..., 1]
    assert (cov > 0.99).mean() > 0.2 and (cov == 0).mean() > 0.05
    assert not np.array_equal(want[0][1], want_d[0][1])
    return s, cams, depth, want, want_d


REGIMES = {
    "cull 2": ({"OPT_OCCLUSION_CULL": 2}, "frames_culled"),
    "cull 3 (front slab)": ({"OPT_OCCLUSION_CULL": 3}, "frames_slab"),
    "cluster cull off": ({"OPT_CLUSTER_CULL": 0}, None),
    "lazy 0": ({"OPT_LAZY_COLOUR": 0}, None),
    "lazy 2": ({"OPT_LAZY_COLOUR": 2, "OPT_OCCLUSION_CULL": 0}, "frames_lazy"),
    "super-tile 1": ({"OPT_SUPER_TILE": 1}, None),
    "super-tile 4": ({"OPT_SUPER_TILE": 4}, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_plane_does_not_depend_on_the_regime(pkg, big, regime):
    E = pkg.engine
    s, cams, depth, want, want_d = big
    opts, stat = REGIMES[regime]
    eng = pkg.Engine(0)
    try:
        for k, v in opts.items():
            eng.set_option(getattr(E, k), v)
        eng.upload(s)
        for k, (c, (rgba, plane)) in enumerate(zip(cams, want)):
            got = eng.render_aov(c)
            assert np.array_equal(_bits(got[1]), _bits(plane)), f"{regime}: the plane of frame {k} differs"
            assert np.array_equal(_bits(got[0]), _bits(rgba)), f"{regime}: the image of frame {k} differs"
        for k, (c, (rgba, plane)) in enumerate(zip(cams[:3], want_d)):
            got = eng.render_aov(c, depth)
            assert np.array_equal(_bits(got[1]), _bits(plane)), f"{regime}: the depth-tested plane of frame {k} differs"
            assert np.array_equal(_bits(got[0]), _bits(rgba)), f"{regime}: the depth-tested image of frame {k} differs"
        st = eng.stats()
        print(f"{regime}: culled {st['frames_culled']} slab {st['frames_slab']} lazy {st['frames_lazy']} repaired {st['frames_repaired']}")
        if stat:
            assert st[stat] >= 2, (regime, stat, st[stat])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1])
def test_band_planes_stitch_to_the_plane(pkg, big, layout):
    """two row shards: each writes its band plane (gsr_band_rows() rows, the padding zero), and the bands' tile rows put back where
    they belong are the unsharded plane"""
    E = pkg.engine
    s, cams, depth, want, want_d = big
    eng = pkg.Engine(0)
    try:
        eng.set_option(E.OPT_SHARD_LAYOUT, layout)
        eng.upload(s)
        for c, d, (rgba, plane) in ((cams[0], None, want[0]), (cams[4], None, want[4]), (cams[1], depth, want_d[1])):
            bands, imgs = [], []
            for idx in range(2):
                eng.set_row_shard(idx, 2)
                img, band = eng.render_aov(c, d)
                assert band.shape == (eng.band_rows(RH), RW, 2)
                bands.append(band); imgs.append(img)
            assert np.array_equal(_bits(pkg.multigpu.stitch_bands_host(np.stack(bands), RH, layout)), _bits(plane)), layout
            assert np.array_equal(_bits(pkg.multigpu.stitch_bands_host(np.stack(imgs), RH, layout)), _bits(rgba)), layout
    finally:
        eng.close()


@pytest.mark.gpu
def test_resolve_on_the_device_is_the_host_rule(pkg, oracle, engine):
    """gsr_resolve_depth_device = gsr_resolve_depth bit for bit, and what it leaves is a depth buffer gsr_render_depth accepts"""
    E = pkg.engine
    s, cam = _scene(pkg, "stock")
    engine.upload(s)
    hb = HipBuffers()
    try:
        d_img, d_plane, d_depth = hb.alloc(W * H * 16), hb.alloc(W * H * 8), hb.alloc(W * H * 4)
        cs = E.camera_struct(cam)
        engine.render_aov_struct_to_device(cs, d_img, d_plane)
        plane = hb.download(d_plane, (H, W, 2))
        assert np.array_equal(_bits(plane), _bits(engine.render_aov(cam)[1]))
        assert ((plane[..., 1] > 0) & (plane[..., 1] < 0.5)).any() and (plane[..., 1] >= 0.5).any() and (plane[..., 1] == 0).any()
        for cov_min in (0.5, 0.0, 0.999):
            engine.resolve_depth_device(d_plane, W * H, cov_min, d_depth)
            engine.synchronize()
            got = hb.download(d_depth, (H, W))
            assert np.array_equal(_bits(got), _bits(engine.resolve_depth(plane, cov_min))), cov_min
            assert (got >= 0).all() and (got <= 1).all()
        engine.resolve_depth_device(d_plane, W * H, 0.5, d_depth)
        resolved = engine.resolve_depth(plane, 0.5)
        assert 0.05 < (resolved < 1).mean() < 0.95
        # ... from device memory, straight into the next depth-tested frame; the same frame from the host copy; and the oracle's
        engine.render_struct_depth_to_device(cs, d_depth, d_img)
        img = hb.download(d_img, (H, W, 4))
        assert np.array_equal(_bits(img), _bits(engine.render_depth(cam, resolved)))
        check_contract(img, oracle, s, cam, depth=resolved, label="depth = resolved AOV")
        assert not np.array_equal(img, engine.render(cam))
        import ctypes as C
        assert engine.L.gsr_resolve_depth_device(engine.h, C.c_void_p(d_plane + 4), 4, C.c_float(0.5), C.c_void_p(d_depth)) == -1
    finally:
        hb.free()


def test_aov_kernels_keep_their_budgets():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): both k_blend_aov instantiations use no
    scratch, at most 80 registers -- the six waves per SIMD of DESIGN.md section 4.5 -- and at most 22 KB of LDS, the limit the
    depth-tested colour kernel is held to (seven workgroups in a CU's 160 KB)"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for prefix in ("_Z11k_blend_aovILb0E", "_Z11k_blend_aovILb1E"):
        hit = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, sorted(rows))
        vg, sg, lds, scratch = hit[0]
        print(f"{prefix}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0 and vg <= 80 and lds <= 22 * 1024, (prefix, hit[0])
