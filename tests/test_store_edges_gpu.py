"""The device's pixel stores, background decode and compositing rule at their edge values.

The lines of csrc/gsr_device.h that turn a finished f32 pixel into a target pixel (gsr_channel_half, gsr_channel_unorm8,
gsr_store_packed), decode a background image (gsr_background_pixel) and composite over it (gsr_composite_over_pixel) run on x86 AND
on gfx950: two compilers, two sets of conversion instructions, two denormal settings.  The host side is held to numpy models at every
edge (test_target_format.py, test_background.py); rendered frames of ordinary scenes hold the device side to the host side only at
the values such frames happen to contain.  Here chosen values go THROUGH THE DEVICE: an empty cloud has S = 0 on every pixel, so over
an image with B_a = 0 the rule gives out_c = fmaf(1, 0, B_c) -- the image's f32 values reach the kernel's epilogue and store as they
are -- and an RGBA16F / RGBA8 image drives the kernel's decode the same way.

Every expectation is the numpy model (test_background.rule / store / decode) AND the host library (composite_over /
convert_pixels); the two must agree with each other and with the device.  Comparisons follow the NaN rule
(helpers.assert_same_pixels): a NaN channel on one side is a NaN on the other, everything else is bit-exact."""
import numpy as np
import pytest

from helpers import NAN_PATTERNS, HipBuffers, assert_same_pixels, pixels_differ, store_edge_classes, veil_scene
from test_background import decode, rule, store
from test_blend_contract import _border_scene
from test_target_format import _inputs

pytestmark = pytest.mark.gpu

FMTS = (0, 1, 2)


def _want(E, S, bg, fmt, label):
    """the over-frame by the numpy rule, after the host library has been held to it"""
    with np.errstate(all="ignore"):
        B = np.asarray(bg, np.float32) if isinstance(bg, tuple) else decode(bg)
        want = rule(S, B, fmt)
    assert_same_pixels(E.composite_over(S, bg, fmt), want, label + ": gsr_composite_over against the numpy rule")
    return want


def _converted(E, f32, fmt, label):
    with np.errstate(all="ignore"):
        want = store(f32, fmt)
    assert_same_pixels(E.convert_pixels(f32, fmt), want, label + ": gsr_convert_pixels against the numpy store")
    return want


def _over_frames(E, eng, hb, cam, img, d_target):
    """[(route, frame)]: the over-frame of an image by host and device targets with host and device images"""
    H, W = cam.height, cam.width
    dt = E.target_dtype(eng.target_format)
    cs = E.camera_struct(cam)
    out = [("host target, host image", eng.render_over(cam, img))]
    b_host, keep = E.background_struct(img, (H, W))
    b_dev, _ = E.background_struct(img, (H, W))
    b_dev.image, b_dev.image_is_device = hb.upload(img), 1
    for route, b in (("device target, host image", b_host), ("device target, device image", b_dev)):
        eng.render_over_struct_to_device(cs, b, d_target)
        eng.synchronize()
        out.append((route, hb.download(d_target, (H, W, 4), dt)))
    host = np.empty((H, W, 4), dt)
    eng.render_over_struct_to_host(cs, b_dev, host.ctypes.data)
    out.append(("host target, device image", host))
    return out


@pytest.fixture()
def rig(pkg):
    """an engine holding an EMPTY cloud, raw device buffers, a device target large enough for every frame below"""
    eng = pkg.Engine(0)
    hb = HipBuffers()
    try:
        eng.upload(pkg.scenes.make_scene(0, seed=1, sh=False))
        yield eng, hb, hb.alloc(52 * 1024 * 16)
    finally:
        eng.close()
        hb.free()


# ---- a. every store edge through the device ----
WA = 257                           # odd, no multiple of the 16-pixel tile


def _edge_image():
    """test_target_format._inputs() -- every byte threshold +- 1 ulp, binary16 ties, the binary16 denormal range, 65504 / 65519.996 /
    65520, +-inf, -0 -- padded with NaNs of both signs and several payloads to a 257-wide frame"""
    x = _inputs().ravel()
    h = -(-x.size // (4 * WA))
    x = np.concatenate([x, np.resize(NAN_PATTERNS, h * WA * 4 - x.size)])
    assert h * WA <= 52 * 1024 and np.isnan(x).sum() >= 8
    return x.reshape(h, WA, 4)


@pytest.mark.parametrize("fmt", FMTS)
def test_every_store_edge_through_the_device(pkg, rig, fmt):
    """pass 1: the edge values as an RGBA32F image with alpha 0 over the empty cloud: out = fmaf(1, 0, B) = B (-0 becomes +0), stored;
    pass 2: the alpha channel left as the raw values, so that k = 1 - B_a is arbitrary (0 * k is NaN under an infinite or NaN
    alpha) and the values that sat in the alpha channel reach the store as out_a = B_a;
    pass 3: pass 1 with the values moved on by two channels, so that passes 1 and 3 together put every value into a colour channel"""
    E = pkg.engine
    eng, hb, d_target = rig
    raw = _edge_image()
    h = raw.shape[0]
    cam = pkg.camera.make_camera(WA, h, sh_order=0)
    S = np.zeros_like(raw)
    eng.set_target_format(fmt)
    zero_alpha = raw.copy()
    zero_alpha[..., 3] = 0
    moved = np.roll(raw.ravel(), 2).reshape(raw.shape).copy()
    moved[..., 3] = 0
    for name, img in (("alpha 0", zero_alpha), ("raw alpha", raw), ("alpha 0, moved", moved)):
        label = f"format {fmt}, {name}"
        want = _want(E, S, img, fmt, label)
        if name != "raw alpha":
            # (what the issue of this test calls store(values): the rule over S = 0, B_a = 0 IS the store, but for the sign of -0)
            stored = _converted(E, img, fmt, label)
            d = pixels_differ(want, stored)
            if fmt == 2:
                assert not d.any(), label
            else:
                assert np.array_equal(d, (img == 0) & np.signbit(img)), label
        with np.errstate(all="ignore"):
            cls = store_edge_classes(rule(S, img, 0))
        print(f"STORE EDGES {label}: {raw.shape[1]}x{h}, values reaching the store: {cls}")
        # (fmaf(1, 0, -0) is +0; the raw pass's infinities sit in a pixel whose alpha is -inf: k = +inf, 0 * k = NaN)
        assert min(v for k, v in cls.items() if k != "neg_zero" and (k != "inf" or name != "raw alpha")) > 0, cls
        assert cls["ties"] >= 12 and cls["byte_edges"] >= 500 and cls["nan"] >= 8 and cls["negatives"] > 10000, cls
        for route, got in _over_frames(E, eng, hb, cam, img, d_target):
            assert_same_pixels(got, want, f"{label}, {route}")
    if fmt == 2:
        assert want.min() == 0 and want.max() == 255


# ---- b. every binary16 value through the decode ----
WB, HB = 131, 167


def _half_image():
    bits = np.zeros(HB * WB * 3, np.uint16)
    bits[:65536] = np.arange(65536, dtype=np.uint16)
    img = np.zeros((HB, WB, 4), np.uint16)
    img[..., :3] = bits.reshape(HB, WB, 3)
    return img.view(np.float16)


@pytest.mark.parametrize("fmt", FMTS)
def test_every_binary16_value_through_the_decode(pkg, rig, fmt):
    """all 65536 half bit patterns in the colour channels of an RGBA16F image, alpha 0, over the empty cloud.  RGBA32F target: the bits
    of half.astype(float32) -- denormals, infinities -- except that the rule's fma turns -0 into +0 and a NaN is some NaN; RGBA16F
    target: the identity on every pattern but NaNs and -0; RGBA8: the store of the decoded value"""
    E = pkg.engine
    eng, hb, d_target = rig
    img = _half_image()
    cam = pkg.camera.make_camera(WB, HB, sh_order=0)
    S = np.zeros((HB, WB, 4), np.float32)
    eng.set_target_format(fmt)
    label = f"format {fmt}, all halves"
    want = _want(E, S, img, fmt, label)
    v = img.astype(np.float32)                                                # (exact)
    plain = ~np.isnan(v) & ~((v == 0) & np.signbit(v))
    assert plain.sum() == HB * WB * 4 - 2046 - 1                            # (2046 NaN patterns, one -0)
    cls = store_edge_classes(v)
    print(f"STORE EDGES {label}: {WB}x{HB}, decoded values: {cls}")
    assert cls["nan"] == 2046 and cls["inf"] == 2 and cls["half_denormals"] == 2046 and cls["negatives"] == 31744
    if fmt == 0:
        assert np.array_equal(want.view(np.uint32)[plain], v.view(np.uint32)[plain]) and np.isnan(want[np.isnan(v)]).all()
        assert (want.view(np.uint32)[(v == 0) & np.signbit(v)] == 0).all()
    if fmt == 1:
        assert np.array_equal(want.view(np.uint16)[plain], img.view(np.uint16)[plain])
    for route, got in _over_frames(E, eng, hb, cam, img, d_target):
        assert_same_pixels(got, want, f"{label}, {route}")


# ---- c. every byte through the decode ----
@pytest.mark.parametrize("fmt", FMTS)
def test_every_byte_through_the_decode(pkg, rig, fmt):
    """a 17 x 17 RGBA8 image (four tiles, three of them cut) in which every channel, alpha included, takes all 256 values.  S = 0, so
    out_c = fmaf(k, 0, B_c) = B_c for every finite k.  RGBA32F target: float32(byte) / float32(255), one IEEE division, bit for bit;
    RGBA8 target: the identity on every byte"""
    E = pkg.engine
    eng, hb, d_target = rig
    i = np.arange(17 * 17)
    img = np.stack([i % 256, (3 * i + 7) % 256, (255 - i) % 256, (5 * i + 1) % 256], -1).astype(np.uint8).reshape(17, 17, 4)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(4))
    cam = pkg.camera.make_camera(17, 17, sh_order=0)
    S = np.zeros((17, 17, 4), np.float32)
    eng.set_target_format(fmt)
    label = f"format {fmt}, all bytes"
    want = _want(E, S, img, fmt, label)
    if fmt == 0:
        assert np.array_equal(want.view(np.uint32), (img.astype(np.float32) / np.float32(255.0)).view(np.uint32))
        assert (want != (img.astype(np.float32) * (np.float32(1.0) / np.float32(255.0)))).any()      # (a reciprocal would show)
    if fmt == 2:
        assert np.array_equal(want, img)
    for route, got in _over_frames(E, eng, hb, cam, img, d_target):
        assert_same_pixels(got, want, f"{label}, {route}")


# ---- d. out-of-range frames in every format, over backgrounds, with the AOV, culled ----
def _camera_d(pkg, name, shift=0):
    """the scene's camera, `shift` steps further along its orbit"""
    if name == "adversarial":
        return pkg.camera.make_camera(257, 129, sh_order=3, frame=3 + shift)
    return pkg.camera.make_camera(240, 180, sh_order=0 if name == "beyond one" else 3, frame=2 + shift)


def _scene_d(pkg, name):
    cam = _camera_d(pkg, name)
    if name == "adversarial":           # the scene of test_gpu_parity.test_adversarial_inputs at its 257 x 129 camera
        rng = np.random.default_rng(5)
        s = pkg.scenes.make_scene(4000, seed=81, sh=True)
        f16 = pkg.scenes.f16bits
        s.P[10] = np.nan
        s.P[11, 0] = np.inf
        s.P[12] = -np.inf
        s.scale[20:40] = 0
        s.scale[40:46] = f16(np.full((6, 3), 3.0e4))
        s.scale[46:50] = f16(np.full((4, 3), np.inf))
        s.alpha[60:70] = -0.5
        s.alpha[70:80] = 37.0
        s.alpha[80:85] = np.nan
        s.alpha[85:90] = 1.0 / 255.0
        s.orient[90:100] = 0
        s.orient[100:110] = f16(rng.normal(0, 30, (10, 4)))
        s.shx[110:120] = 0x7C00
        return s, cam
    if name == "beyond one":            # the Cd in [-2, 6] veil of test_blend_contract.test_colours_beyond_one
        return veil_scene(pkg, cam, n=2500, seed=11, colours=(-2.0, 6.0)), cam
    # Cd near 6e4 with SH coefficients of the same size on top (a splat's colour is max(Cd + SH, 0): up to a few 1e5), stacked
    s = pkg.scenes.make_scene(5000, seed=14, sh=True)
    rng = np.random.default_rng(14)
    s.Cd[:] = pkg.scenes.f16bits(rng.uniform(5.5e4, 6.5e4, (s.n, 3)))
    for a in (s.shx, s.shy, s.shz):
        a[:, :15] = pkg.scenes.f16bits(rng.normal(0.0, 2.0e4, (s.n, 15)))
    return s, cam


def _frame_classes(img):
    c = img[..., :3]
    return {"nan": int(np.isnan(img).any(-1).sum()), "inf": int(np.isinf(img).any(-1).sum()), "above_65520": int((np.isfinite(c) & (c > 65520)).sum()),
            "in_1_65504": int(((c > 1) & (c < 65504)).sum()), "negative": int((c < 0).sum())}


# Teeth: what the RGBA32F frame of each scene must hold before anything is compared -- at least HALF of what the CPU oracle's frame
# of the same scene and camera holds (oracle.render; pixels for nan / inf, colour channels otherwise).  The oracle's frames hold:
#   adversarial   nan 0, inf 0, above 65520     0, in (1, 65504)    16, negative    0
#   beyond one    nan 0, inf 0, above 65520     0, in (1, 65504) 52512, negative 3043
#   overflow      nan 0, inf 0, above 65520  5895, in (1, 65504) 34612, negative    0
# NO frame holds a NaN or an infinity, and none can: the contract makes a splat's colour finite where it is formed (NaN -> 0, +-inf ->
# +-3e38: csrc/k_preprocess.h, gso_finite_colour in the oracle), a fragment's weight is at most 1 and a pixel's weights sum to
# 1 - T <= 1, so a channel stays below 3e38 (1 + a few ulp) < FLT_MAX.  Non-finite values reach the stores of these frames through the
# backgrounds below, and through the images of the tests above.  So "nan" and "inf" are asserted to be EXACTLY 0 -- the invariant, which
# a kernel that stopped making colours finite would break -- and the other classes to reach half of the oracle's count.
TEETH = {"adversarial": {"above_65520": 0, "in_1_65504": 8, "negative": 0},
         "beyond one": {"above_65520": 0, "in_1_65504": 26256, "negative": 1521},
         "overflow": {"above_65520": 2947, "in_1_65504": 17306, "negative": 0}}
SCENES = ("adversarial", "beyond one", "overflow")
# A front-slab frame needs the cloud's bounding box (gsr_plan_frame: bbox_ok), and the adversarial cloud, with NaN and infinite
# positions, has none: OPT_OCCLUSION_CULL = 3 renders it as ordinary frames.  The other two clouds must take the slab path.
TAKES_SLAB = {"adversarial": False, "beyond one": True, "overflow": True}


def _backgrounds(w, h, seed=33):
    """a colour with k = 0.5, a colour with k < 0 and a channel beyond binary16; an RGBA16F image with alpha in {0, 0.4, 1} and, on a
    lattice of pixels, alpha 1.5, -0.5, +inf, NaN and colours that are infinite, negative or NaN (the background is the caller's data and
    is not sanitised); an RGBA8 image of random bytes"""
    rng = np.random.default_rng(seed)
    alpha = rng.choice(np.array([0.0, 0.4, 1.0], np.float32), (h, w))
    f = np.concatenate([rng.random((h, w, 3)).astype(np.float32) * alpha[..., None], alpha[..., None]], -1).astype(np.float16)
    f[0::7, 0::5, 3] = 1.5
    f[1::7, 1::5, 3] = -0.5
    f[2::7, 2::5, 3] = np.inf
    f[3::7, 3::5, 3] = np.nan
    f[4::7, 4::5, 0] = np.inf
    f[5::7, 0::5, 1] = -3.0
    f[6::7, 1::5, 2] = np.nan
    return {"colour": (0.1, 0.2, 0.3, 0.5), "colour beyond": (70000.0, -0.25, 0.5, 1.5), "f16": f, "u8": rng.integers(0, 256, (h, w, 4)).astype(np.uint8)}


@pytest.fixture(scope="module")
def plain_frames(pkg):
    """{scene: (splats, [the scene's camera, the next two of its orbit], their RGBA32F frames from a context that was never given a
    format)}.  The moved cameras are for the front-slab frames: a redraw of one camera is served from the sort cache and is never a slab"""
    out = {}
    eng = pkg.Engine(0)
    try:
        for name in SCENES:
            s, cam = _scene_d(pkg, name)
            cams = [cam] + [_camera_d(pkg, name, shift) for shift in (1, 2)]
            eng.upload(s)
            out[name] = (s, cams, [eng.render(c).copy() for c in cams])
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("name", SCENES)
def test_out_of_range_frames_in_every_format(pkg, plain_frames, name):
    E = pkg.engine
    s, cams, f32s = plain_frames[name]
    cam, f32 = cams[0], f32s[0]
    H, W = cam.height, cam.width
    assert s.n <= 20000 and W * H <= 52 * 1024
    got = _frame_classes(f32)
    print(f"STORE EDGES frame '{name}' {W}x{H}: {got}; all channels: {store_edge_classes(f32)}")
    assert got["nan"] == 0 and got["inf"] == 0, (name, got)
    for k, v in TEETH[name].items():
        assert got[k] >= v, (name, k, got[k], v)
    bgs = _backgrounds(W, H)
    eng = pkg.Engine(0)
    try:
        eng.upload(s)
        for fmt in FMTS:
            eng.set_target_format(fmt)
            label = f"'{name}', format {fmt}"

            def wanted(i):
                """{None: the packed frame of camera i, key: its over-frame} by the numpy models, the host library held to them"""
                out = {None: _converted(E, f32s[i], fmt, f"{label}, camera {i}")}
                for key, bg in bgs.items():
                    out[key] = _want(E, f32s[i], bg, fmt, f"{label}, camera {i} over {key}")
                return out

            def frames(tag, i, want):
                """the packed frame and every over-frame of camera i: 1 + len(bgs) frames"""
                assert_same_pixels(eng.render(cams[i]), want[None], f"{label}, {tag}")
                for key, bg in bgs.items():
                    assert_same_pixels(eng.render_over(cams[i], bg), want[key], f"{label} over {key}, {tag}")

            want = wanted(0)
            frames("default policy", 0, want)
            rgba, plane = eng.render_aov(cam)
            assert_same_pixels(rgba, want[None], f"{label}, beside the AOV")
            assert_same_pixels(plane[..., 1], f32[..., 3], f"{label}, cov against the f32 alpha")
            # occlusion culling forced on: the same camera three times (it engages from the slot's second frame)
            before = eng.stats()
            eng.set_option(E.OPT_OCCLUSION_CULL, 2)
            try:
                for k in range(3):
                    frames(f"occlusion cull 2, frame {k}", 0, want)
                culled = eng.stats()["frames_culled"] - before["frames_culled"]
                # every frame a front slab: phase 2 continues from the raw f32 pixels kept beside the target, never from a stored or
                # composited one.  The camera moves, or the frame would be a sort-cache hit and no slab
                before = eng.stats()
                eng.set_option(E.OPT_OCCLUSION_CULL, 3)
                for i in (1, 2):
                    frames(f"occlusion cull 3, camera {i}", i, wanted(i))
                slabs = eng.stats()["frames_slab"] - before["frames_slab"]
            finally:
                eng.set_option(E.OPT_OCCLUSION_CULL, 1)
            print(f"{label}: of {3 * (1 + len(bgs))} frames under cull 2 {culled} were culled; of {2 * (1 + len(bgs))} under cull 3 {slabs} were front slabs")
            assert culled >= 1, (label, culled)
            if TAKES_SLAB[name]:
                assert slabs >= 2, (label, slabs)
            else:
                assert slabs == 0, (label, slabs)
    finally:
        eng.close()


# ---- e. the smallest targets, with canaries ----
GUARD = 64
SIZES = [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (31, 33)]


def _guarded(hb, nbytes):
    """a device buffer of nbytes between two guards of 64 bytes, all of it 0xA5; returns (base, the pixel-aligned pointer inside)"""
    base = hb.upload(np.full(nbytes + 2 * GUARD, 0xA5, np.uint8))
    return base, base + GUARD


def _check_guarded(hb, base, want, label):
    """the bytes between the guards are `want`'s (NaN rule), and all 128 guard bytes are still 0xA5"""
    raw = hb.download(base, (want.nbytes + 2 * GUARD,), np.uint8)
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), f"{label}: a write outside the target: {raw[:GUARD].tolist()} ... {raw[-GUARD:].tolist()}"
    assert_same_pixels(raw[GUARD:-GUARD].view(want.dtype).reshape(want.shape), want, label)


def _small_image(w, h, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    alpha = rng.choice(np.array([0.0, 0.4, 1.0], np.float32), (h, w))
    f = np.concatenate([rng.random((h, w, 3)).astype(np.float32) * alpha[..., None], alpha[..., None]], -1)
    return f.astype(np.float32 if fmt == 0 else np.float16)


@pytest.mark.parametrize("w,h", SIZES)
def test_smallest_targets_keep_inside_their_bytes(pkg, w, h):
    """test_blend_contract's border scene at the sizes where a tile is cut on one side or both, down to one pixel: every format, plain
    and over an image (of another format than the target's), and the AOV plane, into device targets between guard bytes"""
    E = pkg.engine
    cam = pkg.camera.make_camera(w, h, sh_order=0, frame=0)
    s = _border_scene(pkg, cam, seed=w * 1000 + h)
    plain, eng = pkg.Engine(0), pkg.Engine(0)
    hb = HipBuffers()
    try:
        plain.upload(s)
        eng.upload(s)
        f32 = plain.render(cam).copy()
        assert f32[..., 3].max() > 0
        cs = E.camera_struct(cam)
        for fmt in FMTS:
            eng.set_target_format(fmt)
            label = f"{w}x{h}, format {fmt}"
            nbytes = w * h * 4 * E.target_dtype(fmt).itemsize
            want = _converted(E, f32, fmt, label)
            base, ptr = _guarded(hb, nbytes)
            eng.render_struct_to_device(cs, ptr)
            eng.synchronize()
            _check_guarded(hb, base, want, label + ", plain")
            img = _small_image(w, h, (fmt + 1) % 3, seed=w + h + fmt)
            b, keep = E.background_struct(img, (h, w))
            base, ptr = _guarded(hb, nbytes)
            eng.render_over_struct_to_device(cs, b, ptr)
            eng.synchronize()
            _check_guarded(hb, base, _want(E, f32, img, fmt, label), label + ", over an image")
            base, ptr = _guarded(hb, nbytes)
            pbase, pptr = _guarded(hb, w * h * 8)
            eng.render_aov_struct_to_device(cs, ptr, pptr)
            eng.synchronize()
            _check_guarded(hb, base, want, label + ", beside the AOV")
            plane = hb.download(pbase, (w * h * 8 + 2 * GUARD,), np.uint8)
            assert (plane[:GUARD] == 0xA5).all() and (plane[-GUARD:] == 0xA5).all(), label + ": a write outside the AOV plane"
            assert_same_pixels(plane[GUARD:-GUARD].view(np.float32).reshape(h, w, 2)[..., 1], f32[..., 3], label + ", cov")
    finally:
        plain.close()
        eng.close()
        hb.free()


@pytest.mark.parametrize("layout", [0, 1])
def test_a_band_leaves_its_padding_rows_alone(pkg, layout):
    """31 x 33 under set_row_shard(1, 2): three tile rows, the band image is two tile rows tall.  Interleaved rows: rank 1 owns tile row
    1 and one tile row is padding; contiguous bands: it owns tile row 2 -- ONE pixel row -- and 31 rows are padding.  A device target
    is never written there: the padding, like the guards, is still 0xA5"""
    E = pkg.engine
    w, h = 31, 33
    cam = pkg.camera.make_camera(w, h, sh_order=0, frame=0)
    s = _border_scene(pkg, cam, seed=w * 1000 + h)
    plain, eng = pkg.Engine(0), pkg.Engine(0)
    hb = HipBuffers()
    try:
        plain.upload(s)
        f32 = plain.render(cam).copy()
        eng.set_option(E.OPT_SHARD_LAYOUT, layout)
        eng.upload(s)
        eng.set_row_shard(1, 2)
        rows = eng.band_rows(h)
        owned = pkg.multigpu.owned_tile_rows(h, 1, 2, layout)
        assert rows == 32 and owned == ([1], [2])[layout]
        cs = E.camera_struct(cam)

        def band(full):
            """the device band: 0xA5 wherever the rank owns nothing"""
            out = np.empty((rows, w) + full.shape[2:], full.dtype)
            out.view(np.uint8).fill(0xA5)
            for lrow, trow in enumerate(owned):
                y0, y1 = trow * 16, min(trow * 16 + 16, h)
                out[lrow * 16: lrow * 16 + (y1 - y0)] = full[y0:y1]
            return out

        for fmt in FMTS:
            eng.set_target_format(fmt)
            label = f"layout {layout}, format {fmt}"
            nbytes = rows * w * 4 * E.target_dtype(fmt).itemsize
            want = _converted(E, f32, fmt, label)
            img = _small_image(w, h, (fmt + 2) % 3, seed=layout + fmt)
            b, keep = E.background_struct(img, (h, w))
            base, ptr = _guarded(hb, nbytes)
            eng.render_struct_to_device(cs, ptr)
            eng.synchronize()
            _check_guarded(hb, base, band(want), label + ", plain")
            base, ptr = _guarded(hb, nbytes)
            eng.render_over_struct_to_device(cs, b, ptr)
            eng.synchronize()
            _check_guarded(hb, base, band(_want(E, f32, img, fmt, label)), label + ", over an image")
            base, ptr = _guarded(hb, nbytes)
            pbase, pptr = _guarded(hb, rows * w * 8)
            eng.render_aov_struct_to_device(cs, ptr, pptr)
            eng.synchronize()
            _check_guarded(hb, base, band(want), label + ", beside the AOV")
            cov = np.ascontiguousarray(f32[..., 3:4])
            plane = hb.download(pbase, (rows * w * 8 + 2 * GUARD,), np.uint8)
            assert (plane[:GUARD] == 0xA5).all() and (plane[-GUARD:] == 0xA5).all(), label + ": a write outside the AOV plane"
            got = plane[GUARD:-GUARD].view(np.float32).reshape(rows, w, 2)
            assert_same_pixels(np.ascontiguousarray(got[..., 1:2]), band(cov), label + ", cov and the plane's padding")
            assert np.array_equal(np.ascontiguousarray(got[..., 0]).view(np.uint32) == 0xA5A5A5A5, band(cov)[..., 0].view(np.uint32) == 0xA5A5A5A5), label + ", zsum's padding"
    finally:
        eng.set_row_shard(0, 1)
        plain.close()
        eng.close()
        hb.free()
