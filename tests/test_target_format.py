"""Target formats (gsr_set_target_format), the part that needs no GPU: the pixel sizes, the argument checks, the dry shim, and
gsr_convert_pixels -- the host conversion every GPU frame in a packed format is held to (tests/test_target_format_gpu.py) --
against independent numpy models, bit for bit."""
import ctypes as C

import numpy as np
import pytest

GSR_E_INVALID = -1


def test_pixel_bytes(pkg):
    L = pkg.load_library()
    e = pkg.engine
    assert (e.TARGET_RGBA32F, e.TARGET_RGBA16F, e.TARGET_RGBA8) == (0, 1, 2)
    assert [L.gsr_target_pixel_bytes(f) for f in (0, 1, 2)] == [16, 8, 4]
    for bad in (-1, 3, 4, 16, 255, 1 << 20):
        assert L.gsr_target_pixel_bytes(bad) == GSR_E_INVALID


def test_null_context_is_rejected(pkg):
    L = pkg.load_library()
    assert L.gsr_set_target_format(None, 1) == GSR_E_INVALID
    assert L.gsr_get_target_format(None) == GSR_E_INVALID
    assert L.gsr_multi_set_target_format(None, 1) == GSR_E_INVALID
    assert L.gsplat_renderer_set_target_format(None, 1) == GSR_E_INVALID


def test_dry_shim_validates_and_remembers(pkg):
    R = pkg.GSplatRenderer(device=-1)
    try:
        assert R.targetFormat() == 0
        for fmt in (1, 2, 0, 2):
            assert R.setTargetFormat(fmt) == 0
            assert R.targetFormat() == fmt
        for bad in (-1, 3, 7):
            assert R.setTargetFormat(bad) == GSR_E_INVALID
            assert R.targetFormat() == 2      # the format in use stays
    finally:
        R.close()


def _ulps(x, k):
    """x moved by k float32 steps"""
    x = np.asarray(x, np.float32)
    out = x.copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return out


def _inputs():
    rng = np.random.default_rng(20240611)
    k = np.arange(0, 256, dtype=np.float64)
    # the thresholds between two bytes, k/255 +- 0.5/255, as float32, and one step either side of each
    edges = np.concatenate([(k - 0.5) / 255.0, (k + 0.5) / 255.0, k / 255.0]).astype(np.float32)
    parts = [rng.uniform(-1.0, 2.0, 200_000).astype(np.float32), edges, _ulps(edges, 1), _ulps(edges, -1),
             np.array([65504.0, 65519.996, 65520.0, 65536.0, 1.0e7, -65504.0, -65520.0, -1.0e7], np.float32),
             np.array([0.0, -0.0, np.inf, -np.inf], np.float32),
             # float32 denormals, and the range where binary16 itself is denormal (2^-24 .. 2^-14) with its round-to-even ties
             np.array([1.0e-45, -1.0e-45, 1.0e-40, 1.1754942e-38, 2.0 ** -25, _ulps(2.0 ** -25, 1), 2.0 ** -24, 1.5 * 2.0 ** -24,
                       2.5 * 2.0 ** -24, 2.0 ** -14, _ulps(2.0 ** -14, -1), 6.0e-8, 6.1e-5], np.float32),
             # ties of the 11-bit significand: 1 + (2j + 1) 2^-11 rounds to even
             (1.0 + (2.0 * np.arange(16) + 1.0) * 2.0 ** -11).astype(np.float32),
             rng.uniform(-70000.0, 70000.0, 4096).astype(np.float32)]
    x = np.concatenate([p.ravel() for p in parts])
    x = np.concatenate([x, np.zeros((-x.size) % 4, np.float32)])
    return x.reshape(-1, 4)


def test_convert_rgba32f_is_a_copy(pkg):
    x = _inputs()
    out = pkg.engine.convert_pixels(x, pkg.engine.TARGET_RGBA32F)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), x.view(np.uint32))


def test_convert_rgba16f_is_round_to_nearest_even(pkg):
    """gsr_convert_pixels(RGBA16F) == x.astype(np.float16) on the uint16 views: numpy's conversion is IEEE round to nearest even
    with overflow to infinity (65520 is the first value that rounds to inf; 65519.996 still gives 65504)."""
    x = _inputs()
    assert x.size >= 100_000
    out = pkg.engine.convert_pixels(x, pkg.engine.TARGET_RGBA16F)
    assert out.dtype == np.float16 and out.shape == x.shape
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert np.array_equal(out.view(np.uint16), want.view(np.uint16))
    # ... and the rule attributes are quantised with (gsplat_quantize_half)
    assert np.array_equal(out.view(np.uint16), pkg.engine.quantize_half(x))


def test_convert_rgba8_is_one_rounding_then_truncation(pkg):
    """gsr_convert_pixels(RGBA8) == floor(float32(clip(x, 0, 1) * 255 + 0.5)) with NaN -> 0, on the uint8 views.  The model forms
    c * 255 + 0.5 in float64 and rounds ONCE to float32: c has 24 significant bits and 255 has 8, so the float64 product (53 bits)
    is exact, and adding 0.5 is exact in float64 as well wherever the sum lies within 2^-20 of an integer -- the only place where
    a second rounding could change floor().  The model therefore equals the kernel's single-rounding fmaf(c, 255, 0.5) followed by
    truncation."""
    x = np.concatenate([_inputs().ravel(), np.array([np.nan, -np.nan, np.nan, 0.25], np.float32)]).reshape(-1, 4)
    out = pkg.engine.convert_pixels(x, pkg.engine.TARGET_RGBA8)
    assert out.dtype == np.uint8 and out.shape == x.shape
    y = np.where(np.isnan(x), np.float32(0.0), x)
    want = np.floor((np.clip(y, 0, 1).astype(np.float64) * 255.0 + 0.5).astype(np.float32)).astype(np.uint8)
    assert np.array_equal(out, want)
    assert out.min() == 0 and out.max() == 255


def test_convert_argument_checks(pkg):
    L = pkg.load_library()
    x = np.zeros((2, 4), np.float32)
    out = np.zeros(32, np.uint8)
    assert L.gsr_convert_pixels(x.ctypes.data, 2, 3, out.ctypes.data) == GSR_E_INVALID
    assert L.gsr_convert_pixels(None, 2, 1, out.ctypes.data) == GSR_E_INVALID
    assert L.gsr_convert_pixels(x.ctypes.data, 2, 1, None) == GSR_E_INVALID
    assert L.gsr_convert_pixels(x.ctypes.data, -1, 1, out.ctypes.data) == GSR_E_INVALID
    assert L.gsr_convert_pixels(None, 0, 2, None) == 0
    with pytest.raises(pkg.GsrError):
        pkg.engine.convert_pixels(np.zeros((3, 3), np.float32), 1)


def test_frame_gatherer_takes_a_dtype(pkg):
    """multigpu.FrameGatherer sizes its buffers by the band's channel type (no process group needed to construct one rank)"""
    import inspect
    assert "dtype" in inspect.signature(pkg.multigpu.FrameGatherer.__init__).parameters
    g = np.arange(2 * 16 * 5 * 4, dtype=np.float32).reshape(2, 16, 5, 4)
    for dt in (np.float32, np.float16, np.uint8):
        img = pkg.multigpu.stitch_bands_host(g.astype(dt), 24)
        assert img.dtype == dt and img.shape == (24, 5, 4)
