"""One context's host-target staging buffers across a change of frame size, shard, layout and target format.

A frame slot keeps its staging buffers -- the image, the AOV plane, the copy of a host depth buffer -- from frame to frame and
regrows them only when a frame needs more.  A sharded context's band is padded to whole tile rows (gsr_band_rows), and the rule is
that in a HOST target the padding rows read as zeros: the staging buffers are cleared whenever the band's shape -- for the image,
the shape or the target format -- is not the one they were last cleared for.  test_store_edges_gpu.py holds fresh contexts to that;
here ONE context first fills its staging with a larger frame and then renders the padded bands from the same buffers."""
import numpy as np
import pytest

from helpers import assert_same_pixels
from test_blend_contract import _border_scene
from test_store_edges_gpu import FMTS, _converted

pytestmark = pytest.mark.gpu

W, H = 31, 33                      # three tile rows, the last one a single pixel row; under set_row_shard(1, 2) the band is 32 rows
BIG = 48                           # the frame that dirties the staging: more bytes than any band below, in every format


def _band(full, rows, owned):
    """the host band of a rank: the rows of the tile rows it owns, zeros behind them"""
    out = np.zeros((rows,) + full.shape[1:], full.dtype)
    for lrow, trow in enumerate(owned):
        y0, y1 = trow * 16, min(trow * 16 + 16, H)
        out[lrow * 16: lrow * 16 + (y1 - y0)] = full[y0:y1]
    return out


def _padding(a, owned):
    """the bytes of a band behind the rows the rank owns"""
    n = sum(min(trow * 16 + 16, H) - trow * 16 for trow in owned)
    return np.ascontiguousarray(a[n:]).view(np.uint8)


def _fresh_depth_frame(pkg, s, cam, depth):
    with pkg.Engine(0) as e:
        e.upload(s)
        return e.render_depth(cam, depth).copy()


def test_one_context_across_band_shapes_and_formats(pkg):
    E = pkg.engine
    cam = pkg.camera.make_camera(W, H, sh_order=0, frame=0)
    big = pkg.camera.make_camera(BIG, BIG, sh_order=0, frame=0)
    s = _border_scene(pkg, cam, seed=W * 1000 + H)
    plain, eng = pkg.Engine(0), pkg.Engine(0)
    try:
        plain.upload(s)
        f32, plane32 = (a.copy() for a in plain.render_aov(cam))
        assert f32[..., 3].max() > 0
        eng.upload(s)

        # dirty the staging: a larger frame whose alpha is non-zero in every pixel row, image and plane
        rgba, plane = eng.render_aov(big)
        assert rgba.dtype == np.float32 and rgba.shape == (BIG, BIG, 4)
        assert (rgba[..., 3] != 0).any(axis=1).all() and (plane[..., 1] != 0).any(axis=1).all()
        assert BIG * BIG * 16 >= 32 * W * 16 and BIG * BIG * 8 >= 32 * W * 8

        # shrink and shard: the padded bands out of the same buffers
        for layout in (0, 1):
            eng.set_option(E.OPT_SHARD_LAYOUT, layout)
            eng.set_row_shard(1, 2)
            rows = eng.band_rows(H)
            owned = pkg.multigpu.owned_tile_rows(H, 1, 2, layout)
            assert rows == 32 and owned == ([1], [2])[layout]
            for fmt in reversed(FMTS):      # RGBA8, RGBA16F, RGBA32F: each clears more bytes than the one before
                eng.set_target_format(fmt)
                label = f"layout {layout}, format {fmt}"
                want = _band(_converted(E, f32, fmt, label), rows, owned)
                got = eng.render(cam)
                assert_same_pixels(got, want, label)
                assert not _padding(got, owned).any(), label + ": the image's padding rows"
            rgba, plane = eng.render_aov(cam)
            assert_same_pixels(rgba, _band(f32, rows, owned), f"layout {layout}, beside the AOV")
            assert_same_pixels(plane, _band(plane32, rows, owned), f"layout {layout}, the plane")
            assert not _padding(rgba, owned).any() and not _padding(plane, owned).any(), f"layout {layout}: padding beside the AOV"
            eng.set_row_shard(0, 1)

        # the host depth buffer's copy: a larger buffer first, then a smaller one with an occluder, each against a fresh context
        eng.set_option(E.OPT_SHARD_LAYOUT, 0)
        far = np.ones((BIG, BIG), np.float32)
        assert_same_pixels(eng.render_depth(big, far), _fresh_depth_frame(pkg, s, big, far), "far plane, 48 x 48")
        occ = np.ones((H, W), np.float32)
        occ[5:29, 4:27] = np.float32(1.0 - 0.01 / 3.5)      # (window depth at view distance 3.5: the scene stands 2 to 5 away)
        got = eng.render_depth(cam, occ)
        assert_same_pixels(got, _fresh_depth_frame(pkg, s, cam, occ), "occluder, 31 x 33")
        assert not np.array_equal(got, f32)                  # (the occluder really cut fragments)
    finally:
        eng.set_row_shard(0, 1)
        plain.close()
        eng.close()
