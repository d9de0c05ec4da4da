"""The selection overlay without a GPU (gsr_render_marks; include/gsplat_hip.h, "selection overlay"): the ABI, the refusals that need no
context, the style builder, the kernels' resources (a cross-compile), and the numpy models test_marks_gpu.py holds the GPU path to."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import marks_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1


def test_the_library_exports_both_symbols(pkg):
    E, L = pkg.engine, pkg.load_library()
    for name in ("gsr_render_marks", "gsr_get_marks"):
        assert name in E.C_ABI_SYMBOLS and getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("GSR_MARK_DOT", E.MARK_DOT), ("GSR_MARK_OUTLINE", E.MARK_OUTLINE), ("GSR_MARK_COLOUR_FIXED", E.MARK_COLOUR_FIXED),
                        ("GSR_MARK_COLOUR_CD", E.MARK_COLOUR_CD), ("GSR_MARK_ANY_OPACITY", E.MARK_ANY_OPACITY), ("GSR_MARK_MAX_RADIUS", E.MARK_MAX_RADIUS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    # the struct as the header lays it out: four ints, four floats, a pointer, an int, a float, an int (and the tail padding)
    assert C.sizeof(E.gsr_mark_style) == 56 and E.gsr_mark_style.depth.offset == 32 and E.gsr_mark_style.reserved_.offset == 48


def test_a_null_context_is_refused(pkg):
    E, L = pkg.engine, pkg.load_library()
    cam = pkg.camera.make_camera(64, 48, sh_order=3)
    cs = E.camera_struct(cam)
    st, _ = E.mark_style()
    frame = np.zeros((48, 64, 4), np.float32)
    wrote = C.c_int64(-7)
    assert L.gsr_render_marks(None, C.byref(cs), None, 0, C.byref(st), frame.ctypes.data, 0, C.byref(wrote)) == GSR_E_INVALID
    assert b"gsr_render_marks" in L.gsr_last_error() and wrote.value == -7 and not frame.any()
    assert L.gsr_get_marks(None, None, None, None) == GSR_E_INVALID


def test_mark_style_builds_and_refuses(pkg):
    E = pkg.engine
    st, keep = E.mark_style(E.MARK_DOT, 3, (0.5, 0.25, 0.0, 0.5), any_opacity=True, depth=np.zeros((4, 5), np.float32), depth_bias=0.125)
    assert (st.shape, st.radius, st.colour_mode, st.flags, st.depth_is_device, st.reserved_) == (E.MARK_DOT, 3, E.MARK_COLOUR_FIXED, E.MARK_ANY_OPACITY, 0, 0)
    assert list(st.rgba) == [0.5, 0.25, 0.0, 0.5] and st.depth == keep[0].ctypes.data and st.depth_bias == 0.125
    st, keep = E.mark_style(E.MARK_OUTLINE, colour="cd", depth_device=4096)
    assert (st.shape, st.radius, st.colour_mode, st.flags, st.depth, st.depth_is_device) == (E.MARK_OUTLINE, 0, E.MARK_COLOUR_CD, 0, 4096, 1) and not keep
    for r in (0, E.MARK_MAX_RADIUS):
        assert E.mark_style(E.MARK_DOT, r)[0].radius == r
    bad = [dict(shape=0), dict(shape=3), dict(shape=-1),
           dict(radius=-1), dict(radius=E.MARK_MAX_RADIUS + 1), dict(radius=1.5), dict(shape=E.MARK_OUTLINE, radius=1),
           dict(colour=(1.0, 1.0, np.nan, 1.0)), dict(colour=(np.inf, 0.0, 0.0, 1.0)), dict(colour=(0.0, 0.0, 0.0, np.nan)),
           dict(colour=(0.0, 0.0, 0.0, 1.5)), dict(colour=(0.0, 0.0, 0.0, -0.25)), dict(colour=(1.0, 1.0, 1.0)), dict(colour="yellow"),
           dict(depth=np.zeros(4, np.float32), depth_device=4096)]
    for kw in bad:
        with pytest.raises(pkg.GsrError):
            E.mark_style(**kw)


def test_the_kernels_take_no_scratch():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m and re.match(r"_Z6k_markILi[12]EE|_Z14k_mark_resolve", m.group(1)):
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for prefix in ("_Z6k_markILi1EE", "_Z6k_markILi2EE", "_Z14k_mark_resolve"):                           # <DOT>, <OUTLINE>, the resolve
        assert sum(k.startswith(prefix) for k in rows) == 1, (prefix, sorted(rows))
    assert len(rows) == 3, sorted(rows)
    for name, (vgpr, sgpr, lds, scratch) in rows.items():
        print(f"{name}: vgpr {vgpr} sgpr {sgpr} lds {lds} scratch {scratch}")
        assert scratch == 0 and lds == 0, (name, lds, scratch)


# ---- the numpy models -------------------------------------------------------------------------------------------------------------------
def _bits(z):
    return int(np.float32(z).view(np.uint32))


def test_the_dot_model_on_three_hand_made_splats():
    """an 8 x 6 image; splat 0 at pixel (2, 2), depth 0.5; splats 1 and 2 BOTH at pixel (4, 2), depth 0.25 (a tie: 1 shows)"""
    c = np.array([[2.5, 2.25, 0.5], [4.75, 2.5, 0.25], [4.0, 2.99, 0.25]], np.float32)
    all3 = np.ones(3, bool)
    z = MC.dot_keys(c, all3, 8, 6, 0)
    want = np.full((6, 8), MC.EMPTY, np.uint64)
    want[2, 2] = (_bits(0.5) << 32) | 0
    want[2, 4] = (_bits(0.25) << 32) | 1
    assert np.array_equal(z, want)
    # radius 1: the squares [1, 3] x [1, 3] and [3, 5] x [1, 3] share column 3, where the nearer splat 1 wins; 2 shows nowhere
    winner, zw = MC.split_keys(MC.dot_keys(c, all3, 8, 6, 1))
    want = np.full((6, 8), -1, np.int64)
    want[1:4, 1:3] = 0
    want[1:4, 3:6] = 1
    assert np.array_equal(winner, want)
    assert np.array_equal(zw[winner == 0], np.full(6, 0.5, np.float32)) and np.array_equal(zw[winner == 1], np.full(9, 0.25, np.float32))
    # without splat 1 its twin shows in the same pixels
    winner, _ = MC.split_keys(MC.dot_keys(c, np.array([True, False, True]), 8, 6, 1))
    assert np.array_equal(winner, np.where(want == 1, 2, want))
    # radius 8 covers the whole image, clipped; the nearest splat (lowest index on the tie) takes every pixel
    winner, _ = MC.split_keys(MC.dot_keys(c, all3, 8, 6, 8))
    assert (winner == 1).all()
    # centres outside the image, a NaN depth and an undrawn splat leave nothing
    out = np.array([[-0.5, 2.0, 0.5], [8.0, 2.0, 0.5], [2.0, 6.0, 0.5], [2.0, -0.01, 0.5], [np.nan, 1.0, 0.5], [1.0, 1.0, np.nan]], np.float32)
    assert (MC.dot_keys(out, np.ones(6, bool), 8, 6, 8) == MC.EMPTY).all()
    assert (MC.dot_keys(c, np.zeros(3, bool), 8, 6, 8) == MC.EMPTY).all()


def test_the_resolve_model(pkg):
    E = pkg.engine
    under = MC.frame_under(pkg, 8, 6, E.TARGET_RGBA32F)
    winner = np.full((6, 8), -1, np.int64)
    winner[2, 2], winner[2, 4], winner[5, 7] = 0, 1, 1
    zw = np.zeros((6, 8), np.float32)
    zw[2, 2], zw[2, 4], zw[5, 7] = 0.5, 0.25, 0.25
    Cd = pkg.scenes.f16bits(np.array([[1.0, 0.5, 0.25], [0.0, 0.125, 1.0]]))
    col = (0.5, 0.25, 0.0, 0.5)
    out, wrote = MC.resolve(pkg, under, winner, zw, col, Cd, E.TARGET_RGBA32F)
    assert wrote == 3 and np.array_equal(out[winner < 0], under[winner < 0])
    k = np.float32(1.0) - np.float32(0.5)
    assert np.array_equal(out[2, 2], (k * under[2, 2].astype(np.float64) + np.array(col)).astype(np.float32))     # (a half: the fma is exact here)
    out, wrote = MC.resolve(pkg, under, winner, zw, "cd", Cd, E.TARGET_RGBA32F)
    assert wrote == 3 and np.array_equal(out[2, 2], np.float32([1.0, 0.5, 0.25, 1.0])) and np.array_equal(out[5, 7], np.float32([0.0, 0.125, 1.0, 1.0]))
    # the depth test: zw <= depth + bias, on the winner
    depth = np.full((6, 8), 0.375, np.float32)
    out, wrote = MC.resolve(pkg, under, winner, zw, "cd", Cd, E.TARGET_RGBA32F, depth=depth)
    assert wrote == 2 and np.array_equal(out[2, 2], under[2, 2]) and np.array_equal(out[2, 4], np.float32([0.0, 0.125, 1.0, 1.0]))
    out, wrote = MC.resolve(pkg, under, winner, zw, "cd", Cd, E.TARGET_RGBA32F, depth=depth, bias=0.125)
    assert wrote == 3
    # packed formats: decoded, composited, stored; unwritten pixels keep their bytes
    for fmt in (E.TARGET_RGBA16F, E.TARGET_RGBA8):
        u = MC.frame_under(pkg, 8, 6, fmt)
        out, wrote = MC.resolve(pkg, u, winner, zw, (0.0, 0.0, 0.0, 1.0), Cd, fmt)
        assert out.dtype == u.dtype and wrote == 3 and np.array_equal(out[winner < 0], u[winner < 0])
        assert np.array_equal(out[2, 2], E.convert_pixels(np.float32([0, 0, 0, 1]), fmt))
        out, _ = MC.resolve(pkg, u, winner, zw, (0.0, 0.0, 0.0, 0.0), Cd, fmt)
        assert np.array_equal(out, u), "a transparent mark over a decoded pixel does not give the pixel back"


def test_the_cases_hold_what_they_claim(pkg):
    """the seeded splats landed where the table says: in the edge pixels, in the corners, one pixel outside; the twins share a pixel
    and a depth; every size is there in both frames"""
    for n in MC.SIZES:
        for wh in MC.FRAMES:
            c = MC.case(pkg, n, wh)
            w, h = wh
            assert c.n == n
            hit, ctr = MC.dot_centres(pkg, c, any_opacity=True)
            if n < 31:
                assert hit.all() and 0 <= ctr[0, 0] < w and 0 <= ctr[0, 1] < h
                continue
            at = c.specials
            q = lambda label: (int(np.floor(ctr[at[label], 0])), int(np.floor(ctr[at[label], 1])))
            assert q("left")[0] == 0 and q("right")[0] == w - 1 and q("bottom")[1] == 0 and q("top")[1] == h - 1, c
            assert (q("corner00"), q("corner10"), q("corner01"), q("corner11")) == ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)), c
            assert q("out_left")[0] == -1 and q("out_right")[0] == w and q("out_bottom")[1] == -1 and q("out_top")[1] == h, c
            assert all(hit[at[k]] for k in MC.SPECIALS), c
            assert np.array_equal(ctr[at["twin_lo"]].view(np.uint32), ctr[at["twin_hi"]].view(np.uint32)) and at["twin_lo"] < at["twin_hi"]
            plain, _ = MC.dot_centres(pkg, c)
            assert not plain[at["below_255"]] and not plain[at["zero_opacity"]] and hit[at["below_255"]] and hit[at["zero_opacity"]]
            assert plain.sum() > n // 2
