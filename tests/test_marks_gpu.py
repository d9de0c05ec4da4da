"""The selection overlay on the GPU (gsr_render_marks): the splats a mask selects drawn into a finished frame as dots or outlines.

Everything is BIT-EXACT, so there are no tolerances.  What a frame must hold comes from marks_cases.py's models -- gsr_select_eval's
centres and a per-pixel minimum in numpy (dots), the oracle's wire overlay of the subset (outlines), gsr_composite_over and
gsr_convert_pixels (the resolve step) -- never from the GPU path.  Clouds at the word, wave and workgroup edges, frames 64 x 48 and
37 x 29, both GSR_OPT_STORAGE_ORDER values."""
import ctypes as C

import numpy as np
import pytest

import marks_cases as MC
from helpers import HipBuffers, load_golden

GSR_E_INVALID = -1
GUARD = 64                   # bytes in front of and behind every device frame and mask
FILL = 0xA5
YELLOW = (1.0, 1.0, 0.0, 1.0)
VEIL = (0.5, 0.25, 0.0, 0.5)         # translucent, premultiplied


def _draw(pkg, eng, hb, cam, mask, style, under, mask_device=False, target_device=False, garbage=True):
    """gsr_render_marks through the C ABI.  mask: bool (n,) or None; host or device memory on either side, device buffers between guard
    bytes that must not change -> (image, pixels written)"""
    E, L = pkg.engine, pkg.load_library()
    st = style[0] if isinstance(style, tuple) else style
    cs = E.camera_struct(cam)
    wrote = C.c_int64(-1)
    words = None if mask is None else (MC.words_with_garbage(pkg, mask) if garbage else E.pack_mask(mask))
    guard = np.full(GUARD, FILL, np.uint8)
    mptr = None
    if words is not None:
        mptr = hb.upload(np.concatenate([guard, words.view(np.uint8), guard])) + GUARD if mask_device else words.ctypes.data
    out = np.ascontiguousarray(under).copy()
    if target_device:
        base = hb.upload(np.concatenate([guard, out.reshape(-1).view(np.uint8), guard]))
        rc = L.gsr_render_marks(eng.h, C.byref(cs), C.c_void_p(mptr) if mptr else None, int(mask_device), C.byref(st), C.c_void_p(base + GUARD), 1, C.byref(wrote))
        back = hb.download(base, (2 * GUARD + out.nbytes,), np.uint8)
        assert (back[:GUARD] == FILL).all() and (back[-GUARD:] == FILL).all(), "a guard byte of the device frame changed"
        out = back[GUARD:-GUARD].view(out.dtype).reshape(out.shape).copy()
    else:
        rc = L.gsr_render_marks(eng.h, C.byref(cs), C.c_void_p(mptr) if mptr else None, int(mask_device), C.byref(st), out.ctypes.data, 0, C.byref(wrote))
    assert rc == 0, L.gsr_last_error()
    if words is not None and mask_device:
        back = hb.download(mptr - GUARD, (2 * GUARD + words.nbytes,), np.uint8)
        assert np.array_equal(back, np.concatenate([guard, words.view(np.uint8), guard])), "the verb wrote to the mask"
    return out, wrote.value


def _same(got, want, label):
    g, w = got, want
    assert w[1] == g[1], (label, "n_pixels", g[1], w[1])
    assert np.array_equal(g[0].view(np.uint8), w[0].view(np.uint8)), (label, int((g[0] != w[0]).any(-1).sum()), "pixels differ")


def _engine(pkg, case, order, fmt=None):
    E = pkg.engine
    U = pkg.Engine(0)
    U.set_option(E.OPT_STORAGE_ORDER, order)
    if fmt is not None:
        U.set_target_format(fmt)
    U.upload(case.splats, case.origin)
    return U


# ---- 1. dots: every size, both frames, every radius, every kind of mask ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("n", MC.SIZES)
def test_dots(pkg, n, order):
    E = pkg.engine
    fmt = E.TARGET_RGBA32F
    hb = HipBuffers()
    try:
        for wh in MC.FRAMES:
            c = MC.case(pkg, n, wh)
            under = MC.frame_under(pkg, wh[0], wh[1], fmt, seed=n)
            with _engine(pkg, c, order) as U:
                drawn_any = 0
                for label, m in MC.masks(pkg, n, n + order).items():
                    marked = np.ones(n, bool) if m is None else m
                    for radius in MC.RADII:
                        for colour in (VEIL, "cd"):
                            want = MC.expected_dots(pkg, c, under, marked, radius, colour, fmt)
                            style = E.mark_style(E.MARK_DOT, radius, colour)
                            sides = ((False, False), (True, True)) if label != "random" else ((False, False), (True, False), (False, True), (True, True))
                            for md, td in sides:
                                _same(_draw(pkg, U, hb, c.cam, m, style, under, md, td), want, (c, label, radius, colour, md, td))
                            drawn_any += want[1]
                    if label == "all_clear":
                        assert want[1] == 0 and np.array_equal(want[0], under)
                assert drawn_any > 0, "nothing was ever drawn: the case tests nothing"
                # the Python door
                m = MC.masks(pkg, n, n + order)["random"]
                want = MC.expected_dots(pkg, c, under, m, 1, YELLOW, fmt)
                _same(U.render_marks(c.cam, m, E.mark_style(E.MARK_DOT, 1, YELLOW), under), want, (c, "render_marks"))
                d_under, d_mask = hb.upload(under), hb.upload(E.pack_mask(m))
                assert U.render_marks_device(c.cam, d_mask, E.mark_style(E.MARK_DOT, 1, YELLOW), d_under) == want[1]
                assert np.array_equal(hb.download(d_under, under.shape), want[0])
                got = U.get_marks()
                assert got["calls"] > 0 and got["pixels_last"] == want[1] and got["ms"][3] >= got["ms"][0] > 0.0, got
    finally:
        hb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_of_two_splats_at_one_position_the_lower_upload_index_shows(pkg, order):
    E = pkg.engine
    c = MC.case(pkg, 300, MC.FRAMES[0])
    lo, hi = c.specials["twin_lo"], c.specials["twin_hi"]
    only = np.zeros(c.n, bool)
    only[[lo, hi]] = True
    under = MC.frame_under(pkg, *MC.FRAMES[0], E.TARGET_RGBA32F)
    hb = HipBuffers()
    try:
        with _engine(pkg, c, order) as U:
            for radius in MC.RADII:
                got, wrote = _draw(pkg, U, hb, c.cam, only, E.mark_style(E.MARK_DOT, radius, "cd"), under)
                written = (got != under).any(-1)
                assert wrote == written.sum() > 0
                cd = np.append(c.splats.Cd[lo].view(np.float16).astype(np.float32), np.float32(1.0))
                assert (got[written] == cd).all(), radius
                only_hi = np.zeros(c.n, bool)
                only_hi[hi] = True
                got_hi, _ = _draw(pkg, U, hb, c.cam, only_hi, E.mark_style(E.MARK_DOT, radius, "cd"), under)
                assert np.array_equal((got_hi != under).any(-1), written) and not np.array_equal(got_hi, got)
    finally:
        hb.free()


# ---- 2. a translucent and an opaque colour in all three target formats ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", ("RGBA32F", "RGBA16F", "RGBA8"))
def test_dots_and_outlines_in_every_target_format(pkg, oracle, fmt_name):
    E = pkg.engine
    fmt = getattr(E, "TARGET_" + fmt_name)
    hb = HipBuffers()
    try:
        for n, wh in ((257, MC.FRAMES[1]), (300, MC.FRAMES[0])):
            c = MC.case(pkg, n, wh)
            m = MC.masks(pkg, n, 7)["random"]
            under = MC.frame_under(pkg, wh[0], wh[1], fmt, seed=3)
            with _engine(pkg, c, 1, fmt) as U:
                for colour in (VEIL, YELLOW, "cd", (0.0, 0.0, 0.0, 0.0)):
                    for td in (False, True):
                        want = MC.expected_dots(pkg, c, under, m, 1, colour, fmt)
                        _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_DOT, 1, colour), under, td, td), want, (c, fmt_name, colour, td, "dots"))
                        want = MC.expected_outlines(pkg, oracle, c, under, m, colour, fmt)
                        _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_OUTLINE, 0, colour), under, td, td), want, (c, fmt_name, colour, td, "outlines"))
    finally:
        hb.free()


# ---- 3. radius 0 is gsr_select's pixel ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_radius_0_dots_lie_on_the_centre_pixels_select_hits(pkg, order):
    E = pkg.engine
    for n, wh in ((300, MC.FRAMES[0]), (257, MC.FRAMES[1])):
        c = MC.case(pkg, n, wh)
        w, h = wh
        prior = MC.masks(pkg, n, 5)["random"]
        _, ctr = MC.dot_centres(pkg, c, any_opacity=True)
        zs = ctr[~np.isnan(ctr[:, 2]), 2]
        depth = np.random.default_rng(n).uniform(zs.min(), zs.max(), (h, w)).astype(np.float32)
        under = MC.frame_under(pkg, w, h, E.TARGET_RGBA32F)
        with _engine(pkg, c, order) as U:
            for kw in ({}, {"depth": depth, "depth_bias": 2.0 ** -20}):
                sel, n_hit, n_set = U.select(c.cam, E.select_region((0.0, 0.0, float(w), float(h)), op=E.SELECT_INTERSECT, **kw), prior)
                _, cs = MC.dot_centres(pkg, c)
                pixels = np.zeros((h, w), bool)
                pixels[cs[sel, 1].astype(np.int64), cs[sel, 0].astype(np.int64)] = True
                got, wrote = U.render_marks(c.cam, prior, E.mark_style(E.MARK_DOT, 0, YELLOW, **kw), under)
                assert 0 < pixels.sum() == wrote and np.array_equal((got != under).any(-1), pixels), (c, sorted(kw))
                assert kw == {} or wrote < U.render_marks(c.cam, prior, E.mark_style(E.MARK_DOT, 0, YELLOW), under)[1], "the depth clause hid nothing"


# ---- 4. the depth test ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_the_depth_test(pkg, oracle, order):
    E = pkg.engine
    fmt = E.TARGET_RGBA32F
    hb = HipBuffers()
    try:
        for n, wh in ((300, MC.FRAMES[0]), (255, MC.FRAMES[1])):
            c = MC.case(pkg, n, wh)
            w, h = wh
            m = MC.masks(pkg, n, 11)["random"]
            under = MC.frame_under(pkg, w, h, fmt)
            _, ctr = MC.dot_centres(pkg, c, any_opacity=True)
            zs = ctr[~np.isnan(ctr[:, 2]), 2]
            depth = np.random.default_rng(n).uniform(zs.min(), zs.max(), (h, w)).astype(np.float32)
            halves = np.where(np.arange(w)[None, :] < w // 2, np.float32(-1.0), np.float32(1.0)) * np.ones((h, 1), np.float32)
            with _engine(pkg, c, order) as U:
                for bias in (0.0, 2.0 ** -12, -(2.0 ** -12)):
                    for radius in (0, 8):
                        want = MC.expected_dots(pkg, c, under, m, radius, VEIL, fmt, depth=depth, bias=bias)
                        free = MC.expected_dots(pkg, c, under, m, radius, VEIL, fmt)
                        assert 0 < want[1] < free[1], "the depth buffer decides nothing: the case tests nothing"
                        _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_DOT, radius, VEIL, depth=depth, depth_bias=bias), under), want, (c, bias, radius, "host depth"))
                        style = E.mark_style(E.MARK_DOT, radius, VEIL, depth_device=hb.upload(depth), depth_bias=bias)
                        _same(_draw(pkg, U, hb, c.cam, m, style, under, True, True), want, (c, bias, radius, "device depth"))
                # outlines under -1 | 1: the left half is the frame, the right half the untested overlay
                free = _draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_OUTLINE, 0, "cd"), under)
                _same(free, MC.expected_outlines(pkg, oracle, c, under, m, "cd", fmt), (c, "untested outlines"))
                for td, style in ((False, E.mark_style(E.MARK_OUTLINE, 0, "cd", depth=halves)), (True, E.mark_style(E.MARK_OUTLINE, 0, "cd", depth_device=hb.upload(halves)))):
                    got, wrote = _draw(pkg, U, hb, c.cam, m, style, under, td, td)
                    assert np.array_equal(got[:, :w // 2], under[:, :w // 2]) and np.array_equal(got[:, w // 2:], free[0][:, w // 2:])
                    assert 0 < wrote == (free[0] != under).any(-1)[:, w // 2:].sum() < free[1]
    finally:
        hb.free()


# ---- 5. outlines ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("n", MC.SIZES)
def test_outlines(pkg, oracle, n, order):
    E = pkg.engine
    fmt = E.TARGET_RGBA32F
    hb = HipBuffers()
    try:
        for wh in MC.FRAMES:
            c = MC.case(pkg, n, wh)
            under = MC.frame_under(pkg, wh[0], wh[1], fmt, seed=n)
            with _engine(pkg, c, order) as U:
                drawn_any = 0
                for label, m in MC.masks(pkg, n, n + order).items():
                    marked = np.ones(n, bool) if m is None else m
                    for colour in ("cd", VEIL):
                        for any_opacity in (False, True):
                            want = MC.expected_outlines(pkg, oracle, c, under, marked, colour, fmt, any_opacity=any_opacity)
                            style = E.mark_style(E.MARK_OUTLINE, 0, colour, any_opacity=any_opacity)
                            for md, td in ((False, False), (True, True)):
                                _same(_draw(pkg, U, hb, c.cam, m, style, under, md, td), want, (c, label, colour, any_opacity, md, td))
                            drawn_any += want[1]
                assert drawn_any > 0, "nothing was ever drawn: the case tests nothing"
                # every splat, whatever its opacity: the wire-over display's bytes
                got, wrote = _draw(pkg, U, hb, c.cam, None, E.mark_style(E.MARK_OUTLINE, 0, "cd", any_opacity=True), under)
                assert np.array_equal(got, U.render_wire_over(c.cam, under)) and wrote == (U.render_wire(c.cam)[..., 3] > 0).sum()
    finally:
        hb.free()


@pytest.mark.gpu
def test_outlines_on_the_golden_wire_scene(pkg, oracle):
    E = pkg.engine
    d, s, cam = load_golden("w1_wire")
    c = MC.Case("w1_wire", s, cam, (0.0, 0.0, 0.0), {})
    m = np.random.default_rng(41).random(s.n) < 0.5
    under = MC.frame_under(pkg, cam.width, cam.height, E.TARGET_RGBA32F)
    hb = HipBuffers()
    try:
        with _engine(pkg, c, 1) as U:
            want = MC.expected_outlines(pkg, oracle, c, under, m, "cd", E.TARGET_RGBA32F)
            assert want[1] > 1000
            _same(_draw(pkg, U, hb, cam, m, E.mark_style(E.MARK_OUTLINE, 0, "cd"), under, True, True), want, "w1_wire, random mask")
            got, _ = _draw(pkg, U, hb, cam, None, E.mark_style(E.MARK_OUTLINE, 0, "cd", any_opacity=True), under)
            assert np.array_equal(got, U.render_wire_over(cam, under))
    finally:
        hb.free()


# ---- 6. under a visibility in force ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, oracle, order):
    E = pkg.engine
    fmt = E.TARGET_RGBA32F
    c = MC.case(pkg, 300, MC.FRAMES[0])
    m = MC.masks(pkg, c.n, 13)["random"]
    volumes = [E.crop_box((0.1, 0, 0), 0.7)]
    vis = E.visibility_eval(E.visibility_struct(volumes)[0], c.splats.P).astype(bool)
    resident = np.where(vis, c.splats.alpha, np.float32(0.0)).astype(np.float32)
    under = MC.frame_under(pkg, *MC.FRAMES[0], fmt)
    hb = HipBuffers()
    try:
        with _engine(pkg, c, order) as U:
            U.set_visibility(volumes=volumes)
            assert U.get_visibility()[1] == int((~vis).sum()) > 0 and (m & ~vis).any()
            for any_opacity in (False, True):
                dots = MC.expected_dots(pkg, c, under, m, 1, "cd", fmt, resident_alpha=resident, any_opacity=any_opacity)
                lines = MC.expected_outlines(pkg, oracle, c, under, m, "cd", fmt, resident_alpha=resident, any_opacity=any_opacity)
                for md in (False, True):
                    _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_DOT, 1, "cd", any_opacity=any_opacity), under, md, md), dots, ("dots", any_opacity, md))
                    _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_OUTLINE, 0, "cd", any_opacity=any_opacity), under, md, md), lines, ("outlines", any_opacity, md))
                if any_opacity:
                    assert dots[1] > hidden_dots and lines[1] > hidden_lines, "the hidden splats add nothing: the case tests nothing"
                    assert not np.array_equal(dots[0], MC.expected_dots(pkg, c, under, m & vis, 1, "cd", fmt, any_opacity=True)[0])
                else:
                    hidden_dots, hidden_lines = dots[1], lines[1]
                    _same(dots, MC.expected_dots(pkg, c, under, m & vis, 1, "cd", fmt), "the model: hidden splats are not drawn")
            U.set_visibility()
            _same(_draw(pkg, U, hb, c.cam, m, E.mark_style(E.MARK_DOT, 1, "cd"), under), MC.expected_dots(pkg, c, under, m, 1, "cd", fmt), "the visibility cleared")
    finally:
        hb.free()


# ---- 7. nothing is disturbed, and refusals write nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_marks_change_and_invalidate_nothing(pkg):
    E = pkg.engine
    c = MC.case(pkg, 300, MC.FRAMES[0])
    m = MC.masks(pkg, c.n, 17)["random"]
    with pkg.Engine(0) as U:
        U.upload(c.splats, c.origin)
        frame = U.render(c.cam).copy()
        U.render(c.cam)
        planes = [U.debug_resident(k).copy() for k in (E.RESIDENT_GEOA,)]
        before = U.stats()
        assert before["sorts_skipped"] >= 1
        for style in (E.mark_style(E.MARK_DOT, 8, VEIL), E.mark_style(E.MARK_OUTLINE, 0, "cd")):
            marked, wrote = U.render_marks(c.cam, m, style, frame)
            assert wrote > 0 and not np.array_equal(marked, frame)
        after = U.stats()
        for k, v in before.items():
            if isinstance(v, int):
                assert after[k] == v, (k, v, after[k])
        again = U.render(c.cam)
        assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
        assert U.stats()["sorts_skipped"] == before["sorts_skipped"] + 1, "the marks invalidated the cached depth order"
        assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), planes[0])
        assert U.get_marks()["calls"] == 2


@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    E, L = pkg.engine, pkg.load_library()
    c = MC.case(pkg, 300, MC.FRAMES[0])
    cs = E.camera_struct(c.cam)
    w, h, words = c.cam.width, c.cam.height, (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20
        room = hb.upload(np.full(size, FILL, np.uint8))
        host_frame = np.full((h, w, 4), 0.25, np.float32)
        host_mask = np.full(words, 0xffffffff, np.uint32)
        pageable = np.full(w * h * 4, 0.5, np.float32)
        wrote = C.c_int64(-7)

        def style(**kw):
            st, _ = E.mark_style()
            for k, v in kw.items():
                if k == "rgba":
                    st.rgba[:] = v
                else:
                    setattr(st, k, v)
            return st

        def cam_with(**kw):
            s = E.camera_struct(c.cam)
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        def call(eng, cam=cs, mask=None, mask_device=0, st=style(), target=room, device=1):
            return L.gsr_render_marks(eng.h, C.byref(cam) if cam is not None else None, C.c_void_p(mask) if mask is not None else None, mask_device,
                                      C.byref(st) if st is not None else None, C.c_void_p(target) if target is not None else None, device, C.byref(wrote))

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()
            U.upload(c.splats, c.origin)
            cases = {
                "NULL camera": lambda: call(U, cam=None), "NULL style": lambda: call(U, st=None), "NULL target": lambda: call(U, target=None),
                "shape 0": lambda: call(U, st=style(shape=0)), "shape 3": lambda: call(U, st=style(shape=3)),
                "radius -1": lambda: call(U, st=style(radius=-1)), "radius 9": lambda: call(U, st=style(radius=9)),
                "outline with a radius": lambda: call(U, st=style(shape=E.MARK_OUTLINE, radius=1)),
                "colour mode 2": lambda: call(U, st=style(colour_mode=2)), "flags 2": lambda: call(U, st=style(flags=2)),
                "reserved_ 1": lambda: call(U, st=style(reserved_=1)),
                "NaN colour": lambda: call(U, st=style(rgba=[0.0, float("nan"), 0.0, 1.0])), "inf colour": lambda: call(U, st=style(rgba=[float("inf"), 0.0, 0.0, 1.0])),
                "alpha 1.5": lambda: call(U, st=style(rgba=[0.0, 0.0, 0.0, 1.5])), "alpha -0.5": lambda: call(U, st=style(rgba=[0.0, 0.0, 0.0, -0.5])),
                "NaN alpha": lambda: call(U, st=style(rgba=[0.0, 0.0, 0.0, float("nan")])),
                "width 0": lambda: call(U, cam=cam_with(width=0)), "height too large": lambda: call(U, cam=cam_with(height=E.MAX_DIM + 1)),
                "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, mask_device=1),
                "misaligned mask": lambda: call(U, mask=room + 2, mask_device=1),
                "mask past its allocation": lambda: call(U, mask=room + size - (words * 4 - 4), mask_device=1),
                "pageable target": lambda: call(U, target=host_frame.ctypes.data, device=1),
                "misaligned target": lambda: call(U, target=room + 4),
                "target past its allocation": lambda: call(U, target=room + size - (w * h * 16 - 16)),
                "pageable depth": lambda: call(U, st=style(depth=pageable.ctypes.data, depth_is_device=1)),
                "depth past its allocation": lambda: call(U, st=style(depth=room + size - (w * h * 4 - 4), depth_is_device=1)),
                "host target, pageable device depth": lambda: call(U, st=style(depth=pageable.ctypes.data, depth_is_device=1), target=host_frame.ctypes.data, device=0),
            }
            for label, fn in cases.items():
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_render_marks" in L.gsr_last_error(), label
            assert wrote.value == -7 and (host_frame == 0.25).all() and (host_mask == 0xffffffff).all() and (pageable == 0.5).all()
            assert (hb.download(room, (size,), np.uint8) == FILL).all(), "a refused call wrote to device memory"
            assert U.get_marks() == {"calls": 0, "pixels_last": 0, "ms": [0.0] * 4}
            assert L.gsr_get_marks(U.h, None, None, None) == 0          # every pointer may be NULL
            # n_pixels may be NULL
            assert L.gsr_render_marks(U.h, C.byref(cs), None, 0, C.byref(style()), C.c_void_p(room), 1, None) == 0 and U.get_marks()["calls"] == 1
            # an upload in progress
            assert L.gsr_upload_begin(U.h, c.n, 1, None) == 0
            assert call(U) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_upload_abort(U.h) == 0
            # the empty cloud: GSR_OK, 0 pixels, the target byte-identical
            U.upload(c.splats, c.origin)
            assert U.remove(np.ones(c.n, bool)) == 0
            assert call(U, target=host_frame.ctypes.data, device=0) == 0 and wrote.value == 0 and (host_frame == 0.25).all()
            got, n_px = U.render_marks(c.cam, None, E.mark_style(E.MARK_OUTLINE, colour="cd"), host_frame)
            assert n_px == 0 and np.array_equal(got, host_frame)
    finally:
        hb.free()


# ---- 8. fuzz ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fuzz_against_the_two_models(pkg, oracle):
    E = pkg.engine
    rng = np.random.default_rng(2024)
    hb = HipBuffers()
    fmts = (E.TARGET_RGBA32F, E.TARGET_RGBA16F, E.TARGET_RGBA8)
    drawn = {E.MARK_DOT: 0, E.MARK_OUTLINE: 0}
    try:
        for it in range(30):
            n, w, h = int(rng.integers(1, 420)), int(rng.integers(5, 90)), int(rng.integers(5, 70))
            cam = pkg.camera.make_camera(w, h, sh_order=3, frame=int(rng.integers(0, 40)), distance=float(rng.uniform(1.2, 3.5)), near=0.01, far=50.0)
            s = pkg.scenes.make_scene(n, seed=500 + it, sh=bool(it % 2), log_scale_range=(-4.0, -1.5))
            s.alpha[rng.random(n) < 0.1] = 0.0
            origin = (0.0, 0.0, 0.0) if it % 3 else tuple(float(x) for x in rng.uniform(-2, 2, 3))
            c = MC.Case(f"fuzz{it}", s, cam, origin, {})
            m = None if it % 7 == 6 else rng.random(n) < rng.choice([0.05, 0.5, 0.95])
            marked = np.ones(n, bool) if m is None else m
            fmt = fmts[it % 3]
            under = MC.frame_under(pkg, w, h, fmt, seed=it)
            shape = E.MARK_DOT if it % 2 else E.MARK_OUTLINE
            colour = "cd" if rng.random() < 0.5 else tuple(float(x) for x in rng.random(4).astype(np.float32))
            any_opacity = bool(rng.random() < 0.5)
            md, td = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
            with _engine(pkg, c, it % 2, fmt) as U:
                if shape == E.MARK_DOT:
                    radius = int(rng.integers(0, E.MARK_MAX_RADIUS + 1))
                    kw = {}
                    if rng.random() < 0.5:
                        kw = {"depth": rng.uniform(0.985, 1.0, (h, w)).astype(np.float32), "bias": float(rng.choice([0.0, 2.0 ** -10, -(2.0 ** -10)]))}
                    want = MC.expected_dots(pkg, c, under, marked, radius, colour, fmt, any_opacity=any_opacity, **kw)
                    style = E.mark_style(shape, radius, colour, any_opacity, kw.get("depth"), kw.get("bias", 0.0))
                else:
                    passes = rng.random((h, w)) < 0.7 if rng.random() < 0.5 else None
                    want = MC.expected_outlines(pkg, oracle, c, under, marked, colour, fmt, any_opacity=any_opacity, depth_pass=passes)
                    style = E.mark_style(shape, 0, colour, any_opacity, None if passes is None else np.where(passes, np.float32(1.0), np.float32(-1.0)))
                _same(_draw(pkg, U, hb, cam, m, style, under, md, td), want, (it, n, w, h, shape, colour, any_opacity, md, td))
                drawn[shape] += want[1]
            hb.free()
        assert drawn[E.MARK_DOT] > 100 and drawn[E.MARK_OUTLINE] > 100, drawn
    finally:
        hb.free()
