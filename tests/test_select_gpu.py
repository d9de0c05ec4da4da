"""Selection on the GPU (gsr_select): resident splats picked by screen region -- a rect, a painted image, a depth test.

Everything is BIT-EXACT, so there are no tolerances.  What a mask must hold comes from gsr_select_eval (the rule on the host), the numpy
restatement of the op and a random prior mask with garbage behind n -- never from the GPU path.  The cases are select_cases.py's; each
runs under both GSR_OPT_STORAGE_ORDER values."""
import ctypes as C

import numpy as np
import pytest

import select_cases as SC
import test_move_gpu as M
from helpers import HipBuffers

GSR_E_INVALID = -1
GUARD = 16                   # words on either side of every mask
FILL = 0xA5A5A5A5
NAMES = SC.case_names()


def _guarded(words):
    return np.concatenate([np.full(GUARD, FILL, np.uint32), words.astype(np.uint32), np.full(GUARD, FILL, np.uint32)])


def _select_raw(pkg, eng, hb, cam_struct, region, prior_words, device):
    """gsr_select through the C ABI into a guarded mask that holds prior_words, in device or host memory -> (words, n_hit, n_set);
    asserts that the guard words in front of and behind the destination are unchanged"""
    L = pkg.load_library()
    r = region[0] if isinstance(region, tuple) else region
    buf = _guarded(prior_words)
    hit, nset = C.c_int64(-1), C.c_int64(-1)
    if device:
        base = hb.upload(buf)
        rc = L.gsr_select(eng.h, C.byref(cam_struct), C.byref(r), C.c_void_p(base + 4 * GUARD), 1, C.byref(hit), C.byref(nset))
        out = hb.download(base, buf.shape, np.uint32)
    else:
        out = buf.copy()
        rc = L.gsr_select(eng.h, C.byref(cam_struct), C.byref(r), out.ctypes.data + 4 * GUARD, 0, C.byref(hit), C.byref(nset))
    assert rc == 0, L.gsr_last_error()
    assert (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all(), "a guard word changed"
    return out[GUARD:-GUARD], hit.value, nset.value


def _check(pkg, eng, hb, case, cam_struct, want_hit, prior, words, label, **region_kw):
    """every op, into a device mask and into a host mask"""
    E = pkg.engine
    for op in range(5):
        want = SC.apply_op(op, prior, want_hit)
        for device in (True, False):
            got, n_hit, n_set = _select_raw(pkg, eng, hb, cam_struct, case.region(pkg, op=op, **region_kw), words, device)
            tag = f"{label} op {SC.OPS[op]} {'device' if device else 'host'} mask"
            assert np.array_equal(got, E.pack_mask(want)), tag          # (pack_mask leaves the bits at and behind n clear)
            assert (n_hit, n_set) == (int(want_hit.sum()), int(want.sum())), (tag, n_hit, n_set)


# ---- 1. per case and op ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_masks_per_case_and_op(pkg, name, order):
    E = pkg.engine
    c = SC.case(pkg, name)
    cs = E.camera_struct(c.cam)
    prior, words = SC.prior_words(pkg, c.n, 40 + c.n)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats, c.origin)
            want = c.eval(pkg)
            _check(pkg, U, hb, c, cs, want, prior, words, name)
            sel = U.get_select()
            assert sel["selects"] == 10 and sel["hit_last"] == int(want.sum()) and sel["ms"][0] > 0.0 and sel["ms"][3] >= sel["ms"][0], sel
            # each of image and depth alone, from host memory and from device memory
            d_image, d_depth = hb.upload(E.pack_image(c.image)), hb.upload(c.depth)
            for kw, dev in (({"image": True, "depth": False}, {"image_device": d_image}), ({"image": False, "depth": True}, {"depth_device": d_depth})):
                want_k = c.eval(pkg, **kw)
                assert c.n == 1 or not np.array_equal(want_k, want), "the clause left out changes nothing: the case tests nothing"
                for source, region in (("host", c.region(pkg, **kw)), ("device", c.region(pkg, image=False, depth=False, **dev))):
                    for device in (True, False):
                        got, n_hit, n_set = _select_raw(pkg, U, hb, cs, region, words, device)
                        assert np.array_equal(got, E.pack_mask(want_k)) and n_hit == n_set == int(want_k.sum()), (name, kw, source, device)
            # the Python door: Engine.select and Engine.select_device
            mask, n_hit, n_set = U.select(c.cam, c.region(pkg, op=E.SELECT_TOGGLE), prior)
            assert np.array_equal(mask, prior ^ want) and (n_hit, n_set) == (int(want.sum()), int((prior ^ want).sum()))
            mask, n_hit, n_set = U.select(c.cam, c.region(pkg))
            assert np.array_equal(mask, want)
            dm = hb.upload(words)
            assert U.select_device(c.cam, c.region(pkg, op=E.SELECT_ADD, image=False, depth=False, image_device=d_image, depth_device=d_depth), dm) == \
                (int(want.sum()), int((prior | want).sum()))
            assert np.array_equal(hb.download(dm, words.shape, np.uint32), E.pack_mask(prior | want))
    finally:
        hb.free()


# ---- 2. under a visibility in force ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, order):
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    cs = E.camera_struct(c.cam)
    volumes = [E.crop_box((0.1, 0, 0), 0.8)]
    hide = np.arange(c.n) % 3 == 0
    vis = E.visibility_eval(E.visibility_struct(volumes, hide)[0], c.splats.P).astype(bool)
    resident = np.where(vis, c.splats.alpha, np.float32(0.0)).astype(np.float32)
    plain, hidden_too = c.eval(pkg, opacity=resident), c.eval(pkg, opacity=resident, any_opacity=True)
    assert (c.eval(pkg) & ~vis).any(), "no hidden splat would have been hit: the case tests nothing"
    assert not (plain & ~vis).any() and (hidden_too & ~vis).any() and plain.any()
    prior, words = SC.prior_words(pkg, c.n, 77)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats, c.origin)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA = U.debug_resident(E.RESIDENT_GEOA)
            _check(pkg, U, hb, c, cs, plain, prior, words, "hidden splats are not hit")
            _check(pkg, U, hb, c, cs, hidden_too, prior, words, "GSR_SELECT_ANY_OPACITY hits them", any_opacity=True)
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA) and U.get_visibility()[1] == int((~vis).sum())
            U.set_visibility()
            _check(pkg, U, hb, c, cs, c.eval(pkg), prior, words, "the visibility cleared")
    finally:
        hb.free()


# ---- 3. after a remove and an add: the new index space -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_after_remove_and_add(pkg):
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    cs = E.camera_struct(c.cam)
    gone = np.random.default_rng(8).random(c.n) < 0.3
    extra = M._cloud(pkg, 21, n=101)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(c.splats, c.origin)
            s = c.splats.subset(~gone)
            assert U.remove(gone) == s.n
            for label, cloud in (("after a remove", s), ("after an add", None)):
                if cloud is None:
                    cloud = s.concat(extra)
                    assert U.add(extra) == cloud.n
                want = E.select_eval(c.cam, c.origin, c.region(pkg), cloud.P, cloud.alpha)
                assert 0 < want.sum() < cloud.n and (cloud.n + 31) // 32 != (c.n + 31) // 32
                prior, words = SC.prior_words(pkg, cloud.n, 5)
                for op in (E.SELECT_REPLACE, E.SELECT_TOGGLE):
                    for device in (True, False):
                        got, n_hit, n_set = _select_raw(pkg, U, hb, cs, c.region(pkg, op=op), words, device)
                        m = SC.apply_op(op, prior, want)
                        assert np.array_equal(got, E.pack_mask(m)) and (n_hit, n_set) == (int(want.sum()), int(m.sum())), (label, op, device)
    finally:
        hb.free()


# ---- 4. against the frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("n357_persp", "n357_offcentre_origin", NAMES[-2]))
def test_against_the_frame_s_records(pkg, name):
    E = pkg.engine
    c = SC.case(pkg, name)
    with pkg.Engine(0) as U:
        U.upload(c.splats, c.origin)
        U.render(c.cam)
        rec = U.debug_records(c.n)
        mask, n_hit, _ = U.select(c.cam, c.region(pkg, rect=None, image=False, depth=False))
    vis = rec["visible"] == 1
    assert vis.sum() > c.n // 2
    _, centre = c.eval(pkg, centres=True, rect=None, image=False, depth=False)
    assert np.array_equal(rec["cx"][vis].view(np.uint32), centre[vis, 0].view(np.uint32)), "cx"
    assert np.array_equal(rec["cy"][vis].view(np.uint32), centre[vis, 1].view(np.uint32)), "cy"
    assert mask[vis].all(), "a record the frame drew is not in the everywhere-rect selection"
    assert n_hit == int(mask.sum()) < c.n


# ---- 5. nothing is invalidated ---------------------------------------------------------------------------------------------------------------
KEPT = ("uploads", "moves", "upload_ms", "move_ms")


@pytest.mark.gpu
def test_a_select_keeps_the_cached_order(pkg):
    c = SC.case(pkg, "n357_persp")
    with pkg.Engine(0) as U:
        U.upload(c.splats, c.origin)
        frame = U.render(c.cam).copy()
        U.render(c.cam)
        st = U.stats()
        assert st["sorts_skipped"] >= 1
        planes = M._planes(U)
        assert np.array_equal(U.select(c.cam, c.region(pkg))[0], c.eval(pkg))
        again = U.render(c.cam)
        st2 = U.stats()
        assert st2["sorts_skipped"] == st["sorts_skipped"] + 1, "the select invalidated the cached depth order"
        assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
        for k in KEPT:
            assert st2[k] == st[k], (k, st[k], st2[k])
        M._assert_same_planes(M._planes(U), planes, "a select between frames")


@pytest.mark.gpu
def test_a_select_keeps_the_depth_horizons(pkg):
    """a cloud that fills the frame, culled against the previous frame's horizons (the scene of test_read_gpu): the frames around a
    select are culled as those of a context that never selects, none is repaired, and gsr_get_stats is otherwise the same"""
    E = pkg.engine
    s = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    s.alpha[:] = 0.97
    cams = [pkg.camera.make_camera(200, 120, sh_order=3, frame=180 + k, step_deg=0.25, distance=2.2) for k in range(6)]
    region = E.select_region((40.5, 30.25, 120.0, 90.75))
    want = E.select_eval(cams[3], (0, 0, 0), region, s.P, s.alpha)
    assert 1000 < want.sum() < s.n - 1000

    def run(select):
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_OCCLUSION_CULL, 2)
            U.upload(s)
            out, stats = [], []
            for k, cam in enumerate(cams):
                if select and k == 3:
                    mask, n_hit, n_set = U.select(cam, region)
                    assert np.array_equal(mask, want) and n_hit == n_set == int(want.sum())
                out.append(U.render(cam).copy())
                stats.append(U.stats())
            return out, stats

    base, st0 = run(False)
    got, st1 = run(True)
    print("frames_culled", [t["frames_culled"] for t in st0], [t["frames_culled"] for t in st1], "repaired", st0[-1]["frames_repaired"], st1[-1]["frames_repaired"])
    assert st0[2]["frames_culled"] >= 1, "no frame was culled before the select: the case tests nothing"
    assert [t["frames_culled"] for t in st1] == [t["frames_culled"] for t in st0]
    assert [t["frames_repaired"] for t in st1] == [t["frames_repaired"] for t in st0]
    assert st1[-1]["frames_culled"] > st1[2]["frames_culled"], "culling stopped at the select"
    for k, v in st0[-1].items():                                        # every counter (the clocks, floats, differ between any two runs)
        if isinstance(v, int):
            assert st1[-1][k] == v, (k, v, st1[-1][k])
    for k in KEPT:
        assert st1[-1][k] == st1[0][k], k
    for k in range(len(cams)):
        assert np.array_equal(got[k], base[k]), k


# ---- 6. composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_select_then_remove_from_the_device_mask(pkg, order):
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    want = c.eval(pkg)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats, c.origin)
            dm = hb.upload(np.full((c.n + 31) // 32, 0xffffffff, np.uint32))
            assert U.select_device(c.cam, c.region(pkg), dm) == (int(want.sum()), int(want.sum()))
            assert U.remove_device(dm) == int((~want).sum())            # nothing crossed the link in between
            got = M._planes(U)
        M._assert_same_planes(got, M._fresh_planes(pkg, c.splats.subset(~want), order, True, c.origin), f"select + remove, order {order}")
    finally:
        hb.free()


@pytest.mark.gpu
def test_select_then_set_visibility(pkg):
    c = SC.case(pkg, "n357_persp")
    want = c.eval(pkg)
    cams = [c.cam, pkg.camera.make_camera(c.cam.width, c.cam.height, sh_order=3, frame=9, near=0.01, far=50.0)]
    with pkg.Engine(0) as U:
        U.upload(c.splats, c.origin)
        before = U.render(cams[0]).copy()
        mask, _, _ = U.select(c.cam, c.region(pkg))
        U.set_visibility(mask=mask)
        got = [U.render(cam).copy() for cam in cams]
    zeroed = M._copy(pkg, c.splats)
    zeroed.alpha[want] = 0.0
    fresh = M._fresh_frames(pkg, zeroed, cams, origin=c.origin)
    assert not np.array_equal(before, got[0]), "hiding the selection changed nothing: the case tests nothing"
    for k in range(len(cams)):
        assert np.array_equal(got[k].view(np.uint32), fresh[k].view(np.uint32)), k


# ---- 7. refusals, with nothing written ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    E, L = pkg.engine, pkg.load_library()
    c = SC.case(pkg, "n357_persp")
    cs = E.camera_struct(c.cam)
    w, h, words = c.cam.width, c.cam.height, (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.upload(np.full(size // 4, FILL, np.uint32))
        host_mask = np.full(words + 2, FILL, np.uint32)
        cnt = [C.c_int64(-7), C.c_int64(-7)]
        pageable = np.full(w * h, FILL, np.uint32)
        ok, _ = E.select_region(None)

        def region(**kw):
            r, _ = E.select_region(None)
            for k, v in kw.items():
                setattr(r, k, v)
            return r

        def call(eng, cam=cs, reg=ok, mask=room, device=1):
            return L.gsr_select(eng.h, C.byref(cam) if cam is not None else None, C.byref(reg) if reg is not None else None,
                                C.c_void_p(mask) if mask is not None else None, device, C.byref(cnt[0]), C.byref(cnt[1]))

        def cam_with(**kw):
            s = E.camera_struct(c.cam)
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()                    # before any upload
            assert call(U, mask=host_mask.ctypes.data, device=0) == GSR_E_INVALID
            U.upload(c.splats, c.origin)
            frame = U.render(c.cam).copy()
            U.render(c.cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            short_mask = room + size - (words * 4 - 4)                  # one word short of the end of its allocation
            short_image = room + size - (((w * h + 31) // 32) * 4 - 4)
            short_depth = room + size - (w * h * 4 - 4)
            cases = {
                "NULL camera": lambda: call(U, cam=None), "NULL region": lambda: call(U, reg=None), "NULL mask": lambda: call(U, mask=None),
                "op 5": lambda: call(U, reg=region(op=5)), "op -1": lambda: call(U, reg=region(op=-1)),
                "flags 2": lambda: call(U, reg=region(flags=2)), "reserved_ 1": lambda: call(U, reg=region(reserved_=1)),
                "width 0": lambda: call(U, cam=cam_with(width=0)), "height 0": lambda: call(U, cam=cam_with(height=0)),
                "width too large": lambda: call(U, cam=cam_with(width=E.MAX_DIM + 1)), "height < 0": lambda: call(U, cam=cam_with(height=-1)),
                "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, device=1),
                "misaligned mask": lambda: call(U, mask=room + 2),
                "mask past its allocation": lambda: call(U, mask=short_mask),
                "pageable image": lambda: call(U, reg=region(image=pageable.ctypes.data, image_is_device=1)),
                "image past its allocation": lambda: call(U, reg=region(image=short_image, image_is_device=1)),
                "pageable depth": lambda: call(U, reg=region(depth=pageable.ctypes.data, depth_is_device=1)),
                "depth past its allocation": lambda: call(U, reg=region(depth=short_depth, depth_is_device=1)),
                "host mask, pageable device depth": lambda: call(U, reg=region(depth=pageable.ctypes.data, depth_is_device=1), mask=host_mask.ctypes.data, device=0),
            }
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_select" in L.gsr_last_error(), label
                assert np.array_equal(U.render(c.cam), frame), label
                assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
            M._assert_same_planes(M._planes(U), planes, "refusals")
            assert cnt[0].value == -7 and cnt[1].value == -7 and (host_mask == FILL).all() and (pageable == FILL).all()
            assert (hb.download(room, (size // 4,), np.uint32) == FILL).all(), "a refused select wrote to device memory"
            assert U.get_select() == {"selects": 0, "hit_last": 0, "ms": [0.0] * 4}
            assert L.gsr_get_select(U.h, None, None, None) == 0         # every pointer may be NULL
            # either count may be NULL
            assert L.gsr_select(U.h, C.byref(cs), C.byref(ok), C.c_void_p(room), 1, None, None) == 0 and U.get_select()["selects"] == 1
            # an upload in progress
            assert L.gsr_upload_begin(U.h, c.n, 1, None) == 0
            assert call(U) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_upload_abort(U.h) == 0
            # the empty cloud: GSR_OK, nothing written, both counts 0
            U.upload(c.splats, c.origin)
            assert U.remove(np.ones(c.n, bool)) == 0
            assert call(U, mask=host_mask.ctypes.data, device=0) == 0 and cnt[0].value == 0 and cnt[1].value == 0 and (host_mask == FILL).all()
            mask, n_hit, n_set = U.select(c.cam, E.select_region(None))
            assert mask.shape == (0,) and (n_hit, n_set) == (0, 0)
    finally:
        hb.free()


# ---- 8. several ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_select(pkg):
    E = pkg.engine
    c = SC.case(pkg, "n357_persp")
    prior, _ = SC.prior_words(pkg, c.n, 9)
    with pkg.Engine(0) as U:
        U.upload(c.splats, c.origin)
        single = [U.select(c.cam, c.region(pkg, op=op), prior) for op in range(5)]
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(c.splats, c.origin)
        Mu.render(c.cam)
        for op in range(5):
            mask, n_hit, n_set = Mu.select(c.cam, c.region(pkg, op=op), prior)
            want = SC.apply_op(op, prior, c.eval(pkg))
            assert np.array_equal(mask, want) and np.array_equal(mask, single[op][0]) and (n_hit, n_set) == single[op][1:], op
        assert [Mu.stats(r)["n_splats"] for r in range(2)] == [c.n, c.n]
