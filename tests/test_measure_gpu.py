"""Measuring a selection on the GPU (gsr_measure): counts, bounds, extent, the nine tree sums and histograms of the resident splats a
mask selects.

Everything is BIT-EXACT, so there are no tolerances.  What a result must hold comes from gsr_measure_eval (the rule on the host) over
Engine.read() of the same context -- itself held to the uploaded arrays; test_measure.py holds the eval to the numpy restatement of
measure_cases.py -- never from the GPU path.  Each case runs under both GSR_OPT_STORAGE_ORDER values, from a host mask, a guarded
device mask and NULL."""
import ctypes as C

import numpy as np
import pytest

import measure_cases as MC
import test_move_gpu as M
from helpers import HipBuffers

GSR_E_INVALID = -1
GUARD = 16                   # words on either side of every device mask
FILL = 0xA5A5A5A5
NAMES = MC.case_names()


def _raw(pkg, eng, hb, req, words, how):
    """gsr_measure through the C ABI from `words` in host memory ("host"), in guarded device memory ("device") or from NULL ("null")
    -> the result; asserts that the guard words and the mask itself are unchanged"""
    L, E = pkg.load_library(), pkg.engine
    res = E.gsr_measure_result()
    hist = np.full(max(E._measure_hist_words(req), 1) + 4, FILL, np.uint32)
    hp = hist.ctypes.data if req.n_hist > 0 else None
    if how == "device":
        buf = np.concatenate([np.full(GUARD, FILL, np.uint32), words.astype(np.uint32), np.full(GUARD, FILL, np.uint32)])
        base = hb.upload(buf)
        rc = L.gsr_measure(eng.h, C.c_void_p(base + 4 * GUARD), 1, C.byref(req), C.byref(res), hp)
        assert np.array_equal(hb.download(base, buf.shape, np.uint32), buf), "the device mask or a guard word changed"
    elif how == "host":
        keep = words.copy()
        rc = L.gsr_measure(eng.h, keep.ctypes.data, 0, C.byref(req), C.byref(res), hp)
        assert np.array_equal(keep, words), "the host mask changed"
    else:
        rc = L.gsr_measure(eng.h, None, 0, C.byref(req), C.byref(res), hp)
    assert rc == 0, L.gsr_last_error()
    assert (hist[E._measure_hist_words(req):] == FILL).all(), "a word behind the histograms changed"
    return E._measure_result(req, res, hist)


def _assert_same(got, want, label):
    if not MC.same_result(got, want):
        for f in ("n_selected", "n_measured", "n_extent"):
            assert getattr(got, f) == getattr(want, f), (label, f, getattr(got, f), getattr(want, f))
        for f in ("lo", "hi", "lo_e", "hi_e"):
            assert list(np.asarray(list(getattr(got, f)), np.float32).view(np.uint32)) == list(np.asarray(list(getattr(want, f)), np.float32).view(np.uint32)), \
                (label, f, list(getattr(got, f)), list(getattr(want, f)))
        assert [float(v).hex() for v in got.sum] == [float(v).hex() for v in want.sum], (label, "sum")
        for k, (a, b) in enumerate(zip(got.hist, want.hist)):
            assert np.array_equal(a, b), (label, "hist", k, np.flatnonzero(a != b)[:8].tolist())
        raise AssertionError((label, "the results differ"))


def _read_equals(R, s):
    """Engine.read() of a context holds the uploaded arrays the rule looks at, bit for bit"""
    assert np.array_equal(R.P.view(np.uint32), np.ascontiguousarray(s.P, np.float32).view(np.uint32))
    assert np.array_equal(R.alpha.view(np.uint32), np.ascontiguousarray(s.alpha, np.float32).view(np.uint32))
    assert np.array_equal(R.scale, s.scale) and np.array_equal(R.Cd, s.Cd)


def _eval(pkg, req, R, mask=None, vis=None):
    return pkg.engine.measure_eval(req, R.P, R.alpha, R.scale, R.Cd, mask=mask, vis=vis)


# ---- 1. per case, mask and source ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_results_per_case_and_mask(pkg, name, order):
    E = pkg.engine
    c = MC.case(pkg, name)
    full, counts, moments, rest = MC.request(pkg, 7, MC.HISTS_A), MC.request(pkg, 0, MC.HISTS_B), MC.request(pkg, 4), MC.request(pkg, 3, MC.HISTS_C)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats)
            R = U.read()
            _read_equals(R, c.splats)
            calls = 0
            for mask_name, (sel, words) in c.masks(pkg).items():
                want = _eval(pkg, full, R, words)
                for how in ("host", "device"):
                    _assert_same(_raw(pkg, U, hb, full, words, how), want, f"{name} order {order} mask {mask_name} {how}")
                    calls += 1
                for req in (counts, moments, rest):
                    _assert_same(_raw(pkg, U, hb, req, words, "device"), _eval(pkg, req, R, words), f"{name} order {order} mask {mask_name} what {req.what}")
                    calls += 1
            for req in (full, counts):
                _assert_same(_raw(pkg, U, hb, req, None, "null"), _eval(pkg, req, R), f"{name} order {order} NULL mask what {req.what}")
                calls += 1
            # the Python door: Engine.measure and Engine.measure_device
            sel, words = c.masks(pkg)["random"]
            want = _eval(pkg, full, R, words)
            _assert_same(U.measure(full, sel), want, "Engine.measure, a boolean mask")
            _assert_same(U.measure(full, words), want, "Engine.measure, packed words")
            _assert_same(U.measure(full), _eval(pkg, full, R), "Engine.measure, no mask")
            dm = hb.upload(words)
            got = U.measure_device(full, dm)
            _assert_same(got, want, "Engine.measure_device")
            assert np.array_equal(got.centroid(), want.centroid(), equal_nan=True) and np.array_equal(got.covariance(), want.covariance(), equal_nan=True)
            calls += 4
            # the tallies: get_measure counts the measures, the others count nothing
            t = U.get_measure()
            assert t["measures"] == calls and t["measured_last"] == want.n_measured and t["ms"][0] > 0.0 and t["ms"][3] >= t["ms"][0], t
            assert U.get_select()["selects"] == 0 and U.get_select_attrs()["selects"] == 0 and U.get_read()["reads"] == 1
            assert U.get_transform()["transforms"] == 0
    finally:
        hb.free()


# ---- 2. under a visibility in force ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, order):
    """the ALPHA channel bins the TRUE alpha (a hidden splat's resident opacity is +0); SKIP_HIDDEN drops the hidden splats (volumes and
    mask in force, through gsr_splat_visible); the hidden set stays what it was"""
    E = pkg.engine
    c = MC.case(pkg, "n257_sh")
    s = c.splats
    volumes = [E.crop_box(tuple(float(v) for v in MC.OFFSET + np.float32([0.3, 0.0, 0.0])), 0.8)]
    hide = np.arange(c.n) % 4 == 3
    vis_struct, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(vis_struct, s.P)
    assert (~visible).sum() > 50 and visible.sum() > 50
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA, hidden_count = U.debug_resident(E.RESIDENT_GEOA), U.get_visibility()[1]
            R = U.read()
            _read_equals(R, s)
            for mask_name in ("all", "random", "alt2"):
                sel, words = c.masks(pkg)[mask_name]
                for what, hists in ((7, MC.HISTS_A), (0, MC.HISTS_B), (0, (MC.HISTS_A[0],)), (4, ())):
                    plain, skip = MC.request(pkg, what, hists), MC.request(pkg, what, hists, skip_hidden=True)
                    want_plain, want_skip = _eval(pkg, plain, R, words, vis=vis_struct), _eval(pkg, skip, R, words, vis=vis_struct)
                    assert want_skip.n_selected == int((sel & visible).sum()) < want_plain.n_selected == int(sel.sum())
                    for how in ("host", "device"):
                        _assert_same(_raw(pkg, U, hb, plain, words, how), want_plain, f"visibility {mask_name} {what} {how}")
                        _assert_same(_raw(pkg, U, hb, skip, words, how), want_skip, f"skip hidden {mask_name} {what} {how}")
            # the true alpha is binned: the histogram of the whole cloud is the uploaded alphas', though a third is resident as +0
            alpha_only = MC.request(pkg, 0, (MC.HISTS_A[0],))
            assert np.array_equal(U.measure(alpha_only).hist[0], MC.histogram(s.alpha, *MC.HISTS_A[0][1:]))
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA) and U.get_visibility()[1] == hidden_count
            # a mask alone (no volume), then nothing in force: SKIP_HIDDEN hides nothing
            U.set_visibility(mask=hide)
            skip = MC.request(pkg, 7, MC.HISTS_A, skip_hidden=True)
            vm, keep2 = E.visibility_struct((), hide)
            _assert_same(U.measure(skip), _eval(pkg, skip, R, vis=vm), "a mask alone in force")
            U.set_visibility()
            _assert_same(U.measure(skip), _eval(pkg, MC.request(pkg, 7, MC.HISTS_A), R), "the visibility cleared")
    finally:
        hb.free()


# ---- 3. the gizmo: transform the selection about its centroid, measure again ----------------------------------------------------------
@pytest.mark.gpu
def test_transform_about_the_centroid(pkg):
    E = pkg.engine
    c = MC.case(pkg, "n257_nosh")
    sel, words = c.masks(pkg)["random"]
    req = MC.request(pkg, 7, MC.HISTS_A)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        first = U.measure(req, sel)
        pivot = first.centroid()
        assert np.isfinite(pivot).all()
        moved = U.transform(E.xform(axis_angle=((0.0, 0.0, 1.0), 30.0), scale=1.25, pivot=tuple(pivot)), sel)
        assert moved == int(sel.sum())
        R = U.read()
        assert not np.array_equal(R.P.view(np.uint32), c.splats.P.view(np.uint32))
        second = U.measure(req, sel)
        _assert_same(second, _eval(pkg, req, R, sel), "after a transform about the centroid")
        assert not MC.same_result(first, second)
        # a turn and a uniform scale about the centroid leave the centroid where it was, to the rounding of the float32 positions
        # (half an ulp of 2048 per coordinate and splat: 1.2e-4, and as much again for the pivot rounded to float32)
        assert np.allclose(second.centroid(), pivot, rtol=0, atol=5e-4)


# ---- 4. nothing is invalidated ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_measure_between_frames_changes_nothing(pkg):
    s = pkg.scenes.make_scene(16385, seed=41, sh=True, log_scale_range=(-4.0, -2.5))      # (around the origin: the frames show it)
    cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
    req = MC.request(pkg, 7, MC.HISTS_C)
    sel = np.random.default_rng(6).random(s.n) < 0.5

    def run(measure):
        with pkg.Engine(0) as U:
            U.upload(s)
            first = U.render(cam).copy()
            assert first.any(), "an empty frame: the case tests nothing"
            st, pol, planes = U.stats(), U.policy_state(), M._planes(U)
            if measure:
                _assert_same(U.measure(req, sel), _eval(pkg, req, s, sel), "between two frames")
                assert U.stats() == st, "a measure changed gsr_stats"
                assert U.policy_state() == pol, "a measure changed the policy state"
                M._assert_same_planes(M._planes(U), planes, "a measure between frames")
            second = U.render(cam).copy()
            return first, second, {k: v for k, v in U.stats().items() if isinstance(v, int)}, U.policy_state()

    base, got = run(False), run(True)
    assert np.array_equal(base[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(base[1].view(np.uint32), got[1].view(np.uint32))
    assert base[2] == got[2] and base[3] == got[3]
    assert got[2]["sorts_skipped"] >= 1, "the second frame did not reuse the cached depth order: the case tests nothing"


# ---- 5. refusals, with nothing launched or written ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    import test_measure as T
    E, L = pkg.engine, pkg.load_library()
    c = pkg.scenes.make_scene(257, seed=42, sh=True, log_scale_range=(-4.0, -2.5))        # (around the origin: the frames show it)
    words = (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20                                                 # (a multiple of any granularity the allocator may round to)
        room = hb.upload(np.full(size // 4, FILL, np.uint32))
        host_mask = np.full(words + 2, FILL, np.uint32)
        res = E.gsr_measure_result()
        res.n_selected = -9
        hist = np.full(1200, 9, np.uint32)
        ok = MC.request(pkg, 7, MC.HISTS_A)

        def call(eng, req=ok, mask=room, device=1, out=res, h=hist.ctypes.data):
            return L.gsr_measure(eng.h, C.c_void_p(mask) if mask is not None else None, device, C.byref(req) if req is not None else None,
                                 C.byref(out) if out is not None else None, h)

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()                    # before any upload
            assert call(U, mask=None, device=0) == GSR_E_INVALID
            U.upload(c)
            cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
            frame = U.render(cam).copy()
            U.render(cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            cases = {"NULL request": lambda: call(U, req=None), "NULL result": lambda: call(U, out=None),
                     "no hist_out": lambda: call(U, h=None), "hist_out without a histogram": lambda: call(U, req=MC.request(pkg, 7)),
                     "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, device=1),
                     "misaligned mask": lambda: call(U, mask=room + 2),
                     "mask past its allocation": lambda: call(U, mask=room + size - (words * 4 - 4))}
            for label, r in T._bad_requests(pkg):
                for device in (1, 0):
                    cases[f"{label}, {'device' if device else 'host'} mask"] = (lambda r=r, device=device:
                                                                                 call(U, req=r, mask=room if device else host_mask.ctypes.data, device=device))
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_measure" in L.gsr_last_error(), label
                assert U.get_measure() == {"measures": 0, "measured_last": 0, "ms": [0.0] * 4}, label      # nothing was launched
                if n_case % 8 == 0:
                    assert np.array_equal(U.render(cam), frame), label
            M._assert_same_planes(M._planes(U), planes, "refusals")
            assert U.stats()["sorts_skipped"] > skipped, "the cached order did not survive the refusals"
            assert res.n_selected == -9 and (hist == 9).all() and (host_mask == FILL).all()
            assert (hb.download(room, (size // 4,), np.uint32) == FILL).all(), "a refused measure wrote to device memory"
            assert L.gsr_get_measure(U.h, None, None, None) == 0       # every pointer may be NULL
            # an upload in progress
            assert L.gsr_upload_begin(U.h, c.n, 1, None) == 0
            assert call(U) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_upload_abort(U.h) == 0
    finally:
        hb.free()


# ---- 6. the empty cloud ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_cloud(pkg):
    import test_measure as T
    c = MC.case(pkg, "n63_nosh")
    req = MC.request(pkg, 7, MC.HISTS_A)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        assert U.remove(np.ones(c.n, bool)) == 0
        T._assert_empty(U.measure(req), sum(b + 3 for _, _, _, b, _ in MC.HISTS_A))
        T._assert_empty(U.measure(MC.request(pkg, 0)), 0)
        assert U.get_measure()["measures"] == 0


# ---- 7. several ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_measure(pkg):
    E = pkg.engine
    c = MC.case(pkg, "n16385_nosh")
    req = MC.request(pkg, 7, MC.HISTS_A)
    sel, words = c.masks(pkg)["random"]
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        single = [U.measure(req, sel), U.measure(req)]
    _assert_same(single[0], _eval(pkg, req, c.splats, words), "the single context")
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(c.splats)
        _assert_same(Mu.measure(req, sel), single[0], "MultiEngine.measure, a mask")
        _assert_same(Mu.measure(req), single[1], "MultiEngine.measure, no mask")
        assert [Mu.stats(r)["n_splats"] for r in range(2)] == [c.n, c.n]
