"""Attribute updates on the GPU (gsr_update): resident splats edited in place.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of cloud A, then update(s) --
and a fresh context F that was uploaded the edited arrays with the same options: the resident planes (gsr_debug_read_resident) are the
same bytes, and so is every later frame, whatever the frame's regime.

The cloud: 357 splats = five full clusters of 64 and one of 37 (the partial last cluster); frames of 96 x 64 pixels on the parity
tests' orbit."""
import ctypes as C

import numpy as np
import pytest

from helpers import HipBuffers

N = 357
W, H = 96, 64
GSR_E_INVALID = -1
PLANES = ("geoA", "geoB", "col", "colrow", "clusA", "clusB")
ATTRS = ("Cd", "alpha", "scale", "orient", "shx", "shy", "shz")
SH3 = ("shx", "shy", "shz")
SUBSETS = {
    "alpha": ("alpha",), "Cd": ("Cd",), "SH": SH3, "Cd+SH": ("Cd",) + SH3, "scale": ("scale",), "orient": ("orient",),
    "scale+orient": ("scale", "orient"), "all": ATTRS,
}
RANGES = ((0, N), (0, 1), (N - 1, 1), (171, 1), (50, 150))      # whole cloud; first, last, a middle splat; [50, 200) across clusters


def _cloud(pkg, seed, sh=True):
    """(splats large enough to overlap on a 96 x 64 frame: the frames below have depth complexity)"""
    return pkg.scenes.make_scene(N, seed=seed, sh=sh, log_scale_range=(-3.5, -2.0))


def _copy(pkg, s):
    g = lambda a: None if a is None else a.copy()
    return pkg.scenes.Splats(s.P.copy(), g(s.Cd), g(s.alpha), g(s.scale), g(s.orient), g(s.shx), g(s.shy), g(s.shz))


def _rows(src, names, first, n):
    return {k: np.ascontiguousarray(getattr(src, k)[first:first + n]) for k in names}


def _edit(pkg, eng, s, src, names, first, n):
    """update the engine's splats [first, first + n) with src's rows of `names`; returns the edited cloud (s is not changed)"""
    rows = _rows(src, names, first, n)
    if eng is not None:
        assert eng.update_attrs(first, **rows) == n
    out = _copy(pkg, s)
    for k, v in rows.items():
        getattr(out, k)[first:first + n] = v
    return out


def _planes(eng, sh=True):
    return {name: eng.debug_resident(k) for k, name in enumerate(PLANES) if sh or name != "colrow"}


def _live(planes):
    """the planes with `col` cut to its live region: slots < n of each chunk (the chunks are capacity-strided as stored, and a
    context that held a larger cloud before keeps the larger capacity)"""
    n, chunks = planes["geoA"].size // 16, 6 if "colrow" in planes else 1
    out = dict(planes)
    out["col"] = np.ascontiguousarray(planes["col"].reshape(chunks, -1, 16)[:, :n])
    return out


def _assert_same_planes(got, want, label):
    assert got.keys() == want.keys()
    got, want = _live(got), _live(want)
    for name in want:
        assert got[name].size == want[name].size and want[name].size > 0, (label, name, got[name].size, want[name].size)
        if not np.array_equal(got[name], want[name]):
            at = int(np.argmax(got[name] != want[name]))
            raise AssertionError(f"{label}: plane {name} differs in {int((got[name] != want[name]).sum())} bytes, first at byte {at} "
                                 f"(16-byte word {at // 16})")


def _fresh_planes(pkg, s, order=1, sh=True):
    with pkg.Engine(0) as F:
        F.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        F.upload(s)
        return _planes(F, sh)


def _cams(pkg, frames):
    return [pkg.camera.make_camera(W, H, sh_order=3, frame=f) for f in frames]


@pytest.fixture(scope="module")
def clouds(pkg):
    """A (what is uploaded), B and C (where the new values come from; their positions are never used)"""
    return _cloud(pkg, 11), _cloud(pkg, 12), _cloud(pkg, 13)


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_resident_bits(pkg, clouds, subset, order):
    A, B, _ = clouds
    E = pkg.engine
    names = SUBSETS[subset]
    for first, n in RANGES:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = _planes(U)
            edited = _edit(pkg, U, A, B, names, first, n)
            got = _planes(U)
            assert U.stats()["uploads"] == 1                        # an update is not an upload
        want = _fresh_planes(pkg, edited, order)
        _assert_same_planes(got, want, f"{subset} [{first}, {first + n}) order {order}")
        assert any(not np.array_equal(before[k], got[k]) for k in got), "the update changed nothing: the case tests nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("subset", ("alpha", "Cd", "scale+orient"))
def test_resident_bits_without_sh(pkg, subset, order):
    A, B = _cloud(pkg, 11, sh=False), _cloud(pkg, 12, sh=False)
    E = pkg.engine
    for first, n in RANGES:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            with pytest.raises(E.GsrError):
                U.debug_resident(E.RESIDENT_COLROW)                 # no colour rows without SH
            edited = _edit(pkg, U, A, B, SUBSETS[subset], first, n)
            got = _planes(U, sh=False)
        _assert_same_planes(got, _fresh_planes(pkg, edited, order, sh=False), f"no SH, {subset} [{first}, {first + n}) order {order}")


# ---- 2. cluster bounds both ways ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cluster_bounds_grow_shrink_and_flag(pkg, clouds):
    A = clouds[0]
    E = pkg.engine
    i = 171
    f16 = pkg.scenes.f16bits
    big = _copy(pkg, A)
    big.scale[i] = f16(A.scale[i].view(np.float16).astype(np.float32) * 64.0)
    inf = _copy(pkg, A)
    inf.scale[i, 1] = 0x7c00                                        # +inf
    with pkg.Engine(0) as U:
        U.upload(A)
        slot = int(np.where(U.debug_storage_order(N) == i)[0][0])
        cl = slot // 64
        base = _planes(U)
        wA = lambda p: p["clusA"].view(np.float32).reshape(-1, 4)[:, 3]
        wB = lambda p: p["clusB"].view(np.float32).reshape(-1, 4)[:, 3]
        assert wA(base).size == 6 and wB(base)[cl] == 0.0
        for label, cloud in (("grown", big), ("shrunk back", A), ("inf", inf), ("restored", A)):
            U.update_attrs(i, scale=cloud.scale[i:i + 1])
            got = _planes(U)
            _assert_same_planes(got, _fresh_planes(pkg, cloud), label)
            if label == "grown":
                assert wA(got)[cl] > 8.0 * wA(base)[cl]             # a stale-small bound would drop visible splats
            if label == "inf":
                assert wB(got)[cl] == 1.0 and wB(got).sum() == 1.0  # the "never cull" flag appears ...
            if label in ("shrunk back", "restored"):
                _assert_same_planes(got, base, label + " vs the first upload")    # ... and a stale-large bound or flag goes


# ---- 3. frames ---------------------------------------------------------------------------------------------------------------
def _nearest_third_alpha(A, cam):
    d = np.linalg.norm(A.P.astype(np.float64) - np.asarray(cam.cam_pos, np.float64), axis=1)
    al = A.alpha.copy()
    al[np.argsort(d, kind="stable")[:N // 3]] = 0.0
    return al


def _fresh_frames(pkg, s, cams, opts=()):
    with pkg.Engine(0) as F:
        for k, v in opts:
            F.set_option(k, v)
        F.upload(s)
        return [F.render(c).copy() for c in cams]


def _plain_opts(E):
    return ((E.OPT_OCCLUSION_CULL, 0), (E.OPT_LAZY_COLOUR, 0), (E.OPT_SORT_CACHE, 0))


def _check_frames(pkg, got, edited, unedited, cams, label):
    E = pkg.engine
    want = _fresh_frames(pkg, edited, cams)
    plain = _fresh_frames(pkg, edited, cams, _plain_opts(E))
    stale = _fresh_frames(pkg, unedited, cams, _plain_opts(E))
    for k in range(len(cams)):
        assert np.array_equal(want[k], plain[k]), f"{label}: the fresh contexts disagree on frame {k}"
        assert not np.array_equal(want[k], stale[k]), f"{label}: the edit does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{label}: frame {k} after the update differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
def test_frames_after_updates_default_options(pkg, clouds):
    """(a) opacity 0 on the nearest third, (b) new Cd under a static camera, (c) scale x 4 on a tenth -- one after the other on one
    context with the default options (culling, lazy colour and the sort cache as they default)"""
    A, B, _ = clouds
    cams = _cams(pkg, range(8))
    f16 = pkg.scenes.f16bits
    with pkg.Engine(0) as U:
        U.upload(A)
        for c in cams[:3]:
            U.render(c)
        # (a)
        s1 = _copy(pkg, A)
        s1.alpha[:] = _nearest_third_alpha(A, cams[3])
        U.update_attrs(0, alpha=s1.alpha)
        _check_frames(pkg, [U.render(c).copy() for c in cams[3:5]], s1, A, cams[3:5], "(a) alpha")
        # (b): the camera stands still before and after, so the frame before the update left a cached depth order
        U.render(cams[4])
        skipped = U.stats()["sorts_skipped"]
        s2 = _edit(pkg, U, s1, B, ("Cd",), 0, N)
        _check_frames(pkg, [U.render(cams[4]).copy() for _ in range(2)], s2, s1, [cams[4], cams[4]], "(b) Cd, static camera")
        print("sorts skipped before the Cd update:", skipped, "after its two frames:", U.stats()["sorts_skipped"])
        # (c)
        s3 = _copy(pkg, s2)
        s3.scale[100:136] = f16(s2.scale[100:136].view(np.float16).astype(np.float32) * 4.0)
        U.update_attrs(100, scale=s3.scale[100:136])
        _check_frames(pkg, [U.render(c).copy() for c in cams[5:7]], s3, s2, cams[5:7], "(c) scale x 4")
        _assert_same_planes(_planes(U), _fresh_planes(pkg, s3), "after (a), (b), (c)")


@pytest.mark.gpu
def test_frames_after_update_two_frames_in_flight_device_target(pkg, clouds):
    """(a) with GSR_OPT_FRAMES_IN_FLIGHT = 2 and a device target: the update is issued while the frames before it are still queued"""
    A = clouds[0]
    E = pkg.engine
    cams = _cams(pkg, range(5))
    s1 = _copy(pkg, A)
    s1.alpha[:] = _nearest_third_alpha(A, cams[3])
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
            U.upload(A)
            outs = [hb.alloc(W * H * 16) for _ in cams]
            for c, o in zip(cams[:3], outs[:3]):
                U.render_to_device(c, o)
            U.update_attrs(0, alpha=s1.alpha)                       # (no synchronisation by the caller)
            for c, o in zip(cams[3:], outs[3:]):
                U.render_to_device(c, o)
            U.synchronize()
            got = [hb.download(o, (H, W, 4)) for o in outs]
        before = _fresh_frames(pkg, A, cams[:3])
        for k in range(3):
            assert np.array_equal(got[k], before[k]), f"frame {k}, queued before the update, was disturbed by it"
        _check_frames(pkg, got[3:], s1, A, cams[3:], "(a) alpha, two frames in flight")
    finally:
        hb.free()


@pytest.mark.gpu
def test_frames_after_update_occlusion_cull_always(pkg, clouds):
    """(a) with GSR_OPT_OCCLUSION_CULL = 2: horizons left by the unedited cloud must not cull what the edit uncovers"""
    A = clouds[0]
    E = pkg.engine
    cams = _cams(pkg, range(5))
    s1 = _copy(pkg, A)
    s1.alpha[:] = _nearest_third_alpha(A, cams[3])
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_OCCLUSION_CULL, 2)
        U.upload(A)
        for c in cams[:3]:
            U.render(c)
        U.update_attrs(0, alpha=s1.alpha)
        got = [U.render(c).copy() for c in cams[3:]]
        st = U.stats()
        print("frames_culled with GSR_OPT_OCCLUSION_CULL = 2:", st["frames_culled"], "repaired:", st["frames_repaired"])
    _check_frames(pkg, got, s1, A, cams[3:], "(a) alpha, cull 2")


# ---- 4. updates compose ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_two_partial_updates_equal_one_upload(pkg, clouds, order):
    A, B, Cc = clouds
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        U.upload(A)
        s = _edit(pkg, U, A, B, ("Cd", "alpha", "orient"), 0, 200)
        s = _edit(pkg, U, s, Cc, ("scale", "Cd") + SH3, 150, N - 150)
        got = _planes(U)
    _assert_same_planes(got, _fresh_planes(pkg, s, order), f"two overlapping updates, order {order}")


# ---- 5. errors leave the context alone ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_the_context_alone(pkg, clouds):
    A, B, _ = clouds
    E = pkg.engine
    L = pkg.load_library()
    cam = _cams(pkg, [2])[0]
    cd, sh = np.ascontiguousarray(B.Cd), np.ascontiguousarray(B.shx)

    def call(eng, first, n, **ptrs):
        u = E.gsr_attr_update()
        for k, a in ptrs.items():
            setattr(u, k, a.ctypes.data)
        return L.gsr_update(eng.h, first, n, C.byref(u))

    with pkg.Engine(0) as U:
        assert call(U, 0, 1, Cd=cd) == GSR_E_INVALID                # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes, frame = _planes(U), U.render(cam).copy()
        cases = {
            "NULL u": lambda: L.gsr_update(U.h, 0, 1, None),
            "first < 0": lambda: call(U, -1, 2, Cd=cd),
            "n < 0": lambda: call(U, 0, -1, Cd=cd),
            "beyond the cloud": lambda: call(U, N - 1, 2, Cd=cd),
            "first beyond the cloud": lambda: call(U, N + 1, 0, Cd=cd),
            "one SH array": lambda: call(U, 0, N, shy=sh),
            "two SH arrays": lambda: call(U, 0, N, shx=sh, shz=sh),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            _assert_same_planes(_planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        # nothing to do is not an error, and does nothing
        assert call(U, 0, 0, Cd=cd) == 0 and call(U, 5, 10) == 0
        _assert_same_planes(_planes(U), planes, "empty updates")
        assert np.array_equal(U.render(cam), frame)
        # an upload in progress.  (Nothing is comparable here: gsr_upload_begin itself gave the resident cloud up, no frame can be
        # rendered and no plane read while the upload is open; the refusal and its text are what can be held.)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert call(U, 0, 1, Cd=cd) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
    with pkg.Engine(0) as V:                                        # SH arrays for a cloud uploaded without SH
        V.upload(_cloud(pkg, 11, sh=False))
        planes, frame = _planes(V, sh=False), V.render(cam).copy()
        assert call(V, 0, N, shx=sh, shy=sh, shz=sh) == GSR_E_INVALID
        assert call(V, 0, N, Cd=cd, shx=sh, shy=sh, shz=sh) == GSR_E_INVALID      # ... also beside an attribute it could have taken
        _assert_same_planes(_planes(V, sh=False), planes, "SH arrays without SH")
        assert np.array_equal(V.render(cam), frame), "SH arrays without SH"
    with pytest.raises(E.GsrError):
        E.attr_update_struct(Cd=cd, alpha=B.alpha[:5])               # mismatched lengths never reach the library


# ---- 6. several ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_update_matches_single_context(pkg, clouds):
    A = clouds[0]
    E = pkg.engine
    cams = _cams(pkg, range(4))
    s1 = _copy(pkg, A)
    s1.alpha[:] = _nearest_third_alpha(A, cams[2])
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as M:
        M.upload(A)
        for c in cams[:2]:
            M.render(c)
        assert M.update_attrs(0, alpha=s1.alpha) == N
        got = [M.render(c).copy() for c in cams[2:]]
        assert [M.stats(r)["uploads"] for r in range(2)] == [1, 1]
    _check_frames(pkg, got, s1, A, cams[2:], "two ranks, (a) alpha")


# ---- 7. the wire overlay shares the inverse permutation ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wire_first", (True, False))
def test_wire_overlay_after_a_colour_update(pkg, clouds, wire_first):
    A, B, _ = clouds
    cam = _cams(pkg, [1])[0]
    with pkg.Engine(0) as U:
        U.upload(A)
        old = U.render_wire(cam).copy() if wire_first else None     # (builds the inverse the update then uses -- or the update builds it)
        edited = _edit(pkg, U, A, B, ("Cd",), 0, N)
        got = U.render_wire(cam).copy()
    with pkg.Engine(0) as F:
        F.upload(edited)
        want = F.render_wire(cam).copy()
    assert (want[..., 3] > 0).sum() > 100
    assert np.array_equal(got, want)
    assert old is None or not np.array_equal(old, got)


# ---- 8. through the renderer verbs (GSplatRenderer::updateAttributes on a GPU instance) --------------------------------------
def _shim_planes(pkg, R, sh=True):
    """the resident planes of the context behind a GSplatRenderer"""
    import types
    L = pkg.load_library()
    L.gsplat_renderer_engine.restype = C.c_void_p
    ctx = types.SimpleNamespace(L=L, h=C.c_void_p(L.gsplat_renderer_engine(R.h)))
    return {name: pkg.engine.Engine.debug_resident(ctx, k) for k, name in enumerate(PLANES) if sh or name != "colrow"}


def _shim_with(pkg, parts):
    """a GPU renderer with one registered row per part (details 0x100, 0x101, ...: the plan packs them in that order)"""
    R = pkg.GSplatRenderer(0)
    return R, [R.registerUpdate(0x100 + k, (1, 0, 0, 0), 0, p) for k, p in enumerate(parts)]


@pytest.mark.gpu
def test_shim_update_in_place_then_restage(pkg, clouds):
    """two rows resident; the second is edited in place (no staging), which equals a fresh renderer holding the edited arrays, planes
    and frame; a forced re-stage then uploads the arrays the row holds NOW; and after the engine refuses an update the next redraw
    stages again"""
    A, B, _ = clouds
    cam = _cams(pkg, [2])[0]
    a, b = A.subset(slice(0, 200)), A.subset(slice(200, N))
    eb = _copy(pkg, b)
    eb.Cd[:], eb.alpha[:], eb.scale[:] = B.Cd[200:], B.alpha[200:], B.scale[200:]
    R, (ia, ib) = _shim_with(pkg, (a, b))
    F, fids = _shim_with(pkg, (a, eb))
    G, gids = _shim_with(pkg, (eb,))
    try:
        before = R.frame(cam, [ia, ib]).copy()
        assert R.updateAttributes(ib, Cd=eb.Cd, alpha=eb.alpha, scale=eb.scale) == (1, 200, N - 200)
        assert R.query(R.Q_STAGING_COUNT) == 1 and R.query(R.Q_LAST_STATUS) == 0
        got = R.frame(cam, [ia, ib]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 1                       # in place: the redraw staged nothing
        want = F.frame(cam, fids).copy()
        assert np.array_equal(got, want) and not np.array_equal(got, before)
        _assert_same_planes(_shim_planes(pkg, R), _shim_planes(pkg, F), "shim, updated in place")
        # a re-stage (only the second row is shown now) uploads what the row holds: the edited arrays
        got = R.frame(cam, [ib]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 2
        assert np.array_equal(got, G.frame(cam, gids))
        _assert_same_planes(_shim_planes(pkg, R), _shim_planes(pkg, G), "shim, re-staged after the update")
        # the engine refuses (an upload was opened behind the shim's back): the error comes back, and the next redraw stages again
        L = pkg.load_library()
        eng = C.c_void_p(L.gsplat_renderer_engine(R.h))
        assert L.gsr_upload_begin(eng, 1, 1, None) == 0
        rc, first, n = R.updateAttributes(ib, alpha=b.alpha)
        assert rc == GSR_E_INVALID and R.query(R.Q_LAST_STATUS) == GSR_E_INVALID
        assert L.gsr_upload_abort(eng) == 0
        got = R.frame(cam, [ib]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 3
        back = _copy(pkg, eb)
        back.alpha[:] = b.alpha
        H_, hids = _shim_with(pkg, (back,))
        try:
            assert np.array_equal(got, H_.frame(cam, hids))
        finally:
            H_.close()
    finally:
        R.close(); F.close(); G.close()


@pytest.mark.gpu
def test_shim_sh_arrays_stay_home_while_the_pass_carries_no_sh(pkg, clouds):
    """the row joined last decides whether a pass carries SH: here it does not, so an update's SH arrays go into the row (for the next
    re-stage) but not to the GPU, while its Cd does"""
    A, B, _ = clouds
    cam = _cams(pkg, [2])[0]
    x = A.subset(slice(0, 200))
    y = _cloud(pkg, 11, sh=False).subset(slice(200, N))
    ex = _copy(pkg, x)
    ex.Cd[:], ex.shx[:], ex.shy[:], ex.shz[:] = B.Cd[:200], B.shx[:200], B.shy[:200], B.shz[:200]
    R, (ix, iy) = _shim_with(pkg, (x, y))
    F, fids = _shim_with(pkg, (ex, y))
    try:
        before = R.frame(cam, [ix, iy]).copy()
        assert R.query(R.Q_SH_PRESENT) == 0
        assert R.updateAttributes(ix, Cd=ex.Cd, shx=ex.shx, shy=ex.shy, shz=ex.shz) == (1, 0, 200)
        assert R.query(R.Q_LAST_STATUS) == 0 and R.query(R.Q_STAGING_COUNT) == 1
        got = R.frame(cam, [ix, iy]).copy()
        assert np.array_equal(got, F.frame(cam, fids)) and not np.array_equal(got, before)
        _assert_same_planes(_shim_planes(pkg, R, sh=False), _shim_planes(pkg, F, sh=False), "shim, no SH in the pass")
        assert R.rowArray(ix, 5) == R._updates[ix]["shx"].ctypes.data
    finally:
        R.close(); F.close()

