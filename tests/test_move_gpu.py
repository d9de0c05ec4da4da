"""Position updates on the GPU (gsr_move): resident splats moved, re-ordered on the device, no re-upload.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of cloud A, then move(s) --
and a fresh context F that was uploaded the edited arrays with the same options and the origin in force: the resident planes
(gsr_debug_read_resident) and the storage order (gsr_debug_read_storage_order) are the same, and so is every later frame, whatever
the frame's regime.

The cloud: 357 splats = five full clusters of 64 and one of 37 (the partial last cluster); frames of 96 x 64 pixels on the parity
tests' orbit.  New positions come from a second cloud with another seed, so a whole-cloud move really changes the order."""
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
SUBSETS = {"P": (), "P+scale+orient": ("scale", "orient"), "P+all": ATTRS}
RANGES = ((0, N), (0, 1), (N - 1, 1), (171, 1), (50, 150))      # whole cloud; first, last, a middle splat; [50, 200) across clusters


def _cloud(pkg, seed, sh=True, n=N):
    """(splats large enough to overlap on a 96 x 64 frame: the frames below have depth complexity)"""
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-3.5, -2.0))


def _copy(pkg, s):
    g = lambda a: None if a is None else a.copy()
    return pkg.scenes.Splats(s.P.copy(), g(s.Cd), g(s.alpha), g(s.scale), g(s.orient), g(s.shx), g(s.shy), g(s.shz))


def _move(pkg, eng, s, P, first, src=None, names=(), origin=None):
    """move the engine's splats [first, first + n) to the rows of P (n = len(P)), with src's rows of `names` as new attributes;
    returns the edited cloud (s is not changed)"""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = len(P)
    rows = {k: np.ascontiguousarray(getattr(src, k)[first:first + n]) for k in names}
    if eng is not None:
        assert eng.move(first, P, origin=origin, **rows) == n
    out = _copy(pkg, s)
    out.P[first:first + n] = P
    for k, v in rows.items():
        getattr(out, k)[first:first + n] = v
    return out


def _planes(eng, sh=True):
    out = {name: eng.debug_resident(k) for k, name in enumerate(PLANES) if sh or name != "colrow"}
    out["order"] = eng.debug_storage_order(out["geoA"].size // 16).view(np.uint8)
    return out


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


def _fresh_planes(pkg, s, order=1, sh=True, origin=(0.0, 0.0, 0.0)):
    with pkg.Engine(0) as F:
        F.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        F.upload(s, origin)
        return _planes(F, sh)


def _cams(pkg, frames, pivot=(0.0, 0.0, 0.0)):
    return [pkg.camera.make_camera(W, H, sh_order=3, frame=f, pivot=pivot) for f in frames]


def _fresh_frames(pkg, s, cams, opts=(), origin=(0.0, 0.0, 0.0), render=None, prepare=None):
    with pkg.Engine(0) as F:
        for k, v in opts:
            F.set_option(k, v)
        if prepare:
            prepare(F)
        F.upload(s, origin)
        return [(render(F, c) if render else F.render(c)).copy() for c in cams]


def _mirror(P):
    """every position through the centre of the box: what was near is far"""
    P = P.astype(np.float32)
    return (P.min(axis=0) + P.max(axis=0) - P).astype(np.float32)


@pytest.fixture(scope="module")
def clouds(pkg):
    """A (what is uploaded), B and C (where the new positions and values come from)"""
    return _cloud(pkg, 11), _cloud(pkg, 12), _cloud(pkg, 13)


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_resident_bits(pkg, subset, sh, order):
    A, B = _cloud(pkg, 11, sh=sh), _cloud(pkg, 12, sh=sh)
    E = pkg.engine
    names = tuple(k for k in SUBSETS[subset] if sh or k not in SH3)
    for first, n in RANGES:
        label = f"{subset} [{first}, {first + n}) order {order} sh {sh}"
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = _planes(U, sh)
            edited = _move(pkg, U, A, B.P[first:first + n], first, B, names)
            got = _planes(U, sh)
            st = U.stats()
            assert st["uploads"] == 1 and st["moves"] == 1, label     # a move is not an upload
        _assert_same_planes(got, _fresh_planes(pkg, edited, order, sh), label)
        assert not np.array_equal(before["geoA"], got["geoA"]), "the move changed nothing: the case tests nothing"
        if order == 1 and n == N:
            assert not np.array_equal(before["order"], got["order"]), "the storage order did not change: the case tests nothing"
        if order == 0:
            assert np.array_equal(got["order"].view(np.int32), np.arange(N, dtype=np.int32))


# ---- 2. small motion, then the box itself changes ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_small_motion_then_a_corner_moves(pkg, clouds):
    A = _copy(pkg, clouds[0])
    lo, hi = A.P.min(axis=0), A.P.max(axis=0)
    A.P[0] = lo - 1.0                                               # splat 0 IS the box's low corner
    rng = np.random.default_rng(5)
    with pkg.Engine(0) as U:
        U.upload(A)
        before = _planes(U)
        jit = (A.P + rng.uniform(-1.0, 1.0, A.P.shape) * 1.0e-3 * (hi - lo)).astype(np.float32)
        jit[0] = A.P[0]                                             # (the box stays)
        s1 = _move(pkg, U, A, jit, 0)
        got = _planes(U)
        same = int((before["order"].view(np.int32) == got["order"].view(np.int32)).sum())
        print("slots that kept their splat through the jitter:", same, "of", N)
        assert same > N // 2                                        # most of the permutation survives
        _assert_same_planes(got, _fresh_planes(pkg, s1), "jitter")
        s2 = _move(pkg, U, s1, hi + 1.0, 0)                         # from one corner to the other: every Morton code changes
        got = _planes(U)
        _assert_same_planes(got, _fresh_planes(pkg, s2), "corner to corner")
        assert U.stats()["moves"] == 2 and U.stats()["uploads"] == 1


# ---- 3. a new origin -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("new_origin", (True, False))
def test_translation_with_and_without_a_new_origin(pkg, clouds, new_origin):
    A = clouds[0]
    t = np.asarray((10.0, -3.0, 7.0), np.float32)
    old = (0.25, 0.5, -0.125)
    cam = _cams(pkg, [2], pivot=tuple(float(x) for x in t))[0]
    with pkg.Engine(0) as U:
        U.upload(A, old)
        U.render(_cams(pkg, [1])[0])
        edited = _move(pkg, U, A, A.P + t, 0, origin=tuple(t) if new_origin else None)
        got_planes, got = _planes(U), U.render(cam).copy()
    origin = tuple(float(x) for x in t) if new_origin else old
    _assert_same_planes(got_planes, _fresh_planes(pkg, edited, origin=origin), f"translated, new origin {new_origin}")
    want = _fresh_frames(pkg, edited, [cam], origin=origin)[0]
    assert (want[..., 3] > 0).sum() > 100                           # the translated cloud is in view
    assert np.array_equal(got, want)


# ---- 4. repeated moves under a capacity larger than the cloud --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_repeated_moves_with_spare_capacity_then_an_update(pkg, clouds, order):
    A, B, Cc = clouds
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        U.upload(_cloud(pkg, 21, n=500))                            # capacity 500: the colour chunks of the 357 are strided by it
        U.upload(A)
        assert U.debug_resident(pkg.engine.RESIDENT_COL).size == 6 * 500 * 16
        s = _move(pkg, U, A, B.P, 0)
        s = _move(pkg, U, s, Cc.P[50:200], 50, Cc, ("Cd", "alpha"))
        s = _move(pkg, U, s, _mirror(s.P), 0, B, ("scale",) + SH3)  # three moves: the spare and the live planes swap and swap back
        assert U.stats()["moves"] == 3
        _assert_same_planes(_planes(U), _fresh_planes(pkg, s, order), f"three moves, order {order}")
        rows = {k: np.ascontiguousarray(getattr(Cc, k)[100:300]) for k in ("orient", "Cd")}
        assert U.update_attrs(100, **rows) == 200                   # through the inverse permutation rebuilt after the last move
        for k, v in rows.items():
            getattr(s, k)[100:300] = v
        got = _planes(U)
    _assert_same_planes(got, _fresh_planes(pkg, s, order), f"three moves and an update, order {order}")


# ---- 5. an unordered store comes and goes --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_non_finite_position_moves_in_and_out(pkg, clouds):
    """A fresh upload of a cloud with a non-finite position is accepted and stored in UPLOAD order (its box is not finite, so there
    are no Morton codes), its cluster flagged "never cull": a move that brings such a position in must end there, and the move that
    takes it out again must be back in Morton order"""
    A = clouds[0]
    with pkg.Engine(0) as U:
        U.upload(A)
        base = _planes(U)
        bad = np.asarray((np.inf, 0.0, 0.0), np.float32)
        s1 = _move(pkg, U, A, bad, 171)
        got = _planes(U)
        want = _fresh_planes(pkg, s1)
        assert np.array_equal(want["order"].view(np.int32), np.arange(N, dtype=np.int32))      # what F does: upload order
        assert want["clusB"].view(np.float32).reshape(-1, 4)[171 // 64, 3] == 1.0
        _assert_same_planes(got, want, "inf moved in")
        s2 = _move(pkg, U, s1, A.P[171], 171)
        got = _planes(U)
        assert not np.array_equal(got["order"].view(np.int32), np.arange(N, dtype=np.int32))
        _assert_same_planes(got, _fresh_planes(pkg, s2), "inf moved out")
        _assert_same_planes(got, base, "inf moved out vs the first upload")


# ---- 6. frames -----------------------------------------------------------------------------------------------------------------
def _frame_modes(pkg):
    E = pkg.engine
    # the left half of the frame covered at the window depth of the orbit's pivot, the centre of the cloud: fragments on either side
    cam = _cams(pkg, [0])[0]
    clip = cam.proj.reshape(4, 4).T.astype(np.float64) @ cam.view.reshape(4, 4).T.astype(np.float64) @ np.asarray((0.0, 0.0, 0.0, 1.0))
    depth = np.full((H, W), np.float32(0.5 * clip[2] / clip[3] + 0.5), np.float32)
    depth[:, W // 2:] = 1.0

    def twice(eng, c):
        eng.render(c)
        return eng.render(c)

    def shard(layout):
        def prepare(eng):
            eng.set_option(E.OPT_SHARD_LAYOUT, layout)
            eng.set_row_shard(1, 2)
        return prepare

    # label -> (options, render(eng, cam) or None, prepare(eng) or None)
    return {
        "cull 0": (((E.OPT_OCCLUSION_CULL, 0),), None, None),
        "cull 2": (((E.OPT_OCCLUSION_CULL, 2),), None, None),
        "cull 3": (((E.OPT_OCCLUSION_CULL, 3),), None, None),
        "lazy 0": (((E.OPT_LAZY_COLOUR, 0),), None, None),
        "lazy 2": (((E.OPT_LAZY_COLOUR, 2),), None, None),
        "sort cache 2": (((E.OPT_SORT_CACHE, 2),), twice, None),
        "depth-tested": ((), lambda eng, c: eng.render_depth(c, depth), None),
        "rgba16f": ((), None, lambda eng: eng.set_target_format(E.TARGET_RGBA16F)),
        "shard 1/2 interleaved": ((), None, shard(0)),
        "shard 1/2 bands": ((), None, shard(1)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cull 0", "cull 2", "cull 3", "lazy 0", "lazy 2", "sort cache 2", "depth-tested", "rgba16f",
                                  "shard 1/2 interleaved", "shard 1/2 bands"])
def test_frames_after_a_mirror_move(pkg, clouds, mode):
    """five frames leave horizons, hints, cached orders and policies behind; then the cloud goes to its mirror image through the box
    centre, and every later frame is a fresh upload's"""
    A = clouds[0]
    opts, render, prepare = _frame_modes(pkg)[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = _cams(pkg, range(13))
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:5]:
            draw(U, c)
        edited = _move(pkg, U, A, _mirror(A.P), 0)
        got = [draw(U, c).copy() for c in cams[5:]]
    want = _fresh_frames(pkg, edited, cams[5:], opts, render=render, prepare=prepare)
    stale = _fresh_frames(pkg, A, cams[5:], opts, render=render, prepare=prepare)
    if mode == "depth-tested":
        free = _fresh_frames(pkg, edited, cams[5:6])[0]
        assert not np.array_equal(want[0], free) and (want[0][..., 3] > 0).sum() > 100, "the depth buffer rejects nothing, or everything"
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the move does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode}: frame {k} after the move differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", (0, 1))
def test_frames_after_a_move_two_in_flight_device_target(pkg, clouds, deferred):
    """GSR_OPT_FRAMES_IN_FLIGHT = 2 (and GSR_OPT_DEFERRED_CHECK = 1) with a device target: the move is issued while the frames before
    it are still queued, with no synchronisation by the caller"""
    A = clouds[0]
    E = pkg.engine
    cams = _cams(pkg, range(13))
    opts = ((E.OPT_FRAMES_IN_FLIGHT, 2), (E.OPT_DEFERRED_CHECK, deferred))
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            for k, v in opts:
                U.set_option(k, v)
            U.upload(A)
            outs = [hb.alloc(W * H * 16) for _ in cams]
            for c, o in zip(cams[:5], outs[:5]):
                U.render_to_device(c, o)
            edited = _move(pkg, U, A, _mirror(A.P), 0)               # (no synchronisation by the caller)
            for c, o in zip(cams[5:], outs[5:]):
                U.render_to_device(c, o)
            U.synchronize()
            got = [hb.download(o, (H, W, 4)) for o in outs]
        before = _fresh_frames(pkg, A, cams[:5])
        for k in range(5):
            assert np.array_equal(got[k], before[k]), f"frame {k}, queued before the move, was disturbed by it"
        want = _fresh_frames(pkg, edited, cams[5:])
        for k in range(len(want)):
            assert np.array_equal(got[5 + k], want[k]), f"frame {k} after the move, deferred check {deferred}"
    finally:
        hb.free()


# ---- 7. the wire overlay after a move ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wire_first", (True, False))
def test_wire_overlay_after_a_move(pkg, clouds, wire_first):
    A, B, _ = clouds
    cam = _cams(pkg, [1])[0]
    with pkg.Engine(0) as U:
        U.upload(A)
        old = U.render_wire(cam).copy() if wire_first else None     # (builds the inverse the move then scatters through -- or the move does)
        edited = _move(pkg, U, A, B.P, 0)
        got = U.render_wire(cam).copy()                             # (through the inverse of the NEW order)
    with pkg.Engine(0) as F:
        F.upload(edited)
        want = F.render_wire(cam).copy()
    assert (want[..., 3] > 0).sum() > 100
    assert np.array_equal(got, want)
    assert old is None or not np.array_equal(old, got)


# ---- 8. errors leave the context alone -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_the_context_alone(pkg, clouds):
    A, B, _ = clouds
    E = pkg.engine
    L = pkg.load_library()
    cam = _cams(pkg, [2])[0]
    P, sh = np.ascontiguousarray(B.P), np.ascontiguousarray(B.shx)

    def call(eng, first, n, P=P, **ptrs):
        u = E.gsr_attr_update()
        for k, a in ptrs.items():
            setattr(u, k, a.ctypes.data)
        return L.gsr_move(eng.h, first, n, None if P is None else P.ctypes.data, None, C.byref(u))

    with pkg.Engine(0) as U:
        assert call(U, 0, 1) == GSR_E_INVALID                       # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes, frame = _planes(U), U.render(cam).copy()
        cases = {
            "NULL P": lambda: call(U, 0, 1, P=None),
            "first < 0": lambda: call(U, -1, 2),
            "n < 0": lambda: call(U, 0, -1),
            "beyond the cloud": lambda: call(U, N - 1, 2),
            "first beyond the cloud": lambda: call(U, N + 1, 0),
            "one SH array": lambda: call(U, 0, N, shy=sh),
            "two SH arrays": lambda: call(U, 0, N, shx=sh, shz=sh),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            _assert_same_planes(_planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        assert call(U, 5, 0) == 0 and L.gsr_move(U.h, 5, 0, P.ctypes.data, None, None) == 0      # nothing to do is not an error
        _assert_same_planes(_planes(U), planes, "empty move")
        assert np.array_equal(U.render(cam), frame)
        assert U.stats()["moves"] == 0
        # an upload in progress.  (Planes and frames are not comparable here: gsr_upload_begin itself gave the resident cloud up, and
        # after the abort there is no geometry.  What can be held: the refusal, its text, that the refused move did not disturb the
        # open upload's abort, that a move is refused after the abort too, and that the context then takes an upload and a
        # move as a fresh one does.)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert call(U, 0, 1) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
        assert call(U, 0, 1) == GSR_E_INVALID                       # (the aborted upload left zero splats: no range is within them)
        U.upload(A)
        _assert_same_planes(_planes(U), planes, "uploaded again after the refused move")
        assert np.array_equal(U.render(cam), frame)
        edited = _move(pkg, U, A, B.P[50:200], 50)
        _assert_same_planes(_planes(U), _fresh_planes(pkg, edited), "moved after the refused move")
        assert np.array_equal(U.render(cam), _fresh_frames(pkg, edited, [cam])[0])
        assert U.stats()["moves"] == 1
    with pkg.Engine(0) as V:                                        # SH arrays for a cloud uploaded without SH
        V.upload(_cloud(pkg, 11, sh=False))
        planes, frame = _planes(V, sh=False), V.render(cam).copy()
        assert call(V, 0, N, shx=sh, shy=sh, shz=sh) == GSR_E_INVALID
        _assert_same_planes(_planes(V, sh=False), planes, "SH arrays without SH")
        assert np.array_equal(V.render(cam), frame), "SH arrays without SH"
    with pytest.raises(E.GsrError):
        E.move_arrays(P, alpha=B.alpha[:5])                          # mismatched lengths never reach the library


# ---- 9. several ranks ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_move_matches_single_context(pkg, clouds):
    A = clouds[0]
    E = pkg.engine
    cams = _cams(pkg, range(4))
    newP = _mirror(A.P)
    edited = _move(pkg, None, A, newP, 0)
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as M:
        M.upload(A)
        for c in cams[:2]:
            M.render(c)
        assert M.move(0, newP) == N
        got = [M.render(c).copy() for c in cams[2:]]
        st = [M.stats(r) for r in range(2)]
        assert [s["uploads"] for s in st] == [1, 1] and [s["moves"] for s in st] == [1, 1]
    want = _fresh_frames(pkg, edited, cams[2:])
    stale = _fresh_frames(pkg, A, cams[2:])
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k])
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"


# ---- 10. through the renderer verbs (GSplatRenderer::moveSplats on a GPU instance) ------------------------------------------------
def _shim_planes(pkg, R, sh=True):
    """the resident planes of the context behind a GSplatRenderer"""
    import types
    L = pkg.load_library()
    L.gsplat_renderer_engine.restype = C.c_void_p
    ctx = types.SimpleNamespace(L=L, h=C.c_void_p(L.gsplat_renderer_engine(R.h)))
    return {name: pkg.engine.Engine.debug_resident(ctx, k) for k, name in enumerate(PLANES) if sh or name != "colrow"}


def _shim_with(pkg, parts, origins):
    """a GPU renderer with one registered row per part (details 0x100, 0x101, ...: the plan packs them in that order)"""
    R = pkg.GSplatRenderer(0)
    return R, [R.registerUpdate(0x100 + k, (1, 0, 0, 0), 0, p, o) for k, (p, o) in enumerate(zip(parts, origins))]


@pytest.mark.gpu
def test_shim_move_in_place_then_restage(pkg, clouds):
    """two rows resident; the second is moved in place (no staging), with a new origin and new opacities, which equals a fresh renderer
    holding the moved arrays, planes and frame; a forced re-stage then uploads the arrays the row holds NOW"""
    A, B, _ = clouds
    cam = _cams(pkg, [2])[0]
    a, b = A.subset(slice(0, 200)), A.subset(slice(200, N))
    eb = _copy(pkg, b)
    eb.P[:], eb.alpha[:] = _mirror(A.P)[200:], B.alpha[200:]
    oa, ob, ob2 = (0.0, 0.0, 0.0), (0.5, 0.25, -0.5), (-0.25, 1.0, 0.125)
    R, (ia, ib) = _shim_with(pkg, (a, b), (oa, ob))
    F, fids = _shim_with(pkg, (a, eb), (oa, ob2))
    G, gids = _shim_with(pkg, (eb,), (ob2,))
    try:
        before = R.frame(cam, [ia, ib]).copy()
        assert R.moveSplats(ib, eb.P, origin=ob2, alpha=eb.alpha) == (1, 200, N - 200)
        assert R.query(R.Q_STAGING_COUNT) == 1 and R.query(R.Q_LAST_STATUS) == 0
        got = R.frame(cam, [ia, ib]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 1                       # in place: the redraw staged nothing
        want = F.frame(cam, fids).copy()
        assert np.array_equal(R.origin(), F.origin())
        assert np.array_equal(got, want) and not np.array_equal(got, before)
        _assert_same_planes(_shim_planes(pkg, R), _shim_planes(pkg, F), "shim, moved in place")
        st = R.engine_stats()
        assert st["uploads"] == 1 and st["moves"] == 1
        # a re-stage (only the second row is shown now) uploads what the row holds: the moved arrays
        got = R.frame(cam, [ib]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 2
        assert np.array_equal(got, G.frame(cam, gids))
        _assert_same_planes(_shim_planes(pkg, R), _shim_planes(pkg, G), "shim, re-staged after the move")
    finally:
        R.close(); F.close(); G.close()
