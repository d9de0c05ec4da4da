"""Visibility on the GPU (gsr_set_visibility): resident splats hidden by crop volumes or a mask, without a re-upload.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of the cloud, then the verbs
under test -- and a fresh context F that was uploaded the same arrays with alpha[i] replaced by visible(i) ? alpha[i] : +0.0f, where
visible comes from engine.visibility_eval (the host statement of the rule): the resident planes (gsr_debug_read_resident) are the
same bytes, and so is every later frame, whatever the frame's regime.

Clouds: 357 splats (five full clusters and one of 37), 65 without SH (no colour rows), a single splat, 4099 (17 workgroups of
k_visibility and a partial last wave); frames of 96 x 64 pixels on the parity tests' orbit.  Every case asserts from visibility_eval
that it hides at least 5 % and keeps at least 5 % of its cloud (a cloud of fewer than two splats is exempt)."""
import ctypes as C

import numpy as np
import pytest

import test_attr_update_gpu as T
from helpers import HipBuffers

W, H = T.W, T.H
INVALID = -1
CLOUDS = {"357": (357, 11, True), "65 no SH": (65, 11, False), "1": (1, 11, True), "4099": (4099, 21, True)}
CASES = ("BOX", "HALF", "ELL", "BOX-ELL")


def _roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _volumes(E, case, invert=False):
    box = E.crop_box((0, 0, 0), 0.6, invert=invert and case == "BOX")
    ell = lambda inv: E.crop_ellipsoid((0.1, -0.1, 0), (0.9, 0.5, 0.7), _roty(30), invert=inv)   # (rotated: to_unit is not dyadic)
    return {"BOX": [box], "HALF": [E.crop_box((0.5, 0, 0), (0.5, 2, 2))], "ELL": [ell(invert)], "BOX-ELL": [box, ell(True)]}[case]


def _make(pkg, key):
    n, seed, sh = CLOUDS[key]
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-3.5, -2.0))


def _every_third(n):
    hidden = np.zeros(n, bool)
    hidden[::3] = True
    return hidden


def _visible(pkg, s, volumes=(), hidden=None):
    """the rule on the host, with the guard against a vacuous case"""
    E = pkg.engine
    v, keep = E.visibility_struct(volumes, hidden)
    vis = E.visibility_eval(v, s.P)
    if s.P.shape[0] >= 2:
        assert 0.05 <= vis.mean() <= 0.95, f"the case keeps {vis.mean():.3f} of the cloud: it tests nothing"
    return vis


def _effective(pkg, s, vis):
    out = T._copy(pkg, s)
    out.alpha = np.where(vis, s.alpha, np.float32(0.0)).astype(np.float32)
    return out


def _fresh_planes(pkg, s, order, sh):
    return T._fresh_planes(pkg, s, order, sh)


def _fresh(pkg, s, order=1, sh=True):
    """(planes, storage order) of a fresh context uploaded s"""
    with pkg.Engine(0) as F:
        F.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        F.upload(s)
        return T._planes(F, sh), F.debug_storage_order(s.P.shape[0])


def _hidden_count(U):
    return U.get_visibility()[1]


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("key", list(CLOUDS))
def test_resident_bits(pkg, key, order):
    """one context goes through every volume case -- alone, a mask alone, volume plus mask -- one after the other (so every
    application starts from the one before), then is cleared"""
    E = pkg.engine
    s = _make(pkg, key)
    n, sh = s.P.shape[0], CLOUDS[key][2]
    third = _every_third(n)
    plain = _fresh_planes(pkg, s, order, sh)
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_STORAGE_ORDER, order)
        U.upload(s)
        T._assert_same_planes(T._planes(U, sh), plain, f"{key}: the plain upload")
        steps = []
        for case in CASES:
            steps += [(case, _volumes(E, case), None), (case + " + mask", _volumes(E, case), third)]
        steps.insert(1, ("mask alone", [], third))
        for label, vols, hidden in steps:
            vis = _visible(pkg, s, vols, hidden)
            U.set_visibility(volumes=vols, mask=hidden)
            got = T._planes(U, sh)
            T._assert_same_planes(got, _fresh_planes(pkg, _effective(pkg, s, vis), order, sh), f"{key} order {order}: {label}")
            assert _hidden_count(U) == int((~vis).sum()), label
            v = U.get_visibility()[0]
            assert v.n_volumes == len(vols) and not v.mask and v.mask_splats == (n if hidden is not None else 0)
            if n >= 2:
                assert not np.array_equal(got["geoA"], plain["geoA"]), "nothing was hidden"
            U.set_visibility(volumes=vols, mask=hidden)                 # the same again changes nothing
            T._assert_same_planes(T._planes(U, sh), got, f"{label}, set twice")
            assert _hidden_count(U) == int((~vis).sum())
        assert U.stats()["uploads"] == 1
        U.set_visibility()
        T._assert_same_planes(T._planes(U, sh), plain, f"{key} order {order}: cleared")
        assert U.get_visibility()[0].n_volumes == 0 and _hidden_count(U) == 0
        U.set_visibility(E.visibility_struct([])[0])                     # no volume and no mask: cleared as well, again
        T._assert_same_planes(T._planes(U, sh), plain, "cleared twice")


# ---- 2. positions on the boundary ----------------------------------------------------------------------------------------------------
def _boundary_cloud(pkg, nonfinite):
    """128 splats; the first 40 positions: on each of the six faces of BOX the five floats around the face (the float nearest 0.6
    and its two neighbours on either side: 1 / 0.6 is not a float, so which of them is the last one inside is the rule's to say),
    points on an edge and at a corner, signed zeros and tiny coordinates, a NaN and an inf position (or, without them, two ordinary
    points: then the cloud is Morton-ordered), and -0 / sub-1/255 alphas on both sides of the faces"""
    s = pkg.scenes.make_scene(128, seed=11, sh=True, log_scale_range=(-3.5, -2.0))
    f = np.float32(0.6)
    lo, hi = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))
    lo2, hi2 = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))
    pts = []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            for v in (lo2, lo, f, hi, hi2):
                p = np.array([0.125, -0.25, 0.375], np.float32)
                p[ax] = sgn * v
                pts.append(p)
    pts += [[f, f, 0], [hi2, lo2, 0], [lo2, lo2, lo2], [-lo2, lo2, -hi2]]                                          # an edge, corners
    pts += [[0.0, -0.0, 1e-30], [-0.0, 0.5, -0.5], [1e-30, -1e-30, 0.0], [0.5, 0.5, 0.5]]
    assert len(pts) == 38
    pts += [[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1]] if nonfinite else [[0.59, 0.1, 0.1], [0.1, 0.61, 0.1]]
    s.P[:40] = np.asarray(pts, np.float32)
    s.alpha[0:40:4] = np.float32(-0.0)
    s.alpha[1:40:4] = np.float32(1.0 / 256.0)                           # below 1/255: K1 drops it, the resident bits keep it
    s.alpha[2:40:8] = np.float32(1e-30)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("nonfinite", (True, False))
def test_positions_on_the_boundary(pkg, nonfinite):
    """where a contracted or re-ordered FMA chain on either side would show"""
    E = pkg.engine
    s = _boundary_cloud(pkg, nonfinite)
    with pkg.Engine(0) as U:
        U.upload(s)
        for label, vols in (("BOX", _volumes(E, "BOX")), ("BOX inverted", _volumes(E, "BOX", invert=True)), ("ELL", _volumes(E, "ELL"))):
            vis = _visible(pkg, s, vols)
            if label == "BOX":
                # every face has floats on both sides among its five, inside first -- or the 40 positions decide nothing
                head = vis[:30].reshape(6, 5)
                assert head[:, 0].all() and not head[:, 4].any() and (np.diff(head.astype(int), axis=1) <= 0).all(), head
                assert not vis[38:40].any() or not nonfinite
            U.set_visibility(volumes=vols)
            T._assert_same_planes(T._planes(U), _fresh_planes(pkg, _effective(pkg, s, vis), 1, True), f"boundary, {label}")
            assert _hidden_count(U) == int((~vis).sum())
        U.set_visibility()
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, s, 1, True), "boundary, cleared (-0 and tiny alphas come back as they were)")


# ---- 3. frames ---------------------------------------------------------------------------------------------------------------------
def _frame_runs(E):
    return {
        "default policy": dict(opts=()),
        "no occlusion culling": dict(opts=((E.OPT_OCCLUSION_CULL, 0),)),
        "front-slab frames": dict(opts=((E.OPT_OCCLUSION_CULL, 3),)),
        "forced front slab": dict(opts=((E.OPT_FRONT_SLAB, 2),)),
        "lazy colour always": dict(opts=((E.OPT_LAZY_COLOUR, 2),)),
        "two frames in flight": dict(opts=((E.OPT_FRAMES_IN_FLIGHT, 2),)),
        "render_depth": dict(opts=(), depth=True),
        "RGBA16F": dict(opts=(), fmt=E.TARGET_RGBA16F),
        "row band": dict(opts=(), band=(1, 2)),
    }


FRAME_RUNS = ("default policy", "no occlusion culling", "front-slab frames", "forced front slab", "lazy colour always",
              "two frames in flight", "render_depth", "RGBA16F", "row band")


def _setup(E, eng, run):
    for k, v in run["opts"]:
        eng.set_option(k, v)
    if "fmt" in run:
        eng.set_target_format(run["fmt"])
    if "band" in run:
        eng.set_row_band(*run["band"])


def _render(pkg, eng, run, cam):
    if run.get("depth"):
        return eng.render_depth(cam, pkg.scenes.sphere_occluder_depth(cam, 3.42, 0.645)).copy()
    return eng.render(cam).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FRAME_RUNS)
def test_frames(pkg, name):
    """12 consecutive orbit frames on one context: BOX, after four frames BOX and not ELL, after eight everything visible again"""
    E = pkg.engine
    run = _frame_runs(E)[name]
    s = _make(pkg, "357")
    cams = T._cams(pkg, range(12))
    phases = [_volumes(E, "BOX"), _volumes(E, "BOX-ELL"), []]
    got, want, plain = [], [], []
    with pkg.Engine(0) as U:
        _setup(E, U, run)
        U.upload(s)
        for p, vols in enumerate(phases):
            U.set_visibility(volumes=vols)
            got += [_render(pkg, U, run, c) for c in cams[4 * p:4 * p + 4]]
        assert U.stats()["uploads"] == 1
    for p, vols in enumerate(phases):
        eff = _effective(pkg, s, _visible(pkg, s, vols)) if vols else s
        with pkg.Engine(0) as F:
            _setup(E, F, run)
            F.upload(eff)
            want += [_render(pkg, F, run, c) for c in cams[4 * p:4 * p + 4]]
    with pkg.Engine(0) as F:
        _setup(E, F, run)
        F.upload(s)
        plain = [_render(pkg, F, run, c) for c in cams[:8]]
    for k in range(12):
        assert got[k].shape == want[k].shape and got[k].any(), (name, k)
        assert np.array_equal(got[k], want[k]), (f"{name}: frame {k} differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")
    for p in range(2):
        assert any(not np.array_equal(want[k], plain[k]) for k in range(4 * p, 4 * p + 4)), "the crop does not show: the case tests nothing"


# ---- 4. with the other verbs ---------------------------------------------------------------------------------------------------------
def _rotated(P):
    """the whole cloud turned 40 degrees about z and 25 about x (float32 rows)"""
    a, b = np.deg2rad(40.0), np.deg2rad(25.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.ascontiguousarray((P.astype(np.float64) @ (Rx @ Rz).T).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_alpha_update_while_cropped(pkg, order):
    """(a) new alphas for [50, 200) under BOX: the new alphas, then the rule; after clearing, the alphas edited while hidden are there"""
    E = pkg.engine
    s, src = _make(pkg, "357"), pkg.scenes.make_scene(357, seed=12, sh=True, log_scale_range=(-3.5, -2.0))
    box = _volumes(E, "BOX")
    vis = _visible(pkg, s, box)
    edited = T._copy(pkg, s)
    edited.alpha[50:200] = src.alpha[50:200]
    assert (~vis[50:200]).any() and vis[50:200].any()
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_STORAGE_ORDER, order)
        U.upload(s)
        U.set_visibility(volumes=box)
        assert U.update_attrs(50, alpha=src.alpha[50:200]) == 150
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, _effective(pkg, edited, vis), order, True), "alpha update under BOX")
        assert _hidden_count(U) == int((~vis).sum())
        # an update without alpha leaves the hidden set alone
        assert U.update_attrs(0, Cd=src.Cd[:100]) == 100
        edited.Cd[:100] = src.Cd[:100]
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, _effective(pkg, edited, vis), order, True), "Cd update under BOX")
        U.set_visibility()
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, edited, order, True), "cleared after the updates")
        assert U.stats()["uploads"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_move_while_cropped(pkg, order):
    """(b) the whole cloud rotated under BOX (and a mask, which a move keeps): the rule at the moved positions; then a part of the
    cloud moved together with new alphas"""
    E = pkg.engine
    s, src = _make(pkg, "357"), pkg.scenes.make_scene(357, seed=12, sh=True, log_scale_range=(-3.5, -2.0))
    box, third = _volumes(E, "BOX"), _every_third(357)
    moved = T._copy(pkg, s)
    moved.P = _rotated(s.P)
    vis0, vis1 = _visible(pkg, s, box, third), _visible(pkg, moved, box, third)
    assert not np.array_equal(vis0, vis1), "the move changes nobody's visibility: the case tests nothing"
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_STORAGE_ORDER, order)
        U.upload(s)
        U.set_visibility(volumes=box, mask=third)
        assert U.move(0, moved.P) == 357
        planes, perm = _fresh(pkg, _effective(pkg, moved, vis1), order)
        T._assert_same_planes(T._planes(U), planes, f"moved under BOX + mask, order {order}")
        assert np.array_equal(U.debug_storage_order(357), perm)
        assert _hidden_count(U) == int((~vis1).sum()) and U.get_visibility()[0].mask_splats == 357
        # [100, 300) back to where they were, with new alphas in the same call
        part = T._copy(pkg, moved)
        part.P[100:300], part.alpha[100:300] = s.P[100:300], src.alpha[100:300]
        vis2 = _visible(pkg, part, box, third)
        assert U.move(100, part.P[100:300], alpha=part.alpha[100:300]) == 200
        planes, perm = _fresh(pkg, _effective(pkg, part, vis2), order)
        T._assert_same_planes(T._planes(U), planes, f"part moved with alphas, order {order}")
        assert np.array_equal(U.debug_storage_order(357), perm)
        U.set_visibility()
        T._assert_same_planes(T._planes(U), _fresh(pkg, part, order)[0], "cleared after the moves")
        st = U.stats()
        assert st["uploads"] == 1 and st["moves"] == 2


@pytest.mark.gpu
def test_device_verbs_while_cropped(pkg):
    """(c) gsr_update_device / gsr_move_device under BOX, from float32 arrays in device memory"""
    E = pkg.engine
    s = _make(pkg, "357")
    rng = np.random.default_rng(5)
    new_alpha = rng.uniform(0.05, 1.0, 150).astype(np.float32)
    box = _volumes(E, "BOX")
    vis = _visible(pkg, s, box)
    edited = T._copy(pkg, s)
    edited.alpha[50:200] = new_alpha
    moved = T._copy(pkg, edited)
    moved.P = _rotated(s.P)
    vis1 = _visible(pkg, moved, box)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(s)
            U.set_visibility(volumes=box)
            assert U.update_attrs_device(50, n=150, alpha=hb.upload(new_alpha)) == 150
            T._assert_same_planes(T._planes(U), _fresh_planes(pkg, _effective(pkg, edited, vis), 1, True), "update_attrs_device under BOX")
            assert U.move_device(0, hb.upload(moved.P), n=357) == 357
            planes, perm = _fresh(pkg, _effective(pkg, moved, vis1))
            T._assert_same_planes(T._planes(U), planes, "move_device under BOX")
            assert np.array_equal(U.debug_storage_order(357), perm)
            assert _hidden_count(U) == int((~vis1).sum())
            U.set_visibility()
            T._assert_same_planes(T._planes(U), _fresh_planes(pkg, moved, 1, True), "cleared after the device verbs")
    finally:
        hb.free()


@pytest.mark.gpu
def test_reupload_keeps_the_volumes_and_drops_the_mask(pkg):
    """(d) another cloud of another size while BOX and a mask are in force, then one whose capacity must grow"""
    E = pkg.engine
    s, small, large = _make(pkg, "357"), pkg.scenes.make_scene(200, seed=13, sh=True, log_scale_range=(-3.5, -2.0)), _make(pkg, "4099")
    box = _volumes(E, "BOX")
    with pkg.Engine(0) as U:
        U.upload(s)
        U.set_visibility(volumes=box, mask=_every_third(357))
        assert U.get_visibility()[0].mask_splats == 357
        for label, cloud in (("a smaller cloud", small), ("a cloud beyond the capacity", large), ("the first cloud again", s)):
            n = cloud.P.shape[0]
            vis = _visible(pkg, cloud, box)
            U.upload(cloud)
            T._assert_same_planes(T._planes(U), _fresh_planes(pkg, _effective(pkg, cloud, vis), 1, True), f"re-upload: {label}")
            v, hidden = U.get_visibility()
            assert v.n_volumes == 1 and v.volume[0].kind == E.VOL_BOX and v.mask_splats == 0 and hidden == int((~vis).sum()), label
            assert np.array_equal(np.array(v.volume[0].to_unit[:], np.float32), box[0][2])
        U.set_visibility()
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, s, 1, True), "cleared after the re-uploads")
        # a mask alone is dropped by an upload: nothing is in force afterwards
        U.set_visibility(mask=_every_third(357))
        assert _hidden_count(U) == 119
        U.upload(small)
        assert U.get_visibility()[0].mask_splats == 0 and _hidden_count(U) == 0
        T._assert_same_planes(T._planes(U), _fresh_planes(pkg, small, 1, True), "a mask alone, then an upload")


@pytest.mark.gpu
def test_volumes_set_before_the_first_upload(pkg):
    """(e)"""
    E = pkg.engine
    s = _make(pkg, "65 no SH")
    vols = _volumes(E, "BOX-ELL")
    vis = _visible(pkg, s, vols)
    with pkg.Engine(0) as U:
        U.set_visibility(volumes=vols)
        assert U.get_visibility()[0].n_volumes == 2 and _hidden_count(U) == 0
        U.upload(s)
        T._assert_same_planes(T._planes(U, False), _fresh_planes(pkg, _effective(pkg, s, vis), 1, False), "volumes before the upload")
        assert _hidden_count(U) == int((~vis).sum())
        cam = T._cams(pkg, [1])[0]
        got = U.render(cam).copy()
    with pkg.Engine(0) as F:
        F.upload(_effective(pkg, s, vis))
        assert np.array_equal(got, F.render(cam)) and got.any()


# ---- 5. several ranks, and the renderer verbs ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_matches_single_context(pkg):
    E = pkg.engine
    s = _make(pkg, "357")
    box = _volumes(E, "BOX")
    eff = _effective(pkg, s, _visible(pkg, s, box))
    cams = T._cams(pkg, range(3))
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as M:
        M.upload(s)
        M.render(cams[0])
        M.set_visibility(volumes=box)
        got = [M.render(c).copy() for c in cams[1:]]
        M.set_visibility()
        back = M.render(cams[2]).copy()
    want = T._fresh_frames(pkg, eff, cams[1:])
    plain = T._fresh_frames(pkg, s, cams[1:])
    for k in range(2):
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"
        assert not np.array_equal(want[k], plain[k])
    assert np.array_equal(back, plain[1])


def _shim_fresh(pkg, cloud, cam):
    """(frame, planes) of a fresh renderer showing `cloud`"""
    F = pkg.GSplatRenderer(0)
    try:
        rid = F.registerUpdate(0x100, (1, 0, 0, 0), 0, cloud, (0.0, 0.0, 0.0))
        frame = F.frame(cam, [rid]).copy()
        return frame, _shim_planes(pkg, F)
    finally:
        F.close()


def _shim_planes(pkg, R):
    import types
    L = pkg.load_library()
    L.gsplat_renderer_engine.restype = C.c_void_p
    ctx = types.SimpleNamespace(L=L, h=C.c_void_p(L.gsplat_renderer_engine(R.h)))
    return {name: pkg.engine.Engine.debug_resident(ctx, k) for k, name in enumerate(T.PLANES)}


@pytest.mark.gpu
def test_shim_keeps_the_crop_through_a_restage(pkg):
    E = pkg.engine
    s, other = _make(pkg, "357"), pkg.scenes.make_scene(300, seed=13, sh=True, log_scale_range=(-3.5, -2.0))
    box = _volumes(E, "BOX")
    cam = T._cams(pkg, [2])[0]
    origin = (0.0, 0.0, 0.0)
    R = pkg.GSplatRenderer(0)
    try:
        rid = R.registerUpdate(0x100, (1, 0, 0, 0), 0, s, origin)
        plain = R.frame(cam, [rid]).copy()
        masked, keep = E.visibility_struct(box, _every_third(357))
        assert R.setVisibility(masked) == INVALID                       # a mask would be lost by the next re-stage
        assert np.array_equal(R.frame(cam, [rid]), plain)
        assert R.setVisibility(E.visibility_struct(box)[0]) == 0
        got = R.frame(cam, [rid]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 1
        want, planes = _shim_fresh(pkg, _effective(pkg, s, _visible(pkg, s, box)), cam)
        assert np.array_equal(got, want) and not np.array_equal(got, plain)
        T._assert_same_planes(_shim_planes(pkg, R), planes, "shim, cropped in place")
        # a new version of the detail is re-staged: the crop holds for the new cloud
        rid2 = R.registerUpdate(0x100, (2, 0, 0, 0), 0, other, origin)
        got = R.frame(cam, [rid2]).copy()
        assert R.query(R.Q_STAGING_COUNT) == 2
        eff = _effective(pkg, other, _visible(pkg, other, box))
        want, planes = _shim_fresh(pkg, eff, cam)
        assert np.array_equal(got, want)
        T._assert_same_planes(_shim_planes(pkg, R), planes, "shim, re-staged under BOX")
        assert R.setVisibility(None) == 0
        assert np.array_equal(R.frame(cam, [rid2]), _shim_fresh(pkg, other, cam)[0])
    finally:
        R.close()


# ---- 6. refusals that need a context ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_refusals_leave_the_context_untouched(pkg):
    E = pkg.engine
    s = _make(pkg, "357")
    box = _volumes(E, "BOX")
    third = _every_third(357)
    L = pkg.load_library()

    def refused(U, v):
        rc = L.gsr_set_visibility(U.h, C.byref(v))
        assert rc == INVALID, rc
        return L.gsr_last_error().decode()

    with pkg.Engine(0) as U:
        v, keep = E.visibility_struct([], np.zeros(357, bool))
        assert "none is resident" in refused(U, v)                      # a mask before any upload
        U.upload(s)
        U.set_visibility(volumes=box)
        before = T._planes(U)
        state = U.get_visibility()
        for wrong in (356, 358, 0, -1):
            v, keep = E.visibility_struct([], third)
            v.mask_splats = wrong
            assert "mask covers" in refused(U, v)
        for bad in ("kind", "invert", "reserved_", "n_volumes"):
            v, keep = E.visibility_struct(_volumes(E, "HALF"))
            if bad == "kind":
                v.volume[0].kind = 9
            elif bad == "invert":
                v.volume[0].invert = 2
            elif bad == "reserved_":
                v.reserved_ = 7
            else:
                v.n_volumes = 5
            refused(U, v)
        T._assert_same_planes(T._planes(U), before, "after the refusals")
        now = U.get_visibility()
        assert now[1] == state[1] and bytes(now[0]) == bytes(state[0])
        # an upload in progress
        a = E._Arrays(s)
        E._check(L.gsr_upload_begin(U.h, a.n, 1, E._f3((0, 0, 0))))
        assert "upload in progress" in refused(U, E.visibility_struct(_volumes(E, "HALF"))[0])
        assert L.gsr_set_visibility(U.h, None) == INVALID
        E._check(L.gsr_upload_append(U.h, a.n, *a.ptrs()))
        E._check(L.gsr_upload_end(U.h))
        T._assert_same_planes(T._planes(U), before, "BOX is still what is in force after the refused calls")
        assert U.get_visibility()[0].n_volumes == 1
