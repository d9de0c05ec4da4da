"""gsr_transform on the GPU: selected resident splats rotated, scaled and translated where they are, no re-upload.

Everything is BIT-EXACT, in the style of tests/test_move_gpu.py.  Context U uploads cloud A and transforms it; a fresh context F uploads
engine.transform_eval of A -- the host evaluation of the functions the kernel evaluates -- under the same options.  The resident planes
(gsr_debug_read_resident) and the storage order are the same, and so is every later frame.

The clouds: 357 splats = five full clusters of 64 and one of 37; frames of 96 x 64 pixels on the parity tests' orbit."""
import ctypes as C

import numpy as np
import pytest

import test_move_gpu as M
import transform_cases as TC
from helpers import HipBuffers

N, W, H = M.N, M.W, M.H
GSR_E_INVALID = -1
assert N == TC.N


def _xf(pkg, name):
    return TC.make_xform(pkg, name)


def _popcount(mask, n=N):
    return int(TC.selected(mask, n).sum())


def _transformed_planes(pkg, A, x, mask, order=1, sh=True, prepare=None):
    """(planes before, planes after, the count the verb returned) of a context that uploads A and transforms it"""
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        if prepare:
            prepare(U)
        U.upload(A)
        before = M._planes(U, sh)
        moved = U.transform(x, mask)
        st = U.stats()
        assert st["uploads"] == 1 + (1 if prepare else 0) and st["moves"] == 0        # a transform is neither an upload nor a move
        return before, M._planes(U, sh), moved


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
@pytest.mark.parametrize("name", list(TC.TRANSFORMS))
def test_resident_bits(pkg, name, sh, order):
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh)
    x = _xf(pkg, name)
    for mname, mask in TC.masks(pkg).items():
        label = f"{name} / {mname} order {order} sh {sh}"
        before, got, moved = _transformed_planes(pkg, A, x, mask, order, sh)
        assert moved == _popcount(mask), label
        M._assert_same_planes(got, M._fresh_planes(pkg, E.transform_eval(x, A, mask), order, sh), label)
        if mname != "empty" and name != "identity":
            changed = any(not np.array_equal(before[k], got[k]) for k in ("geoA", "geoB", "col"))
            assert changed, f"{label}: the transform changed nothing: the case tests nothing"
        if mname == "empty":
            M._assert_same_planes(got, before, label)
        if order == 1 and name == "rotate" and mname == "null":
            assert not np.array_equal(before["order"], got["order"]), "the storage order did not change: the case tests nothing"
        if order == 0:
            assert np.array_equal(got["order"].view(np.int32), np.arange(N, dtype=np.int32))


# ---- 2. sizes at the edges ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_small_clouds(pkg, n):
    E = pkg.engine
    A = M._cloud(pkg, 11, n=n)
    x = _xf(pkg, "all")
    for mname, mask in TC.masks(pkg, n).items():
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.transform(x, mask) == _popcount(mask, n), (n, mname)
            got = M._planes(U)
        M._assert_same_planes(got, M._fresh_planes(pkg, E.transform_eval(x, A, mask)), f"n = {n} / {mname}")


@pytest.mark.gpu
def test_capacity_above_the_count(pkg):
    """the colour chunks are strided by the capacity, not by n: a context that held 1000 splats and now holds 357, and one that an
    add grew"""
    E = pkg.engine
    A, big = M._cloud(pkg, 11), M._cloud(pkg, 12, n=1000)
    x = _xf(pkg, "all")
    mask = TC.masks(pkg)["every_third"]
    want = M._fresh_planes(pkg, E.transform_eval(x, A, mask))
    _, got, moved = _transformed_planes(pkg, A, x, mask, prepare=lambda U: U.upload(big))
    assert moved == _popcount(mask)
    M._assert_same_planes(got, want, "a context that held 1000 splats before")
    with pkg.Engine(0) as U:
        U.upload(A.subset(slice(0, 200)))
        assert U.add(A.subset(slice(200, N))) == N and U.get_add()["grows"] == 1
        assert U.transform(x, mask) == _popcount(mask)
        got = M._planes(U)
    M._assert_same_planes(got, want, "a context an add grew")


# ---- 3. host, device and pinned masks ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_device_and_pinned_masks(pkg):
    E = pkg.engine
    L = pkg.load_library()
    A = M._cloud(pkg, 11)
    x = _xf(pkg, "all")
    sel = TC.masks(pkg)["every_third"]
    words = E.pack_mask(sel)
    guard = np.full(64, 0xdeadbeef, np.uint32)
    want = M._fresh_planes(pkg, E.transform_eval(x, A, sel))
    hb = HipBuffers()
    pinned = C.c_void_p()
    try:
        dev = hb.upload(np.concatenate([words, guard]))
        assert hb.hip.hipHostMalloc(C.byref(pinned), C.c_size_t(words.nbytes), 0) == 0
        C.memmove(pinned, words.ctypes.data, words.nbytes)
        with pkg.Engine(0) as U:
            U.upload(A)
            planes = M._planes(U)
            moved = C.c_int64(-7)
            assert not U.check_device_source(words.ctypes.data, words.nbytes)
            assert L.gsr_transform(U.h, C.c_void_p(words.ctypes.data), 1, C.byref(x), C.byref(moved)) == GSR_E_INVALID      # a pageable pointer
            assert b"gsr_transform" in L.gsr_last_error() and moved.value == -7
            M._assert_same_planes(M._planes(U), planes, "a pageable pointer as a device mask")
            assert U.get_transform()["transforms"] == 0
            assert U.transform_device(x, dev) == _popcount(sel)
            assert U.get_transform()["moved_last"] == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "device mask")
        back = hb.download(dev, (words.size + 64,), np.uint32)
        assert np.array_equal(back[:words.size], words) and np.array_equal(back[words.size:], guard), "the device mask was written"
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.transform_device(x, pinned.value) == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "pinned mask")
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.transform(x, words) == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "host mask, packed words")
    finally:
        if pinned.value:
            hb.hip.hipHostFree(pinned)
        hb.free()


# ---- 4. an empty selection ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_empty_selection_changes_and_invalidates_nothing(pkg):
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [1])[0]
    x = _xf(pkg, "all")
    with pkg.Engine(0) as U:
        U.upload(A)
        planes = M._planes(U)
        a = U.render(cam).copy()
        U.render(cam)
        st = U.stats()
        assert st["sorts_skipped"] == 1
        assert U.transform(x, np.zeros(N, bool)) == 0
        garbage = np.zeros((N + 31) // 32, np.uint32)
        garbage[-1] = np.uint32((0xffffffff << (N % 32)) & 0xffffffff)  # only bits behind n
        assert U.transform(x, garbage) == 0
        M._assert_same_planes(M._planes(U), planes, "nothing selected")
        assert np.array_equal(U.render(cam), a)
        st2 = U.stats()
        assert st2["sorts_skipped"] == 2, "the cached order did not survive a transform of nothing"
        for k in ("uploads", "moves", "n_splats"):
            assert st2[k] == st[k], k
        assert st2["move_ms"] == st["move_ms"]
        tr = U.get_transform()
        assert tr["transforms"] == 2 and tr["moved_last"] == 0


# ---- 5. frames afterwards ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "cull 0", "cull 3", "lazy 0", "rgba16f", "depth-tested"])
def test_frames_after_a_transform(pkg, mode):
    """two frames leave horizons, hints, cached orders and policies behind; then a third of the cloud is turned, resized and moved about
    a pivot, and every later frame is that of a fresh upload of the evaluated arrays"""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    modes = dict(M._frame_modes(pkg), default=((), None, None))
    opts, render, prepare = modes[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = M._cams(pkg, range(6))
    x = E.xform(axis_angle=((1.0, 2.0, 3.0), 37.0), scale=1.4, translate=(0.1, -0.05, 0.08), pivot=(0.1, 0.0, -0.1))
    mask = TC.masks(pkg)["every_third"]
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:2]:
            draw(U, c)
        assert U.transform(x, mask) == _popcount(mask)
        got = [draw(U, c).copy() for c in cams[2:]]
    want = M._fresh_frames(pkg, E.transform_eval(x, A, mask), cams[2:], opts, render=render, prepare=prepare)
    stale = M._fresh_frames(pkg, A, cams[2:], opts, render=render, prepare=prepare)
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the transform does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode}: frame {k} after the transform differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


# ---- 6. chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_transforms_in_a_row(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    x1, x2 = _xf(pkg, "all"), _xf(pkg, "rotate")
    m1, m2 = TC.masks(pkg)["range_50_200"], TC.masks(pkg)["every_third"]
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.transform(x1, m1) == 150 and U.transform(x2, m2) == _popcount(m2)
        assert U.get_transform()["transforms"] == 2
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, E.transform_eval(x2, E.transform_eval(x1, A, m1), m2)), "eval o eval")


@pytest.mark.gpu
def test_select_then_transform_then_read(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [1])[0]
    x = _xf(pkg, "all")
    hb = HipBuffers()
    try:
        dev = hb.upload(np.zeros((N + 31) // 32, np.uint32))
        with pkg.Engine(0) as U:
            U.upload(A)
            n_hit, n_set = U.select_device(cam, E.select_region(rect=(0.0, 0.0, W / 2.0, float(H))), dev)
            sel = E.unpack_mask(hb.download(dev, ((N + 31) // 32,), np.uint32), N)
            assert 10 < n_hit == n_set == int(sel.sum()) < N - 10
            assert U.transform_device(x, dev) == n_hit
            got = U.read()
    finally:
        hb.free()
    want = E.transform_eval(x, A, sel)
    for k in ("P", "Cd", "alpha", "scale", "orient"):
        assert np.array_equal(getattr(got, k).view(np.uint8), getattr(want, k).view(np.uint8)), k
    for k in ("shx", "shy", "shz"):
        assert np.array_equal(getattr(got, k)[:, :15], getattr(want, k)[:, :15]), k


@pytest.mark.gpu
def test_transform_remove_add_transform(pkg):
    E = pkg.engine
    A, B = M._cloud(pkg, 11), M._cloud(pkg, 12, n=90)
    x1, x2 = _xf(pkg, "all"), _xf(pkg, "scale_half")
    m1 = TC.masks(pkg)["every_third"]
    gone = np.arange(N) % 4 == 1
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.transform(x1, m1) == _popcount(m1)
        s = E.transform_eval(x1, A, m1)
        assert U.remove(gone) == N - int(gone.sum())
        s = s.subset(~gone)
        assert U.add(B) == s.n + B.n
        s = s.concat(B)
        m2 = np.arange(s.n) >= s.n - 120                                # the new splats and some old ones
        assert U.transform(x2, m2) == 120
        s = E.transform_eval(x2, s, m2)
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, s), "transform, remove, add, transform")


@pytest.mark.gpu
def test_update_orient_then_transform(pkg):
    E = pkg.engine
    A, B = M._cloud(pkg, 11), M._cloud(pkg, 12)
    x = _xf(pkg, "rotate")
    mask = TC.masks(pkg)["range_50_200"]
    s = M._copy(pkg, A)
    s.orient[100:260] = B.orient[100:260]
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.update_attrs(100, orient=s.orient[100:260]) == 160
        assert U.transform(x, mask) == 150
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, E.transform_eval(x, s, mask)), "update_attrs of orient, then a transform")


# ---- 7. a visibility in force ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_transform_under_a_visibility(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, [1, 2])
    volumes = [E.crop_box((-1.0, 0.0, 0.0), (1.0, 4.0, 4.0))]          # the half of the cloud with x < 0
    inside = E.visibility_eval(E.visibility_struct(volumes)[0], A.P)
    assert 0.3 <= inside.mean() <= 0.7
    x = E.xform(translate=(5.0, 0.0, 0.0))                              # ... carried out of the box
    want = E.transform_eval(x, A, inside)
    assert not E.visibility_eval(E.visibility_struct(volumes)[0], want.P).any()
    with pkg.Engine(0) as U, pkg.Engine(0) as F:
        U.upload(A)
        U.set_visibility(volumes=volumes)
        assert U.get_visibility()[1] == int((~inside).sum())
        U.render(cams[0])
        assert U.transform(x, inside) == int(inside.sum())
        F.upload(want)
        F.set_visibility(volumes=volumes)
        assert U.get_visibility()[1] == F.get_visibility()[1] == N      # every splat is outside now
        M._assert_same_planes(M._planes(U), M._planes(F), "a visibility in force: the resident opacities")
        for c in cams:
            assert np.array_equal(U.render(c), F.render(c))
        assert np.array_equal(U.read(names=("alpha",)).alpha.view(np.uint32), A.alpha.view(np.uint32)), "the true alphas"
        U.set_visibility()
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, want), "the visibility cleared after a transform")


# ---- 8. non-finite data ------------------------------------------------------------------------------------------------------
def _nan_aware_equal(got, want, dtype):
    g, w = np.ascontiguousarray(got).view(dtype), np.ascontiguousarray(want).view(dtype)
    bits = {2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]
    both_nan = np.isnan(g) & np.isnan(w)
    return bool(((g.view(bits) == w.view(bits)) | both_nan).all())


@pytest.mark.gpu
def test_non_finite_data_follows_the_arithmetic(pkg):
    """a selected splat with P.x = inf and one with a NaN orient half: the planes are F's, a half or float that is NaN on one side
    being NaN on the other (sign and payload unspecified); the never-cull flags of their clusters are compared exactly"""
    E = pkg.engine
    A = M._copy(pkg, M._cloud(pkg, 11))
    A.P[70, 0] = np.inf
    A.orient[200, 1] = 0x7e01
    x = _xf(pkg, "all")
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.transform(x, None) == N
        got = M._live(M._planes(U))
    want = M._live(M._fresh_planes(pkg, E.transform_eval(x, A, None)))
    assert np.array_equal(got["order"], want["order"])
    assert np.array_equal(got["clusB"], want["clusB"]), "cluster hi / never-cull flags"
    assert np.array_equal(got["clusA"], want["clusA"])
    assert np.array_equal(got["col"], want["col"])
    assert _nan_aware_equal(got["geoA"], want["geoA"], np.float32)
    assert _nan_aware_equal(got["geoB"], want["geoB"], np.float16)
    gr, wr = got["colrow"].reshape(-1, 128), want["colrow"].reshape(-1, 128)
    assert _nan_aware_equal(gr[:, :16], wr[:, :16], np.float32) and np.array_equal(gr[:, 16:], wr[:, 16:])
    flags = want["clusB"].view(np.float32).reshape(-1, 4)[:, 3]
    assert flags.sum() >= 1, "no cluster is flagged never-cull: the case tests nothing"
    assert np.isnan(want["geoB"].view(np.float16)).any()


# ---- 9. several ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_transform_matches_single_context(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, range(4))
    x = E.xform(axis_angle=((1.0, 2.0, 3.0), 37.0), scale=1.4, translate=(0.1, -0.05, 0.08), pivot=(0.1, 0.0, -0.1))
    mask = TC.masks(pkg)["every_third"]
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(A)
        for c in cams[:2]:
            Mu.render(c)
        assert Mu.transform(x, mask) == _popcount(mask)
        got = [Mu.render(c).copy() for c in cams[2:]]
        st = [Mu.stats(r) for r in range(2)]
        assert [s["uploads"] for s in st] == [1, 1] and [s["moves"] for s in st] == [0, 0]
    want = M._fresh_frames(pkg, E.transform_eval(x, A, mask), cams[2:])
    stale = M._fresh_frames(pkg, A, cams[2:])
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k])
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"


# ---- 10. refusals with a live context ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_alone(pkg):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    L = pkg.load_library()
    cam = M._cams(pkg, [2])[0]
    x = _xf(pkg, "all")
    words = E.pack_mask(TC.masks(pkg)["every_third"])
    moved = C.c_int64(-7)
    with pkg.Engine(0) as U:
        assert L.gsr_transform(U.h, words.ctypes.data, 0, C.byref(x), C.byref(moved)) == GSR_E_INVALID       # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes, frame = M._planes(U), U.render(cam).copy()
        bad = E.xform(scale=-1.0)
        nan = E.xform()
        nan.translate[1] = np.nan
        cases = {
            "NULL ctx": lambda: L.gsr_transform(None, words.ctypes.data, 0, C.byref(x), C.byref(moved)),
            "NULL x": lambda: L.gsr_transform(U.h, words.ctypes.data, 0, None, C.byref(moved)),
            "a negative scale": lambda: L.gsr_transform(U.h, words.ctypes.data, 0, C.byref(bad), C.byref(moved)),
            "a NaN field": lambda: L.gsr_transform(U.h, None, 0, C.byref(nan), C.byref(moved)),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            assert moved.value == -7, label
            M._assert_same_planes(M._planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        assert U.get_transform()["transforms"] == 0
        assert L.gsr_transform(U.h, words.ctypes.data, 0, C.byref(x), None) == 0                            # n_moved may be NULL
        assert U.get_transform()["transforms"] == 1
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert L.gsr_transform(U.h, words.ctypes.data, 0, C.byref(x), C.byref(moved)) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "uploaded again after the refused transform")
        assert np.array_equal(U.render(cam), frame)
