"""gsr_grade on the GPU: the colour and the opacity of selected resident splats changed where they are, no re-upload.

Everything is BIT-EXACT, in the style of tests/test_transform_gpu.py.  Context U uploads cloud A and grades it; a FRESH context F uploads
engine.grade_eval of A -- the host evaluation of the functions the kernel evaluates -- under the same options.  The resident planes
(gsr_debug_read_resident), the storage order and the cluster bounds are the same, and so is every later frame.  The reference is never
the context under test.

The clouds: 357 splats = five full clusters of 64 and one of 37; frames of 96 x 64 pixels on the parity tests' orbit."""
import ctypes as C

import numpy as np
import pytest

import grade_cases as GC
import test_move_gpu as M
from helpers import HipBuffers

N, W, H = M.N, M.W, M.H
GSR_E_INVALID = -1
assert N == GC.N


def _popcount(mask, n=N):
    return int(GC.selected(mask, n).sum())


def _count(rule, mask, n=N):
    """what the verb returns: the bits set below n, 0 for a rule without flags"""
    return _popcount(mask, n) if rule["flags"] else 0


def _graded_planes(pkg, A, rule, mask, order=1, sh=True, prepare=None):
    """(planes before, planes after, the count the verb returned) of a context that uploads A and grades it"""
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        if prepare:
            prepare(U)
        U.upload(A)
        before = M._planes(U, sh)
        graded = U.grade(rule, mask)
        st = U.stats()
        assert st["uploads"] == 1 + (1 if prepare else 0) and st["moves"] == 0        # a grade is neither an upload nor a move
        return before, M._planes(U, sh), graded


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
@pytest.mark.parametrize("name", GC.RULES)
def test_resident_bits(pkg, name, sh, order):
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh)
    rule = GC.make_rule(pkg, name)
    mask = GC.masks(pkg)["every_third"]
    label = f"{name} / every_third order {order} sh {sh}"
    before, got, graded = _graded_planes(pkg, A, rule, mask, order, sh)
    assert graded == _count(rule, mask), label
    M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(rule, A, mask), order, sh), label)
    for k in ("geoB", "clusA", "clusB", "order"):                # no position, scale or orient changes: these stay
        assert np.array_equal(before[k], got[k]), (label, k)
    changed = any(not np.array_equal(before[k], got[k]) for k in ("geoA", "col"))
    assert changed == (name != "neutral"), f"{label}: changed = {changed}"


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_resident_bits_every_mask(pkg, sh, order):
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh)
    rule = GC.make_rule(pkg, "all")
    for mname, mask in GC.masks(pkg).items():
        label = f"all / {mname} order {order} sh {sh}"
        before, got, graded = _graded_planes(pkg, A, rule, mask, order, sh)
        assert graded == _popcount(mask), label
        M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(rule, A, mask), order, sh), label)
        if mname == "empty":
            M._assert_same_planes(got, before, label)


# ---- 2. sizes at the edges ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
@pytest.mark.parametrize("n", (1, 7, 8, 9, 63, 64, 65))
def test_small_clouds(pkg, n, sh):
    """eight splats per wave, 32 per mask word, 64 per workgroup"""
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh, n=n)
    rule = GC.make_rule(pkg, "all")
    for mname, mask in GC.masks(pkg, n).items():
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.grade(rule, mask) == _popcount(mask, n), (n, mname)
            got = M._planes(U, sh)
        M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(rule, A, mask), sh=sh), f"n = {n} / {mname} sh {sh}")


@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_capacity_above_the_count(pkg, sh):
    """the colour chunks are strided by the capacity, not by n: a context that held 357 splats and now holds 100"""
    E = pkg.engine
    big, A = M._cloud(pkg, 12, sh=sh), M._cloud(pkg, 11, sh=sh, n=100)
    rule = GC.make_rule(pkg, "all")
    mask = GC.masks(pkg, 100)["every_third"]
    _, got, graded = _graded_planes(pkg, A, rule, mask, sh=sh, prepare=lambda U: U.upload(big))
    assert graded == _popcount(mask, 100)
    M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(rule, A, mask), sh=sh), "a context that held 357 splats before")


# ---- 3. host, device and pinned masks ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_device_and_pinned_masks(pkg):
    E = pkg.engine
    L = pkg.load_library()
    A = M._cloud(pkg, 11)
    rule = GC.make_rule(pkg, "all")
    r = E._grade_rule_struct(rule)
    sel = GC.masks(pkg)["every_third"]
    words = E.pack_mask(sel)
    guard = np.full(64, 0xdeadbeef, np.uint32)
    want = M._fresh_planes(pkg, E.grade_eval(rule, A, sel))
    hb = HipBuffers()
    pinned = C.c_void_p()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.alloc(size)
        dev = hb.upload(np.concatenate([words, guard]))
        assert hb.hip.hipHostMalloc(C.byref(pinned), C.c_size_t(words.nbytes), 0) == 0
        C.memmove(pinned, words.ctypes.data, words.nbytes)
        with pkg.Engine(0) as U:
            U.upload(A)
            planes = M._planes(U)
            graded = C.c_int64(-7)
            # refused by the pointer check, before anything is launched (the pure query first: no verb is handed a pointer it would take)
            short = room + size - (words.size - 1) * 4                  # one word short of the end of its allocation
            for label, ptr in (("a pageable pointer", words.ctypes.data), ("one word short", short)):
                assert not U.check_device_source(ptr, words.nbytes), label
                assert L.gsr_grade(U.h, C.c_void_p(ptr), 1, C.byref(r), C.byref(graded)) == GSR_E_INVALID, label
                assert b"gsr_grade" in L.gsr_last_error() and graded.value == -7, label
                M._assert_same_planes(M._planes(U), planes, label)
            assert U.get_grade()["grades"] == 0
            assert U.grade_device(rule, dev) == _popcount(sel)
            assert U.get_grade()["graded_last"] == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "device mask")
        back = hb.download(dev, (words.size + 64,), np.uint32)
        assert np.array_equal(back[:words.size], words) and np.array_equal(back[words.size:], guard), "the device mask was written"
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.grade_device(rule, pinned.value) == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "pinned mask")
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.grade(rule, words) == _popcount(sel)
            M._assert_same_planes(M._planes(U), want, "host mask, packed words")
    finally:
        if pinned.value:
            hb.hip.hipHostFree(pinned)
        hb.free()


# ---- 4. no-ops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_work_changes_and_invalidates_nothing(pkg):
    """an empty mask, only bits behind n, a rule without flags and the neutral parameters: no resident bit, no cached order, no horizon
    and no policy changes"""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [1])[0]
    rule = GC.make_rule(pkg, "all")
    flagless = dict(rule, flags=0)
    garbage = np.zeros((N + 31) // 32, np.uint32)
    garbage[-1] = np.uint32((0xffffffff << (N % 32)) & 0xffffffff)      # only bits behind n
    with pkg.Engine(0) as U:
        U.upload(A)
        planes = M._planes(U)
        a = U.render(cam).copy()
        U.render(cam)
        st, pol = U.stats(), U.policy_state()
        assert st["sorts_skipped"] == 1
        assert U.grade(rule, np.zeros(N, bool)) == 0
        assert U.grade(rule, garbage) == 0
        assert U.grade(flagless, None) == 0
        assert U.grade(GC.make_rule(pkg, "neutral"), None) == 0
        assert U.grade(E.grade_prepare(E.grade_params()), GC.masks(pkg)["every_third"]) == 0
        M._assert_same_planes(M._planes(U), planes, "nothing to do")
        assert U.policy_state() == pol
        assert np.array_equal(U.render(cam), a)
        st2 = U.stats()
        assert st2["sorts_skipped"] == 2, "the cached order did not survive a grade of nothing"
        for k in ("uploads", "moves", "n_splats"):
            assert st2[k] == st[k], k
        gr = U.get_grade()
        assert gr["grades"] == 5 and gr["graded_last"] == 0


# ---- 5. frames afterwards ----------------------------------------------------------------------------------------------------
FRAME_RULES = {"colour": dict(exposure=0.6, gain=(1.3, 0.9, 0.6), saturation=1.4, contrast=1.2, pivot=0.4, offset=(0.05, 0.0, -0.05)),
               "colour+alpha": dict(exposure=0.6, gain=(1.3, 0.9, 0.6), saturation=1.4, alpha_gain=0.4, alpha_offset=0.02)}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(FRAME_RULES))
@pytest.mark.parametrize("mode", ["default", "cull 0", "cull 3", "lazy 0", "rgba16f", "depth-tested"])
def test_frames_after_a_grade(pkg, mode, what):
    """two frames leave horizons, prefixes, cached orders and policies behind; then a third of the cloud is graded, and every later
    frame is that of a fresh upload of the evaluated arrays.  A colour-only grade leaves the policies as they were."""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    modes = dict(M._frame_modes(pkg), default=((), None, None))
    opts, render, prepare = modes[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = M._cams(pkg, range(6))
    rule = E.grade_prepare(E.grade_params(**FRAME_RULES[what]))
    mask = GC.masks(pkg)["every_third"]
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:2]:
            draw(U, c)
        pol = U.policy_state()
        assert U.grade(rule, mask) == _popcount(mask)
        if what == "colour":
            assert U.policy_state() == pol, "a colour-only grade changed the policies"
        got = [draw(U, c).copy() for c in cams[2:]]
    want = M._fresh_frames(pkg, E.grade_eval(rule, A, mask), cams[2:], opts, render=render, prepare=prepare)
    stale = M._fresh_frames(pkg, A, cams[2:], opts, render=render, prepare=prepare)
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the grade does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode} / {what}: frame {k} after the grade differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
def test_static_camera_after_a_colour_grade(pkg):
    """the camera stands still, so the frame before the grade left a cached depth order whose records hold the old colours"""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [3])[0]
    rule = GC.make_rule(pkg, "tint")
    with pkg.Engine(0) as U:
        U.upload(A)
        U.render(cam)
        U.render(cam)
        assert U.stats()["sorts_skipped"] == 1
        assert U.grade(rule, None) == N
        got = [U.render(cam).copy() for _ in range(2)]
    want = M._fresh_frames(pkg, E.grade_eval(rule, A, None), [cam, cam])
    stale = M._fresh_frames(pkg, A, [cam])[0]
    for k in range(2):
        assert not np.array_equal(want[k], stale) and np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
def test_frames_after_an_alpha_grade_occlusion_cull_always(pkg):
    """GSR_OPT_OCCLUSION_CULL = 2: horizons left by the opaque cloud must not cull what the lower alpha of the nearest third uncovers"""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, range(5))
    d = np.linalg.norm(A.P.astype(np.float64) - np.asarray(cams[3].cam_pos, np.float64), axis=1)
    near = np.zeros(N, bool)
    near[np.argsort(d, kind="stable")[:N // 3]] = True
    rule = E.grade_rule(np.eye(3), alpha_gain=0.0)                      # the nearest third turned transparent
    opts = ((E.OPT_OCCLUSION_CULL, 2),)
    with pkg.Engine(0) as U:
        U.set_option(*opts[0])
        U.upload(A)
        for c in cams[:3]:
            U.render(c)
        assert U.grade(rule, near) == N // 3
        got = [U.render(c).copy() for c in cams[3:]]
    edited = E.grade_eval(rule, A, near)
    assert not edited.alpha[near].any()
    want = M._fresh_frames(pkg, edited, cams[3:], opts)
    plain = M._fresh_frames(pkg, edited, cams[3:], ((E.OPT_OCCLUSION_CULL, 0), (E.OPT_LAZY_COLOUR, 0), (E.OPT_SORT_CACHE, 0)))
    stale = M._fresh_frames(pkg, A, cams[3:], opts)
    for k in range(len(want)):
        assert np.array_equal(want[k], plain[k]), f"the fresh contexts disagree on frame {k}"
        assert not np.array_equal(want[k], stale[k]), f"the grade does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), f"cull 2: frame {k} differs in {int((got[k] != want[k]).any(axis=2).sum())} pixels"


# ---- 6. a visibility in force ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("volume", "mask"))
def test_grade_under_a_visibility(pkg, kind):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, [1, 2])
    rule = GC.make_rule(pkg, "alpha_half")
    sel = GC.masks(pkg)["every_third"]
    if kind == "volume":
        volumes = [E.crop_box((-1.0, 0.0, 0.0), (1.0, 4.0, 4.0))]       # the half of the cloud with x < 0 stays visible
        vis = dict(volumes=volumes)
        hidden = ~E.visibility_eval(E.visibility_struct(volumes)[0], A.P).astype(bool)
    else:
        hidden = np.arange(N) % 2 == 1
        vis = dict(mask=hidden)
    assert 0.3 <= hidden.mean() <= 0.7 and (hidden & sel).any() and (~hidden & sel).any()
    want = E.grade_eval(rule, A, sel)
    with pkg.Engine(0) as U, pkg.Engine(0) as F:
        U.upload(A)
        U.set_visibility(**vis)
        assert U.get_visibility()[1] == int(hidden.sum())
        U.render(cams[0])
        assert U.grade(rule, sel) == _popcount(sel)
        F.upload(want)
        F.set_visibility(**vis)
        assert U.get_visibility()[1] == F.get_visibility()[1] == int(hidden.sum())
        got = M._planes(U)
        M._assert_same_planes(got, M._planes(F), f"a visibility ({kind}) in force: the resident opacities")
        order = got["order"].view(np.int32)
        resident_alpha = got["geoA"].view(np.uint32).reshape(-1, 4)[:, 3]
        assert not resident_alpha[hidden[order]].any(), "a hidden splat's resident alpha is not +0.0f"
        for c in cams:
            assert np.array_equal(U.render(c), F.render(c))
        assert np.array_equal(U.read(names=("alpha",)).alpha.view(np.uint32), want.alpha.view(np.uint32)), "the graded TRUE alphas"
        assert not np.array_equal(want.alpha[hidden], A.alpha[hidden]), "no hidden splat was graded: the case tests nothing"
        U.set_visibility()
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, want), f"the visibility ({kind}) lifted after a grade")


# ---- 7. chains ---------------------------------------------------------------------------------------------------------------
def _assert_same_splats(got, want, label):
    for k in ("P", "Cd", "alpha", "scale", "orient"):
        assert np.array_equal(getattr(got, k).view(np.uint8), getattr(want, k).view(np.uint8)), (label, k)
    for k in ("shx", "shy", "shz"):
        assert np.array_equal(getattr(got, k)[:, :15], getattr(want, k)[:, :15]), (label, k)


@pytest.mark.gpu
def test_select_then_grade_then_read(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [1])[0]
    rule = GC.make_rule(pkg, "all")
    hb = HipBuffers()
    try:
        dev = hb.upload(np.zeros((N + 31) // 32, np.uint32))
        with pkg.Engine(0) as U:
            U.upload(A)
            n_hit, n_set = U.select_device(cam, E.select_region(rect=(0.0, 0.0, W / 2.0, float(H))), dev)
            sel = E.unpack_mask(hb.download(dev, ((N + 31) // 32,), np.uint32), N)
            assert 10 < n_hit == n_set == int(sel.sum()) < N - 10
            assert U.grade_device(rule, dev) == n_hit
            got = U.read()
    finally:
        hb.free()
    _assert_same_splats(got, E.grade_eval(rule, A, sel), "select, grade, read")


@pytest.mark.gpu
def test_grade_remove_add_grade(pkg):
    E = pkg.engine
    A, B = M._cloud(pkg, 11), M._cloud(pkg, 12, n=90)
    r1, r2 = GC.make_rule(pkg, "all"), GC.make_rule(pkg, "grey")
    m1 = GC.masks(pkg)["every_third"]
    gone = np.arange(N) % 4 == 1
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.grade(r1, m1) == _popcount(m1)
        s = E.grade_eval(r1, A, m1)
        assert U.remove(gone) == N - int(gone.sum())
        s = s.subset(~gone)
        assert U.add(B) == s.n + B.n
        s = s.concat(B)
        m2 = np.arange(s.n) >= s.n - 120                                # the new splats and some old ones
        assert U.grade(r2, m2) == 120
        s = E.grade_eval(r2, s, m2)
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, s), "grade, remove, add, grade")


@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_update_cd_then_grade(pkg, sh):
    E = pkg.engine
    A, B = M._cloud(pkg, 11, sh=sh), M._cloud(pkg, 12, sh=sh)
    rule = GC.make_rule(pkg, "contrast")
    mask = GC.masks(pkg)["range_50_200"]
    s = M._copy(pkg, A)
    s.Cd[100:260] = B.Cd[100:260]
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.update_attrs(100, Cd=s.Cd[100:260]) == 160
        assert U.grade(rule, mask) == 150
        got = M._planes(U, sh)
    M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(rule, s, mask), sh=sh), "update_attrs of Cd, then a grade")


@pytest.mark.gpu
def test_two_grades_in_a_row(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    r1, r2 = GC.make_rule(pkg, "all"), GC.make_rule(pkg, "alpha_lift")
    m1, m2 = GC.masks(pkg)["range_50_200"], GC.masks(pkg)["every_third"]
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.grade(r1, m1) == 150 and U.grade(r2, m2) == _popcount(m2)
        gr = U.get_grade()
        assert gr["grades"] == 2 and gr["graded_last"] == _popcount(m2) and gr["ms"][1] > 0.0 and gr["ms"][3] >= gr["ms"][1]
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, E.grade_eval(r2, E.grade_eval(r1, A, m1), m2)), "eval o eval")


# ---- 8. several ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_grade_matches_single_context(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, range(4))
    rule = E.grade_prepare(E.grade_params(**FRAME_RULES["colour+alpha"]))
    mask = GC.masks(pkg)["every_third"]
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(A)
        for c in cams[:2]:
            Mu.render(c)
        assert Mu.grade(rule, mask) == _popcount(mask)
        got = [Mu.render(c).copy() for c in cams[2:]]
        st = [Mu.stats(r) for r in range(2)]
        assert [s["uploads"] for s in st] == [1, 1] and [s["moves"] for s in st] == [0, 0]
        _assert_same_splats(Mu.read(), E.grade_eval(rule, A, mask), "rank 0's replica")
    want = M._fresh_frames(pkg, E.grade_eval(rule, A, mask), cams[2:])
    stale = M._fresh_frames(pkg, A, cams[2:])
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k])
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"


# ---- 9. refusals with a live context -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_alone(pkg):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    L = pkg.load_library()
    cam = M._cams(pkg, [2])[0]
    good = E._grade_rule_struct(GC.make_rule(pkg, "all"))
    words = E.pack_mask(GC.masks(pkg)["every_third"])
    graded = C.c_int64(-7)
    with pkg.Engine(0) as U:
        assert L.gsr_grade(U.h, words.ctypes.data, 0, C.byref(good), C.byref(graded)) == GSR_E_INVALID       # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes, frame = M._planes(U), U.render(cam).copy()
        nan = E._grade_rule_struct(GC.make_rule(pkg, "all"))
        nan.M[5] = np.nan
        inf = E._grade_rule_struct(GC.make_rule(pkg, "all"))
        inf.ab = np.inf
        flag = E._grade_rule_struct(GC.make_rule(pkg, "all"))
        flag.flags = 7
        cases = {
            "NULL ctx": lambda: L.gsr_grade(None, words.ctypes.data, 0, C.byref(good), C.byref(graded)),
            "NULL rule": lambda: L.gsr_grade(U.h, words.ctypes.data, 0, None, C.byref(graded)),
            "a NaN in the rule": lambda: L.gsr_grade(U.h, words.ctypes.data, 0, C.byref(nan), C.byref(graded)),
            "an infinite alpha offset": lambda: L.gsr_grade(U.h, None, 0, C.byref(inf), C.byref(graded)),
            "an unknown flag": lambda: L.gsr_grade(U.h, None, 0, C.byref(flag), C.byref(graded)),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            assert graded.value == -7, label
            M._assert_same_planes(M._planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        assert U.get_grade()["grades"] == 0                                                                 # only the calls that passed count
        assert L.gsr_grade(U.h, words.ctypes.data, 0, C.byref(good), None) == 0                             # n_graded may be NULL
        assert U.get_grade()["grades"] == 1
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert L.gsr_grade(U.h, words.ctypes.data, 0, C.byref(good), C.byref(graded)) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "uploaded again after the refused grade")
        assert np.array_equal(U.render(cam), frame)
        assert U.get_grade()["grades"] == 1
