"""Adding on the GPU (gsr_add): splats appended to the resident cloud, ordered and packed on the device, no re-upload.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of cloud A, then the edits --
and a fresh context F that was uploaded the concatenation (the resident arrays as edited so far, then the new rows) with the same
options: the resident planes (gsr_debug_read_resident) and the storage order (gsr_debug_read_storage_order) are the same bytes, and so
is every later frame, whatever the frame's regime.

The cloud, the comparators and the frame modes are test_move_gpu's: 357 splats = five full clusters of 64 and one of 37; frames of
96 x 64 pixels on the parity tests' orbit.  The added clouds were chosen on the CPU with the oracle's Morton rule; every test asserts
the property it relies on from F's storage order, so a case that stops testing anything fails loudly."""
import ctypes as C

import numpy as np
import pytest

import test_device_source_gpu as D
import test_move_gpu as M
from helpers import HipBuffers

N, W, H = M.N, M.W, M.H
GSR_E_INVALID = -1


def _new(pkg, seed, m, sh=True, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """the first m splats of the cloud of another seed, their positions scaled and shifted"""
    B = M._copy(pkg, M._cloud(pkg, seed, sh=sh).subset(slice(0, m)))
    B.P[:] = (B.P * np.float32(scale) + np.asarray(shift, np.float32)).astype(np.float32)
    return B


# label -> (seed, m, scale, shift, the properties F's storage order must show)
CASES = {
    "m = 1": (12, 1, 1.0, (0, 0, 0), ("inside", "old order kept")),
    "m = 27": (12, 27, 1.0, (0, 0, 0), ("inside", "old order kept", "six clusters, all mixed")),
    "m = 28": (12, 28, 1.0, (0, 0, 0), ("inside", "old order kept", "a seventh cluster")),
    "m = 64": (12, 64, 1.0, (0, 0, 0), ("box widens", "old order changes")),
    "m = 357": (12, 357, 1.0, (0, 0, 0), ("box widens", "old order changes")),
    "m = 91, x 1.5": (13, 91, 1.5, (0, 0, 0), ("box widens",)),
    "m = 130, + z 3": (15, 130, 1.0, (0, 0, 3), ("box widens", "old, mixed and new clusters")),
}


def _kinds(order, n_old):
    """per cluster of the storage order: 'old', 'new' or 'mixed'"""
    out = []
    for c in range(0, order.size, 64):
        old = order[c:c + 64] < n_old
        out.append("old" if old.all() else ("mixed" if old.any() else "new"))
    return out


def _check_properties(label, props, A, B, order_a, order_f):
    lo, hi = A.P.min(axis=0), A.P.max(axis=0)
    inside = bool(((B.P >= lo) & (B.P <= hi)).all())
    kept = np.array_equal(order_f[order_f < A.n], order_a)
    kinds = _kinds(order_f, A.n)
    for p in props:
        ok = {"inside": inside, "box widens": not inside, "old order kept": kept, "old order changes": not kept,
              "six clusters, all mixed": kinds == ["mixed"] * 6, "a seventh cluster": len(kinds) == 7,
              "old, mixed and new clusters": kinds == ["old"] * 5 + ["mixed", "new", "new"]}[p]
        assert ok, f"{label}: the case no longer has the property '{p}' (clusters: {kinds})"


def _move_and_update(pkg, U, s, seed):
    """a move of the whole cloud and an update of a range that spans clusters -> the edited cloud"""
    n = s.n
    src = M._cloud(pkg, seed, sh=s.has_sh, n=n)
    assert U.move(0, src.P) == n
    first, cnt = n // 7, n // 2
    rows = {k: np.ascontiguousarray(getattr(src, k)[first:first + cnt]) for k in ("Cd", "alpha", "scale")}
    assert U.update_attrs(first, **rows) == cnt
    out = M._copy(pkg, s)
    out.P[:] = src.P
    for k, v in rows.items():
        getattr(out, k)[first:first + cnt] = v
    return out


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_resident_bits(pkg, sh, order):
    A = M._cloud(pkg, 11, sh=sh)
    E = pkg.engine
    for label, (seed, m, scale, shift, props) in CASES.items():
        B = _new(pkg, seed, m, sh, scale, shift)
        S = A.concat(B)
        label = f"{label} order {order} sh {sh}"
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = M._planes(U, sh)
            assert U.add(B) == N + m, label
            got = M._planes(U, sh)
            st, ad = U.stats(), U.get_add()
            assert st["n_splats"] == N + m and st["uploads"] == 1 and st["moves"] == 0, label    # an add is neither
            assert ad["adds"] == 1 and ad["added_last"] == m and ad["grows"] == 1, (label, ad)
            assert ad["capacity"] == E.add_capacity(N, N + m) == N + m + (N + m) // 4, (label, ad)
            assert ad["ms"][0] > 0.0 and ad["ms"][3] >= ad["ms"][0], (label, ad)
            assert U.debug_resident(E.RESIDENT_COL).size == (6 if sh else 1) * ad["capacity"] * 16      # the new chunk stride
        want = M._fresh_planes(pkg, S, order, sh)
        M._assert_same_planes(got, want, label)
        assert got["geoA"].size == (N + m) * 16 > before["geoA"].size
        order_a, order_f = before["order"].view(np.int32), want["order"].view(np.int32)
        if order == 0:
            assert np.array_equal(order_f, np.arange(N + m, dtype=np.int32))
        else:
            _check_properties(label, props, A, B, order_a, order_f)
            tail = np.concatenate([order_a, np.arange(N, N + m, dtype=np.int32)])
            assert not np.array_equal(order_f, tail), f"{label}: the new order is the old one with the new splats at the tail"


# ---- 2. the capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_several_small_adds_grow_now_and_then(pkg, order):
    """seven adds of 5 %: the capacity follows add_capacity step by step and grows twice; after every add a move of the whole cloud
    and an update still match a fresh upload (stale spare planes or cluster arrays of the old size would not)"""
    E = pkg.engine
    s = M._cloud(pkg, 11)
    B = M._cloud(pkg, 12)
    step = 18
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_STORAGE_ORDER, order)
        U.upload(s)
        cap, grows = N, 0
        for k in range(7):
            rows = B.subset(slice(k * step, (k + 1) * step))
            s = s.concat(rows)
            assert U.add(rows) == s.n
            new = E.add_capacity(cap, s.n)
            grows += new != cap
            cap = new
            ad = U.get_add()
            assert ad["adds"] == k + 1 and ad["added_last"] == step and ad["capacity"] == cap and ad["grows"] == grows, (k, ad, cap, grows)
            M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s, order), f"add {k}, order {order}")
            s = _move_and_update(pkg, U, s, 30 + k)
            M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s, order), f"move and update after add {k}, order {order}")
        assert grows == 2 and U.get_add()["grows"] == 2 < U.get_add()["adds"] == 7
        assert U.stats()["uploads"] == 1 and U.stats()["moves"] == 7


@pytest.mark.gpu
def test_an_add_that_fits_after_a_removal(pkg):
    A = M._cloud(pkg, 11)
    gone = np.zeros(N, bool)
    gone[np.random.default_rng(3).permutation(N)[:100]] = True
    B = _new(pkg, 12, 50)
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.remove(gone) == N - 100
        s = A.subset(~gone).concat(B)
        assert U.add(B) == N - 50
        ad = U.get_add()
        assert ad["grows"] == 0 and ad["capacity"] == N and ad["adds"] == 1, ad
        M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s), "an add that fits")
        s = _move_and_update(pkg, U, s, 41)
        M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s), "move and update after an add that fits")
        assert U.get_add()["capacity"] == N


# ---- 3. a sequence of edits --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sequence_of_edits(pkg):
    """upload -> remove -> add (fits) -> move -> update -> add (grows) -> remove: planes and frames are a fresh upload's"""
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, range(4))
    rng = np.random.default_rng(8)
    gone = rng.random(N) < 0.3
    with pkg.Engine(0) as U:
        U.upload(A)
        U.render(cams[0])
        assert U.remove(gone) == int((~gone).sum())
        s = A.subset(~gone)
        B1 = _new(pkg, 12, 60)
        s = s.concat(B1)
        assert s.n <= N and U.add(B1) == s.n
        assert U.get_add()["grows"] == 0
        U.render(cams[1])
        s = _move_and_update(pkg, U, s, 51)
        B2 = _new(pkg, 13, 200, scale=1.5)
        s = s.concat(B2)
        assert s.n > N and U.add(B2) == s.n
        assert U.get_add()["grows"] == 1 and U.get_add()["adds"] == 2
        gone2 = rng.random(s.n) < 0.25
        assert gone2[-200:].any() and gone2[:-200].any()
        assert U.remove(gone2) == int((~gone2).sum())
        s = s.subset(~gone2)
        got = M._planes(U)
        frames = [U.render(c).copy() for c in cams[2:]]
        assert U.stats()["uploads"] == 1 and U.stats()["moves"] == 1 and U.stats()["n_splats"] == s.n
    M._assert_same_planes(got, M._fresh_planes(pkg, s), "the sequence")
    want = M._fresh_frames(pkg, s, cams[2:])
    for k in range(len(want)):
        assert (want[k][..., 3] > 0).sum() > 100
        assert np.array_equal(frames[k], want[k]), f"frame {k} after the sequence"


# ---- 4. nothing added, and the empty cloud -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_added_changes_and_invalidates_nothing(pkg):
    A = M._cloud(pkg, 11)
    L = pkg.load_library()
    cam = M._cams(pkg, [1])[0]
    with pkg.Engine(0) as U:
        U.upload(A)
        planes = M._planes(U)
        a = U.render(cam).copy()
        U.render(cam)
        assert U.stats()["sorts_skipped"] == 1
        assert U.add(A.subset(slice(0, 0))) == N
        total = C.c_int64(-1)
        assert L.gsr_add(U.h, 0, *([None] * 8), C.byref(total)) == 0 and total.value == N       # no array is looked at
        assert L.gsr_add_device(U.h, 0, None, C.byref(total)) == 0 and total.value == N
        M._assert_same_planes(M._planes(U), planes, "nothing added")
        assert np.array_equal(U.render(cam), a)
        assert U.stats()["sorts_skipped"] == 2, "the cached order did not survive an add of nothing"
        ad = U.get_add()
        assert ad["adds"] == 0 and ad["added_last"] == 0 and ad["grows"] == 0 and ad["capacity"] == N
        assert U.stats()["n_splats"] == N and U.stats()["uploads"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("everything removed", "upload of 0 splats"))
def test_adding_to_the_empty_cloud(pkg, how):
    sh = how == "everything removed"
    A, B = M._cloud(pkg, 11, sh=sh), _new(pkg, 12, 100, sh)
    cam = M._cams(pkg, [2])[0]
    with pkg.Engine(0) as U:
        if sh:
            U.upload(A)
            U.render(cam)
            assert U.remove(np.ones(N, bool)) == 0
        else:
            U.upload(A.subset(slice(0, 0)))
        assert U.stats()["n_splats"] == 0
        assert U.add(B) == 100
        ad = U.get_add()
        assert ad["adds"] == 1 and ad["grows"] == (0 if sh else 1) and ad["capacity"] == (N if sh else pkg.engine.add_capacity(1, 100)), ad
        got, frame = M._planes(U, sh), U.render(cam).copy()
    M._assert_same_planes(got, M._fresh_planes(pkg, B, 1, sh), how)
    assert np.array_equal(frame, M._fresh_frames(pkg, B, [cam])[0])


# ---- 5. with a visibility in force -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("grow", (True, False))
@pytest.mark.parametrize("what", ("volumes", "volumes + mask", "alpha edited while hidden"))
def test_add_under_a_visibility(pkg, what, grow):
    A, B, Cc = M._cloud(pkg, 11), _new(pkg, 12, 91), M._cloud(pkg, 13)
    E = pkg.engine
    cams = M._cams(pkg, [1, 2])
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = None if what == "volumes" else np.arange(N) % 3 == 0
    hide_ext = None if hide is None else np.concatenate([hide, np.zeros(B.n, bool)])
    s = M._copy(pkg, A)
    first, cnt = 100, 60
    va, keep_a = E.visibility_struct(volumes, hide)
    visible_a = E.visibility_eval(va, A.P)
    if what == "alpha edited while hidden":
        assert (~visible_a[first:first + cnt]).any() and visible_a[first:first + cnt].any()
        s.alpha[first:first + cnt] = Cc.alpha[first:first + cnt]
    S = s.concat(B)
    v, keep = E.visibility_struct(volumes, hide_ext)
    visible = E.visibility_eval(v, S.P)
    assert (~visible[N:]).any() and visible[N:].any(), "the volumes hide none or all of the new splats: the case tests nothing"
    with pkg.Engine(0) as U, pkg.Engine(0) as F:
        if not grow:
            U.upload(M._cloud(pkg, 21, n=500))                         # capacity 500: the add fits
        U.upload(A)
        U.set_visibility(volumes=volumes, mask=hide)
        assert U.get_visibility()[1] == int((~visible_a).sum())
        if what == "alpha edited while hidden":
            assert U.update_attrs(first, alpha=s.alpha[first:first + cnt]) == cnt
        U.render(cams[0])
        assert U.add(B) == S.n
        assert U.get_add()["grows"] == int(grow)
        F.upload(S)
        F.set_visibility(volumes=volumes, mask=hide_ext)
        assert U.get_visibility()[1] == F.get_visibility()[1] == int((~visible).sum())
        assert U.get_visibility()[0].mask_splats == (0 if hide is None else S.n)
        assert U.get_visibility()[0].n_volumes == 1
        M._assert_same_planes(M._planes(U), M._planes(F), f"{what}, then an add (grow {grow})")
        for c in cams:
            assert np.array_equal(U.render(c), F.render(c))
        U.set_visibility()                                              # everything visible again: the TRUE alphas were carried
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, S), f"{what}: the visibility cleared after an add (grow {grow})")


# ---- 6. frames afterwards ----------------------------------------------------------------------------------------------------
def _modes(pkg):
    modes = dict(M._frame_modes(pkg))
    modes["row band"] = ((), None, lambda eng: eng.set_row_band(1, 2))
    return modes


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cull 0", "cull 2", "cull 3", "lazy 0", "lazy 2", "sort cache 2", "depth-tested", "rgba16f",
                                  "shard 1/2 interleaved", "shard 1/2 bands", "row band"])
def test_frames_after_an_add(pkg, mode):
    """two frames leave horizons, hints, cached orders and policies behind; then the cloud doubles, and every later frame is that of
    a fresh upload of the concatenation"""
    A, B = M._cloud(pkg, 11), _new(pkg, 12, N)
    S = A.concat(B)
    opts, render, prepare = _modes(pkg)[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = M._cams(pkg, range(6))
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:2]:
            draw(U, c)
        assert U.add(B) == S.n
        got = [draw(U, c).copy() for c in cams[2:]]
    want = M._fresh_frames(pkg, S, cams[2:], opts, render=render, prepare=prepare)
    stale = M._fresh_frames(pkg, A, cams[2:], opts, render=render, prepare=prepare)
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the add does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode}: frame {k} after the add differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", (0, 1))
def test_frames_after_an_add_two_in_flight_device_target(pkg, deferred):
    """frames are in flight when the add is called: those queued before it are not disturbed, those after it show the larger cloud"""
    A, B = M._cloud(pkg, 11), _new(pkg, 12, N)
    S = A.concat(B)
    E = pkg.engine
    cams = M._cams(pkg, range(8))
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
            U.set_option(E.OPT_DEFERRED_CHECK, deferred)
            U.upload(A)
            outs = [hb.alloc(W * H * 16) for _ in cams]
            for c, o in zip(cams[:3], outs[:3]):
                U.render_to_device(c, o)
            assert U.add(B) == S.n                                      # (no synchronisation by the caller)
            for c, o in zip(cams[3:], outs[3:]):
                U.render_to_device(c, o)
            U.synchronize()
            got = [hb.download(o, (H, W, 4)) for o in outs]
        before = M._fresh_frames(pkg, A, cams[:3])
        for k in range(3):
            assert np.array_equal(got[k], before[k]), f"frame {k}, queued before the add, was disturbed by it"
        want = M._fresh_frames(pkg, S, cams[3:])
        stale = M._fresh_frames(pkg, A, cams[3:])
        for k in range(len(want)):
            assert not np.array_equal(want[k], stale[k])
            assert np.array_equal(got[3 + k], want[k]), f"frame {k} after the add, deferred check {deferred}"
    finally:
        hb.free()


# ---- 7. the device form --------------------------------------------------------------------------------------------------------
def _twin(pkg, f, sh=True):
    """the float rows quantised on the host: what the device form must leave"""
    h = D._halves(pkg, {k: v for k, v in f.items() if sh or k != "sh"})
    return pkg.scenes.Splats(h["P"], h["Cd"], h["alpha"], h["scale"], h["orient"], h.get("shx"), h.get("shy"), h.get("shz"))


@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_device_form_matches_the_host_form(pkg, sh):
    A = M._cloud(pkg, 11, sh=sh)
    m = 91
    f = D._floats(22, n=m)
    for k in ("Cd", "scale", "orient", "sh"):
        D._rounds(pkg, f[k])
    B = _twin(pkg, f, sh)
    hb = HipBuffers()
    try:
        ptrs = {k: hb.upload(v) for k, v in f.items() if sh or k != "sh"}
        with pkg.Engine(0) as U:
            U.upload(A)
            assert U.add_device(ptrs, n=m, sh_vec3_per_point=15 if sh else None) == N + m
            ad = U.get_add()
            assert ad["adds"] == 1 and ad["added_last"] == m and ad["ms"][0] == 0.0, ad       # nothing crossed the link
            got = M._planes(U, sh)
            # the NULL defaults: alpha 1, and a second add without Cd, scale and orient
            assert U.add_device({"P": ptrs["P"], **({"sh": ptrs["sh"]} if sh else {})}, n=m, sh_vec3_per_point=15 if sh else None) == N + 2 * m
            got2 = M._planes(U, sh)
        with pkg.Engine(0) as V:
            V.upload(A)
            assert V.add(B) == N + m
            M._assert_same_planes(got, M._planes(V, sh), "device form vs host form")
        M._assert_same_planes(got, M._fresh_planes(pkg, A.concat(B), 1, sh), "device form")
        q = pkg.engine.quantize_half
        ident = np.tile(np.asarray((0, 0, 0, 1), np.float32), (m, 1))
        B2 = pkg.scenes.Splats(B.P, q(np.zeros((m, 3), np.float32)), np.ones(m, np.float32), q(np.ones((m, 3), np.float32)), q(ident),
                               B.shx, B.shy, B.shz)
        M._assert_same_planes(got2, M._fresh_planes(pkg, A.concat(B).concat(B2), 1, sh), "device form, NULL defaults")
    finally:
        hb.free()


@pytest.mark.gpu
def test_device_form_refuses_a_bad_source(pkg):
    A = M._cloud(pkg, 11)
    E, L = pkg.engine, pkg.load_library()
    m = 91
    f = D._floats(22, n=m)
    total = C.c_int64(-7)
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.alloc(size)
        ptrs = {k: hb.upload(v) for k, v in f.items()}
        host_P = np.ascontiguousarray(f["P"])
        with pkg.Engine(0) as U:
            U.upload(A)
            cam = M._cams(pkg, [1])[0]
            frame = U.render(cam).copy()
            U.render(cam)
            skipped = U.stats()["sorts_skipped"]
            planes = M._planes(U)
            short = room + size - (m * 12 - 4)                          # one word short of the end of its allocation
            bad = {"pageable P": ("P", host_P.ctypes.data, m * 12), "P one word short": ("P", short, m * 12),
                   "misaligned alpha": ("alpha", ptrs["alpha"] + 2, m * 4 - 4), "Cd one word short": ("Cd", short, m * 12)}
            for label, (name, ptr, nbytes) in bad.items():
                # (the pure query first: no verb is handed a pointer it would take)
                assert not U.check_device_source(ptr, nbytes), label
                a, n, keep = E.device_attrs_struct(m, 15, **{**ptrs, name: ptr})
                assert L.gsr_add_device(U.h, m, C.byref(a), C.byref(total)) == GSR_E_INVALID, label
                assert b"gsr_add_device" in L.gsr_last_error(), label
                assert total.value == -7, label
            for label, kw, vpp in (("no P", {k: v for k, v in ptrs.items() if k != "P"}, 15), ("no sh for a cloud with SH", {"P": ptrs["P"]}, None),
                                   ("sh_vec3_per_point 17", ptrs, 17), ("sh_vec3_per_point 0", ptrs, 0)):
                a, n, keep = E.device_attrs_struct(m, vpp, **kw)
                assert L.gsr_add_device(U.h, m, C.byref(a), C.byref(total)) == GSR_E_INVALID, label
            assert L.gsr_add_device(U.h, m, None, C.byref(total)) == GSR_E_INVALID
            M._assert_same_planes(M._planes(U), planes, "refused device sources")
            assert np.array_equal(U.render(cam), frame)
            assert U.stats()["sorts_skipped"] == skipped + 1, "a refused add invalidated the cached order"
            assert U.get_add()["adds"] == 0 and U.stats()["n_splats"] == N
        with pkg.Engine(0) as V:                                        # sh for a cloud without SH
            V.upload(M._cloud(pkg, 11, sh=False))
            a, n, keep = E.device_attrs_struct(m, 15, **ptrs)
            assert L.gsr_add_device(V.h, m, C.byref(a), C.byref(total)) == GSR_E_INVALID
            assert V.stats()["n_splats"] == N
    finally:
        hb.free()


# ---- 8. refusals leave the context alone -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_alone(pkg):
    A, B = M._cloud(pkg, 11), _new(pkg, 12, 50)
    E, L = pkg.engine, pkg.load_library()
    cam = M._cams(pkg, [2])[0]
    arr = E.add_arrays(B)
    p = arr.ptrs()
    total = C.c_int64(-7)

    def call(h, m, ptrs):
        return L.gsr_add(h, m, *ptrs, C.byref(total))

    def without(*idx):
        return [None if k in idx else v for k, v in enumerate(p)]

    with pkg.Engine(0) as U:
        assert call(U.h, 50, p) == GSR_E_INVALID                        # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        frame = U.render(cam).copy()
        U.render(cam)
        planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
        cases = {
            "NULL ctx": lambda: call(None, 50, p),
            "m < 0": lambda: call(U.h, -1, p),
            "n + m > 0x7fffffff": lambda: call(U.h, 0x7fffffff - N + 1, p),
            "NULL P": lambda: call(U.h, 50, without(0)), "NULL Cd": lambda: call(U.h, 50, without(1)),
            "NULL alpha": lambda: call(U.h, 50, without(2)), "NULL scale": lambda: call(U.h, 50, without(3)),
            "NULL orient": lambda: call(U.h, 50, without(4)),
            "no SH arrays for a cloud with SH": lambda: call(U.h, 50, without(5, 6, 7)),
            "one SH array missing": lambda: call(U.h, 50, without(6)),
            "two SH arrays missing": lambda: call(U.h, 50, without(5, 7)),
        }
        for n_case, (label, fn) in enumerate(cases.items()):
            assert fn() == GSR_E_INVALID, label
            assert total.value == -7, label
            M._assert_same_planes(M._planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
            assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
        assert U.get_add()["adds"] == 0 and U.stats()["n_splats"] == N
        assert L.gsr_add(U.h, 50, *p, None) == 0                        # n_total may be NULL
        assert U.stats()["n_splats"] == N + 50
        assert L.gsr_get_add(U.h, None, None, None, None, None) == 0    # ... and so may every pointer of gsr_get_add
        M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, A.concat(B)), "added after the refusals")
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert call(U.h, 50, p) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "uploaded again after the refused add")
        assert np.array_equal(U.render(cam), frame)
    with pkg.Engine(0) as V:                                            # SH arrays for a cloud uploaded without SH
        V.upload(M._cloud(pkg, 11, sh=False))
        planes = M._planes(V, sh=False)
        assert call(V.h, 50, p) == GSR_E_INVALID
        M._assert_same_planes(M._planes(V, sh=False), planes, "SH arrays without SH")
        assert V.stats()["n_splats"] == N


# ---- 9. several ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_add_matches_single_context(pkg):
    A, B = M._cloud(pkg, 11), _new(pkg, 12, N)
    S = A.concat(B)
    E = pkg.engine
    cams = M._cams(pkg, range(4))
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(A)
        for c in cams[:2]:
            Mu.render(c)
        assert Mu.add(B) == S.n
        got = [Mu.render(c).copy() for c in cams[2:]]
        st = [Mu.stats(r) for r in range(2)]
        assert [s["n_splats"] for s in st] == [S.n, S.n]
        assert [s["uploads"] for s in st] == [1, 1] and [s["moves"] for s in st] == [0, 0]
    want = M._fresh_frames(pkg, S, cams[2:])
    stale = M._fresh_frames(pkg, A, cams[2:])
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k])
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"
