"""Removal on the GPU (gsr_remove): resident splats deleted, compacted and re-ordered on the device, no re-upload.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of cloud A, then the removal(s)
-- and a fresh context F that was uploaded the survivors' arrays in their relative upload order with the same options: the resident
planes (gsr_debug_read_resident) and the storage order (gsr_debug_read_storage_order) are the same bytes, and so is every later frame,
whatever the frame's regime.

The cloud, the comparators and the frame modes are test_move_gpu's: 357 splats = five full clusters of 64 and one of 37; frames of
96 x 64 pixels on the parity tests' orbit.  The shape with more than one workgroup comes from the exported GSR_REMOVE_BLOCK."""
import ctypes as C

import numpy as np
import pytest

import test_move_gpu as M
from helpers import HipBuffers

N, W, H = M.N, M.W, M.H
GSR_E_INVALID = -1


def _rand(seed, frac, n=N):
    return np.random.default_rng(seed).random(n) < frac


def _exactly(seed, gone_count, n=N):
    """a mask that removes exactly gone_count splats"""
    gone = np.zeros(n, bool)
    gone[np.random.default_rng(seed).permutation(n)[:gone_count]] = True
    return gone


def _span(lo, hi, n=N):
    gone = np.zeros(n, bool)
    gone[lo:hi] = True
    return gone


def _masks():
    """label -> (boolean mask, True = goes; garbage: set the bits behind n in the last word)"""
    all_but_one = np.ones(N, bool)
    all_but_one[200] = False
    return {
        "first": (_span(0, 1), False), "last": (_span(N - 1, N), False), "171": (_span(171, 172), False),
        "[64, 128)": (_span(64, 128), False), "[50, 200)": (_span(50, 200), False),
        "every other": (np.arange(N) % 2 == 1, False), "random 40 %": (_rand(5, 0.4), False), "all but one": (all_but_one, False),
        "320 left": (_exactly(8, N - 320), False), "321 left": (_exactly(9, N - 321), False),
        "garbage behind n": (_rand(6, 0.3), True),
    }


def _words(pkg, gone, garbage=False):
    words = pkg.engine.pack_mask(gone)
    if garbage:
        assert gone.size % 32
        words[-1] |= np.uint32((0xffffffff << (gone.size % 32)) & 0xffffffff)
    return words


def _remove(eng, s, gone, words=None):
    """remove from the engine (None: nowhere) and return the survivors' arrays in their relative upload order"""
    left = int((~gone).sum())
    if eng is not None:
        assert eng.remove(gone if words is None else words) == left
        assert eng.stats()["n_splats"] == left
    return s.subset(~gone)


def _closed_holes(pkg, order_before, gone):
    """the old storage order with the removed splats taken out and the survivors renumbered: what a removal that did NOT re-order would leave"""
    idx, _ = pkg.engine.remove_map(gone)
    closed = idx[order_before.view(np.int32)]
    return closed[closed >= 0]


# ---- 1. resident bits --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_resident_bits(pkg, sh, order):
    A = M._cloud(pkg, 11, sh=sh)
    E = pkg.engine
    for label, (gone, garbage) in _masks().items():
        label = f"{label} order {order} sh {sh}"
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = M._planes(U, sh)
            left = _remove(U, A, gone, _words(pkg, gone, garbage))
            got = M._planes(U, sh)
            st, rm = U.stats(), U.get_removal()
            assert st["uploads"] == 1 and st["moves"] == 0, label       # a removal is neither
            assert rm["removals"] == 1 and rm["removed_last"] == int(gone.sum()), (label, rm)
            assert rm["ms"][0] > 0.0 and rm["ms"][3] >= rm["ms"][0], (label, rm)
        assert left.n == int((~gone).sum()) and 0 < left.n < N
        M._assert_same_planes(got, M._fresh_planes(pkg, left, order, sh), label)
        assert got["geoA"].size == left.n * 16 < before["geoA"].size
        if not (order == 0 and gone[left.n:].all()):                    # (in upload order a removed tail leaves the head where it was)
            assert not np.array_equal(before["geoA"][:got["geoA"].size], got["geoA"]), "no slot holds another splat: the case tests nothing"
        if order == 0:
            assert np.array_equal(got["order"].view(np.int32), np.arange(left.n, dtype=np.int32))
        elif label.startswith("random 40 %"):
            # (checked on the CPU with the Morton rule for seed 5: the survivors' box differs from the cloud's, so 168 of the 206 slots
            #  hold another splat than closing the holes of the old order would put there)
            assert not np.array_equal(_closed_holes(pkg, before["order"], gone), got["order"].view(np.int32)), \
                "the new order is the old one with its holes closed: the case does not test the re-ordering"


# ---- 2. more than one workgroup of the scan ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_several_blocks_partial_last_block_and_word(pkg):
    block = pkg.engine.REMOVE_BLOCK
    blocks = 3 if 3 * block + 37 <= 50_000 else 2
    n = blocks * block + 37
    assert n % 64 and n % 32 and n % block
    A = M._cloud(pkg, 31, sh=False, n=n)
    gone = _rand(32, 0.5, n)
    per_block = [int((~gone[b * block:(b + 1) * block]).sum()) for b in range(blocks + 1)]
    assert all(per_block) and len(set(per_block[:blocks])) > 1          # every block keeps something, and not the same number
    with pkg.Engine(0) as U:
        U.upload(A)
        left = _remove(U, A, gone)
        got = M._planes(U, sh=False)
    M._assert_same_planes(got, M._fresh_planes(pkg, left, 1, sh=False), f"{n} splats in {blocks + 1} blocks")


# ---- 3. none and all -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_removed_changes_and_invalidates_nothing(pkg):
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [1])[0]
    with pkg.Engine(0) as U:
        U.upload(A)
        planes = M._planes(U)
        a = U.render(cam).copy()
        U.render(cam)
        assert U.stats()["sorts_skipped"] == 1
        assert U.remove(np.zeros(N, bool)) == N
        assert U.remove(None, hidden=True) == N                         # no visibility in force: the flag removes nothing
        garbage = np.zeros((N + 31) // 32, np.uint32)
        garbage[-1] = np.uint32((0xffffffff << (N % 32)) & 0xffffffff)  # only bits behind n
        assert U.remove(garbage) == N
        M._assert_same_planes(M._planes(U), planes, "nothing removed")
        assert np.array_equal(U.render(cam), a)
        assert U.stats()["sorts_skipped"] == 2, "the cached order did not survive a removal of nothing"
        rm = U.get_removal()
        assert rm["removals"] == 0 and rm["removed_last"] == 0
        assert U.stats()["n_splats"] == N and U.stats()["uploads"] == 1


@pytest.mark.gpu
def test_everything_removed_leaves_the_empty_cloud(pkg):
    A = M._cloud(pkg, 11)
    cams = M._cams(pkg, [1, 2])
    with pkg.Engine(0) as F:
        F.upload(A.subset(np.zeros(N, bool)))
        assert F.stats()["n_splats"] == 0
        want = F.render(cams[0]).copy()
    with pkg.Engine(0) as U:
        U.upload(A)
        U.render(cams[0])
        assert U.remove(np.ones(N, bool)) == 0
        assert U.stats()["n_splats"] == 0 and U.get_removal()["removed_last"] == N
        assert np.array_equal(U.render(cams[0]), want)
        assert U.remove(np.zeros(0, bool)) == 0                         # the empty cloud takes a removal of nothing
        with pytest.raises(pkg.engine.GsrError):
            U.remove(np.zeros(1, bool))                                 # a mask of another length never reaches the library
        U.upload(A)
        M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, A), "uploaded again after everything went")
        assert np.array_equal(U.render(cams[1]), M._fresh_frames(pkg, A, cams[1:])[0])


# ---- 4. frames afterwards --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cull 0", "cull 2", "cull 3", "lazy 0", "lazy 2", "sort cache 2", "depth-tested", "rgba16f",
                                  "shard 1/2 interleaved", "shard 1/2 bands"])
def test_frames_after_a_removal(pkg, mode):
    """two frames leave horizons, hints, cached orders and policies behind; then 40 % of the cloud goes, and every later frame is
    that of a fresh upload of the survivors"""
    A = M._cloud(pkg, 11)
    opts, render, prepare = M._frame_modes(pkg)[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = M._cams(pkg, range(8))
    gone = _rand(5, 0.4)
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:2]:
            draw(U, c)
        left = _remove(U, A, gone)
        got = [draw(U, c).copy() for c in cams[2:]]
    want = M._fresh_frames(pkg, left, cams[2:], opts, render=render, prepare=prepare)
    stale = M._fresh_frames(pkg, A, cams[2:], opts, render=render, prepare=prepare)
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the removal does not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode}: frame {k} after the removal differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", (0, 1))
def test_frames_after_a_removal_two_in_flight_device_target(pkg, deferred):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    cams = M._cams(pkg, range(8))
    gone = _rand(5, 0.4)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
            U.set_option(E.OPT_DEFERRED_CHECK, deferred)
            U.upload(A)
            outs = [hb.alloc(W * H * 16) for _ in cams]
            for c, o in zip(cams[:3], outs[:3]):
                U.render_to_device(c, o)
            left = _remove(U, A, gone)                                  # (no synchronisation by the caller)
            for c, o in zip(cams[3:], outs[3:]):
                U.render_to_device(c, o)
            U.synchronize()
            got = [hb.download(o, (H, W, 4)) for o in outs]
        before = M._fresh_frames(pkg, A, cams[:3])
        for k in range(3):
            assert np.array_equal(got[k], before[k]), f"frame {k}, queued before the removal, was disturbed by it"
        want = M._fresh_frames(pkg, left, cams[3:])
        stale = M._fresh_frames(pkg, A, cams[3:])
        for k in range(len(want)):
            assert not np.array_equal(want[k], stale[k])
            assert np.array_equal(got[3 + k], want[k]), f"frame {k} after the removal, deferred check {deferred}"
    finally:
        hb.free()


# ---- 5. composition in the new index space ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_later_edits_count_in_the_new_index_space(pkg):
    A, B = M._cloud(pkg, 11), M._cloud(pkg, 12)
    E = pkg.engine
    cam = M._cams(pkg, [1])[0]
    gone = _rand(5, 0.4)
    n1 = int((~gone).sum())
    first, cnt = 30, 100
    hide = np.arange(n1) % 3 == 0                                       # a visibility mask of n' bits
    with pkg.Engine(0) as U, pkg.Engine(0) as F:
        U.upload(A)
        s = _remove(U, A, gone)
        F.upload(s)
        wire = U.render_wire(cam).copy()                                # (through the inverse of the NEW order)
        assert np.array_equal(wire, F.render_wire(cam)) and (wire[..., 3] > 0).sum() > 100
        rows = {k: np.ascontiguousarray(getattr(B, k)[first:first + cnt]) for k in ("Cd", "alpha", "scale")}
        for eng in (U, F):
            assert eng.update_attrs(first, **rows) == cnt
        M._assert_same_planes(M._planes(U), M._planes(F), "update_attrs after a removal")
        for eng in (U, F):
            assert eng.move(first, B.P[first:first + cnt]) == cnt
        M._assert_same_planes(M._planes(U), M._planes(F), "move after a removal")
        for eng in (U, F):
            eng.set_visibility(volumes=[E.crop_box((0, 0, 0), 0.7)], mask=hide)
        assert U.get_visibility()[1] == F.get_visibility()[1] > int(hide.sum())
        M._assert_same_planes(M._planes(U), M._planes(F), "set_visibility after a removal")
        assert np.array_equal(U.render(cam), F.render(cam))
        for eng in (U, F):
            eng.set_visibility()
        # a second removal on top of the first (the planes swapped once already)
        s = M._copy(pkg, s)
        for k, v in rows.items():
            getattr(s, k)[first:first + cnt] = v
        s.P[first:first + cnt] = B.P[first:first + cnt]
        gone2 = _rand(7, 0.3, n1)
        s2 = _remove(U, s, gone2)
        assert U.get_removal()["removals"] == 2 and U.get_removal()["removed_last"] == int(gone2.sum())
        assert U.stats()["uploads"] == 1 and U.stats()["moves"] == 1
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, s2), "a second removal")


# ---- 6. with a visibility in force -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_removal_under_volumes_and_a_mask(pkg, order):
    A, B = M._cloud(pkg, 11), M._cloud(pkg, 12)
    E = pkg.engine
    cams = M._cams(pkg, [1, 2])
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = np.arange(N) % 3 == 0
    v, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(v, A.P)
    assert 0.05 <= visible.mean() <= 0.95
    gone = _rand(5, 0.4)
    assert (gone & ~visible).any() and (~gone & ~visible).sum() > 10 and (~gone & visible).sum() > 10
    first, cnt = 100, 60                                                # alphas edited while some of the rows are hidden
    assert (~visible[first:first + cnt] & ~gone[first:first + cnt]).any()
    s = M._copy(pkg, A)
    s.alpha[first:first + cnt] = B.alpha[first:first + cnt]
    left = s.subset(~gone)
    with pkg.Engine(0) as U, pkg.Engine(0) as F:
        for eng in (U, F):
            eng.set_option(E.OPT_STORAGE_ORDER, order)
        U.upload(A)
        U.set_visibility(volumes=volumes, mask=hide)
        assert U.update_attrs(first, alpha=s.alpha[first:first + cnt]) == cnt
        U.render(cams[0])
        assert U.remove(gone) == left.n
        F.upload(left)
        F.set_visibility(volumes=volumes, mask=hide[~gone])
        assert U.get_visibility()[1] == F.get_visibility()[1] == int((~visible & ~gone).sum())
        assert U.get_visibility()[0].mask_splats == left.n
        M._assert_same_planes(M._planes(U), M._planes(F), "volumes + mask, then a removal")
        for c in cams:
            assert np.array_equal(U.render(c), F.render(c))
        U.set_visibility()                                              # everything visible again: the TRUE alphas were carried
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, left, order), "the visibility cleared after a removal")


@pytest.mark.gpu
@pytest.mark.parametrize("with_mask", (False, True))
def test_remove_hidden(pkg, with_mask):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    volumes = [E.crop_ellipsoid((0.1, -0.1, 0), (0.9, 0.5, 0.7))]
    hide = np.arange(N) % 5 == 0
    v, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(v, A.P)
    assert 0.05 <= visible.mean() <= 0.95 and (hide & E.visibility_eval(E.visibility_struct(volumes)[0], A.P)).any()
    extra = _rand(9, 0.2) if with_mask else np.zeros(N, bool)
    assert not with_mask or ((extra & visible).any() and (extra & ~visible).any())
    stay = visible & ~extra
    with pkg.Engine(0) as U:
        U.upload(A)
        U.set_visibility(volumes=volumes, mask=hide)
        assert U.get_visibility()[1] == int((~visible).sum())
        assert U.remove(extra if with_mask else None, hidden=True) == int(stay.sum())
        assert U.get_visibility()[1] == 0 and U.get_visibility()[0].n_volumes == 1
        assert U.get_removal()["removed_last"] == int((~stay).sum())
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, A.subset(stay)), f"hidden=True, caller's mask {with_mask}")


@pytest.mark.gpu
def test_remove_hidden_without_a_visibility_removes_nothing_extra(pkg):
    A = M._cloud(pkg, 11)
    gone = _span(50, 200)
    with pkg.Engine(0) as U:
        U.upload(A)
        assert U.remove(None, hidden=True) == N and U.get_removal()["removals"] == 0
        assert U.remove(gone, hidden=True) == N - 150
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, A.subset(~gone)), "hidden=True without a visibility")


# ---- 7. a device mask ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_mask(pkg):
    A = M._cloud(pkg, 11)
    L = pkg.load_library()
    gone = _rand(5, 0.4)
    words = pkg.engine.pack_mask(gone)
    left = C.c_int64(-1)
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.alloc(size)
        dev = hb.upload(words)
        with pkg.Engine(0) as U:
            U.upload(A)
            planes = M._planes(U)
            # refused by the pointer check, before anything is launched (the pure query first: no verb is handed a pointer it would take)
            short = room + size - (words.size - 1) * 4                  # one word short of the end of its allocation
            for label, ptr, nbytes in (("pageable", words.ctypes.data, words.nbytes), ("one word short", short, words.nbytes),
                                       ("misaligned", dev + 2, words.nbytes - 4)):
                assert not U.check_device_source(ptr, nbytes), label
                assert L.gsr_remove(U.h, C.c_void_p(ptr), 1, 0, C.byref(left)) == GSR_E_INVALID, label
                assert b"gsr_remove" in L.gsr_last_error(), label
                M._assert_same_planes(M._planes(U), planes, label)
            assert U.get_removal()["removals"] == 0 and U.stats()["n_splats"] == N
            assert U.remove_device(dev) == int((~gone).sum())
            assert U.get_removal()["ms"][0] == 0.0                      # nothing crossed the link
            got = M._planes(U)
        with pkg.Engine(0) as V:
            V.upload(A)
            assert V.remove(gone) == int((~gone).sum())
            M._assert_same_planes(got, M._planes(V), "device mask vs host mask")
        M._assert_same_planes(got, M._fresh_planes(pkg, A.subset(~gone)), "device mask")
    finally:
        hb.free()


# ---- 8. errors leave the context alone -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_the_context_alone(pkg):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    L = pkg.load_library()
    cam = M._cams(pkg, [2])[0]
    words = E.pack_mask(_rand(5, 0.4))
    left = C.c_int64(-7)
    with pkg.Engine(0) as U:
        assert L.gsr_remove(U.h, words.ctypes.data, 0, 0, C.byref(left)) == GSR_E_INVALID       # before any upload
        assert b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes, frame = M._planes(U), U.render(cam).copy()
        cases = {
            "NULL ctx": lambda: L.gsr_remove(None, words.ctypes.data, 0, 0, C.byref(left)),
            "NULL mask without the flag": lambda: L.gsr_remove(U.h, None, 0, 0, C.byref(left)),
            "NULL device mask without the flag": lambda: L.gsr_remove(U.h, None, 1, 0, C.byref(left)),
            "unknown flag bits": lambda: L.gsr_remove(U.h, words.ctypes.data, 0, 2, C.byref(left)),
            "unknown flag bits beside the known one": lambda: L.gsr_remove(U.h, words.ctypes.data, 0, 1 | 4, C.byref(left)),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            assert left.value == -7, label
            M._assert_same_planes(M._planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        assert U.get_removal()["removals"] == 0
        assert L.gsr_remove(U.h, words.ctypes.data, 0, 0, None) == 0                             # n_left may be NULL
        assert U.stats()["n_splats"] == int((~_rand(5, 0.4)).sum())
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert L.gsr_remove(U.h, words.ctypes.data, 0, 0, C.byref(left)) == GSR_E_INVALID
        assert b"upload in progress" in L.gsr_last_error()
        assert L.gsr_upload_abort(U.h) == 0
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "uploaded again after the refused removal")
        assert np.array_equal(U.render(cam), frame)


# ---- 9. several ranks --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_remove_matches_single_context(pkg):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    cams = M._cams(pkg, range(4))
    gone = _rand(5, 0.4)
    left = A.subset(~gone)
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(A)
        for c in cams[:2]:
            Mu.render(c)
        assert Mu.remove(gone) == left.n
        got = [Mu.render(c).copy() for c in cams[2:]]
        st = [Mu.stats(r) for r in range(2)]
        assert [s["n_splats"] for s in st] == [left.n, left.n]
        assert [s["uploads"] for s in st] == [1, 1] and [s["moves"] for s in st] == [0, 0]
    want = M._fresh_frames(pkg, left, cams[2:])
    stale = M._fresh_frames(pkg, A, cams[2:])
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k])
        assert np.array_equal(got[k], want[k]), f"two ranks, frame {k}"
