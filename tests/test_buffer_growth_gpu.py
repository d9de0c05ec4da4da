"""One context's growable device buffers across small -> large -> small, and what the debug read-backs refuse.

The host code keeps its device buffers from call to call and replaces one only when a call needs more than it holds
(csrc/gsr_host_buffers.h).  Part 1 drives every such buffer through a growth and a reuse: ONE context renders 32 x 32, then 80 x 48,
then 32 x 32 again (or uploads 100, 4099, 100 splats), and every result is held, bit for bit, to a fresh context that does only that
one step.  A buffer that was freed and kept its capacity, a capacity that was kept for a freed buffer, a plane offset taken from a
stale capacity: each shows as a differing pixel (or a fault).  Every case ends with the live handles back where they were.

Part 2 pins what the debug read-backs (csrc/gsr_debug_read.h) refuse: a context without a frame, a wrong count, a NULL output --
and that a read-back leaves the context's next frame as it would have been."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

import test_move_gpu as M
import test_read_gpu as R
from helpers import assert_same_pixels

pytestmark = pytest.mark.gpu

N = 300                                   # four full clusters of 64 and one of 44
SIZES = ((32, 32), (80, 48), (32, 32))    # 4 tiles, 15 tiles, 4 tiles again
GSR_E_INVALID = -1


@contextlib.contextmanager
def _no_leak(E):
    gc.collect()                          # (an engine another test dropped goes now, not in the middle)
    base = E.live_handles()
    yield
    assert E.live_handles() == base


def _cams(pkg):
    return [pkg.camera.make_camera(w, h, sh_order=3, frame=1) for w, h in SIZES]


def _same(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_pixels(g, w, f"{label}, result {k}")


def _drive(pkg, step, prepare=lambda e: None, check=lambda e: None):
    """step(engine, camera) -> a list of arrays: one context through the three sizes, each size's results against a fresh context's"""
    s = M._cloud(pkg, 11, n=N)
    cams = _cams(pkg)
    with _no_leak(pkg.engine):
        with pkg.Engine(0) as U:
            prepare(U)
            U.upload(s)
            got = [step(U, c) for c in cams]
            check(U)
        fresh = {}
        for k, c in enumerate(cams):
            if SIZES[k] not in fresh:
                with pkg.Engine(0) as F:
                    prepare(F)
                    F.upload(s)
                    fresh[SIZES[k]] = step(F, c)
            _same(got[k], fresh[SIZES[k]], f"step {k}, {SIZES[k][0]} x {SIZES[k][1]}")
    return got


def _disc(cam):
    """a host depth buffer: the far plane, and a disc at view distance 4.2 in front of most of the cloud (the unit ball stands 4.62 away;
    window depth = 1 - near / distance for a far plane this far out)"""
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    d = np.ones((cam.height, cam.width), np.float32)
    d[(x - cam.width / 2) ** 2 + (y - cam.height / 2) ** 2 <= (0.3 * min(cam.width, cam.height)) ** 2] = np.float32(1.0 - 0.01 / 4.2)
    return d


# ---- 1. growth and reuse ------------------------------------------------------------------------------------------------------
def test_plain_frames(pkg):
    """the tile set, the list buffer, the tile order"""
    got = _drive(pkg, lambda e, c: [e.render(c)])
    assert all(g[0][..., 3].max() > 0 for g in got)
    assert_same_pixels(got[2][0], got[0][0], "32 x 32 before and after 80 x 48")


def test_depth_tested_frames(pkg):
    """the depth pyramids: five planes at offsets that are multiples of the capacity"""
    got = _drive(pkg, lambda e, c: [e.render_depth(c, _disc(c)), e.render_depth(c, _disc(c))])
    plain = _drive(pkg, lambda e, c: [e.render(c)])
    for g, p in zip(got, plain):
        assert g[0][..., 3].max() > 0 and not np.array_equal(g[0], p[0])      # (the disc really cut fragments, and left some)


def test_front_slab_frames_packed_and_over(pkg):
    """phase 1's transmittance and float32 pixels (tbuf, fb32), dropped by a change of target format and allocated again"""
    E = pkg.engine

    def step(e, c):
        bg = np.full((c.height, c.width, 4), 0.25, np.float32)
        e.set_target_format(E.TARGET_RGBA16F)
        out = [e.render(c), e.render_over(c, bg)]
        e.set_target_format(E.TARGET_RGBA32F)
        return out + [e.render_over(c, (0.1, 0.2, 0.3, 0.5)), e.render(c)]

    def check(e):
        assert e.stats()["frames_slab"] >= 3

    got = _drive(pkg, step, prepare=lambda e: e.set_option(E.OPT_FRONT_SLAB, 2), check=check)
    assert got[0][0].dtype == np.float16 and got[0][3].dtype == np.float32


def test_wire_frames(pkg):
    """the wire overlay's depth buffer and staged image"""
    got = _drive(pkg, lambda e, c: [e.render_wire(c)])
    assert all((g[0][..., 3] > 0).sum() > 20 for g in got)


def test_position_keyed_order(pkg):
    """OPT_SORT_CACHE = 2, the same camera twice at each size: the second frame takes the position-keyed order (blk_pre, pos_order)"""
    E = pkg.engine

    def check(e):
        assert e.stats()["sorts_skipped"] >= 3

    _drive(pkg, lambda e, c: [e.render(c), e.render(c)], prepare=lambda e: e.set_option(E.OPT_SORT_CACHE, 2), check=check)


def test_uploads_grow_and_shrink(pkg):
    """the upload arena, the Morton scratch, the sort histogram: 100 -> (an add that grows the capacity) -> 4099 -> 100 splats, each
    followed by a frame and a read; the read against the arrays, the frame against a fresh context's"""
    names = R._names(True)
    cam = pkg.camera.make_camera(48, 48, sh_order=3, frame=1)
    clouds = [M._cloud(pkg, 21, n=100), None, M._cloud(pkg, 22, n=4099), M._cloud(pkg, 23, n=100)]
    more = M._cloud(pkg, 24, n=400)
    clouds[1] = clouds[0].concat(more)
    with _no_leak(pkg.engine):
        got = []
        with pkg.Engine(0) as U:
            for k, s in enumerate(clouds):
                if k == 1:
                    assert U.add(more) == s.n and U.get_add()["grows"] == 1
                else:
                    U.upload(s)
                got.append(U.render(cam))
                R._assert_rows(U.read(), s, 0, s.n, names, f"step {k}: {s.n} splats")
        for k, s in enumerate(clouds):
            with pkg.Engine(0) as F:
                F.upload(s)
                assert_same_pixels(got[k], F.render(cam), f"step {k}: {s.n} splats")
            assert got[k][..., 3].max() > 0


# ---- 2. what the read-backs refuse --------------------------------------------------------------------------------------------
def _buf(n, dtype=np.uint32):
    return np.zeros(max(int(n), 1), dtype)


def _calls(eng, pkg, n, st):
    """{name: f(d, null) -> rc}: every read-back of the last frame with the counts it expects; d = 1: with a count it refuses, null:
    with a NULL output"""
    L, h, E = eng.L, eng.h, pkg.engine
    n_tiles, n_lists, n_pairs = st["tiles_x"] * st["tiles_y"], st["stiles_x"] * st["stiles_y"], st["pairs_total"]
    keep = []                             # (the arrays live as long as the calls do: the library writes through their addresses)

    def b(count, dtype=np.uint32, null=False):
        keep.append(_buf(count, dtype))
        return None if null else keep[-1].ctypes.data

    i32, cnt = np.int32, C.c_int64()
    return {
        "records": lambda d=0, null=False: L.gsr_debug_read_records(h, b(n + d, E.DEBUG_RECORD_DTYPE, null), n + d),
        "cull": lambda d=0, null=False: L.gsr_debug_read_cull(h, b(n + d, null=null), n + d, b(n), (n + 63) // 64, C.byref(cnt)),
        "depth_order": lambda d=0, null=False: L.gsr_debug_read_depth_order(h, b(n, i32, null), n - 2 * n * d, C.byref(cnt)),
        "tile_lists": lambda d=0, null=False: L.gsr_debug_read_tile_lists(h, b(n_lists + d, i32, null), b(n_lists + d, i32), n_lists + d,
                                                                        b(n_pairs, i32), n_pairs),
        "tile_lists, the pairs": lambda d=0, null=False: L.gsr_debug_read_tile_lists(h, b(n_lists, i32), b(n_lists, i32), n_lists,
                                                                                   b(n_pairs + d, i32, null), n_pairs + d),
        "tile_work": lambda d=0, null=False: L.gsr_debug_read_tile_work(h, b(4 * (n_tiles + d), null=null), n_tiles + d),
        # (a count other than the image's tiles is not refused: the read-back holds no tile count of its own; no tiles at all are)
        "horizons": lambda d=0, null=False: L.gsr_debug_read_horizons(h, b(4 * n_tiles, np.float32, null), n_tiles - n_tiles * d),
    }


def test_read_backs_need_a_frame(pkg):
    n = 65
    s = M._cloud(pkg, 31, n=n)
    with _no_leak(pkg.engine), pkg.Engine(0) as eng:
        eng.upload(s)
        st = dict(tiles_x=2, tiles_y=2, stiles_x=1, stiles_y=1, pairs_total=0)
        for name, call in _calls(eng, pkg, n, st).items():
            assert call() == GSR_E_INVALID, name
            assert eng.L.gsr_last_error(), name
        plan, big = _buf(32, np.int32), _buf(n + 1, np.int32)
        assert eng.L.gsr_debug_last_plan(eng.h, plan.ctypes.data) == GSR_E_INVALID
        order = eng.debug_storage_order(n)
        assert sorted(order.tolist()) == list(range(n))
        assert eng.L.gsr_debug_read_storage_order(eng.h, big.ctypes.data, n + 1) == GSR_E_INVALID
        assert eng.L.gsr_debug_read_storage_order(eng.h, None, n) == GSR_E_INVALID


def test_read_backs_after_a_frame(pkg):
    n = 65                                # one full cluster and one splat
    s = M._cloud(pkg, 31, n=n)
    cam, cam2 = (pkg.camera.make_camera(32, 32, sh_order=3, frame=f) for f in (1, 2))
    with _no_leak(pkg.engine):
        with pkg.Engine(0) as F:
            F.upload(s)
            first, second = F.render(cam), F.render(cam2)
        with pkg.Engine(0) as eng:
            eng.upload(s)
            assert_same_pixels(eng.render(cam), first, "the frame the read-backs look at")
            st = eng.stats()
            assert st["tiles_x"] * st["tiles_y"] == 4 and st["pairs_total"] > 0
            for name, call in _calls(eng, pkg, n, st).items():
                assert call() == 0, (name, eng.L.gsr_last_error())
                assert call(1) == GSR_E_INVALID, name + ": a wrong count"
                assert call(0, True) == GSR_E_INVALID, name + ": a NULL output"
            assert eng.L.gsr_debug_last_plan(eng.h, None) == GSR_E_INVALID
            # ... and what they hand back is the frame's
            depth_order = eng.debug_depth_order(n)
            assert 0 < len(depth_order) <= n and len(set(depth_order.tolist())) == len(depth_order)
            ts, te, pv = eng.debug_tile_lists()
            assert len(ts) == len(te) == st["stiles_x"] * st["stiles_y"] and (ts <= te).all()
            assert len(pv) == st["pairs_total"] and set(pv.tolist()) <= set(depth_order.tolist())
            assert eng.debug_records(n)["visible"].sum() == len(depth_order)
            assert eng.debug_tile_work().shape == (2, 2, 4) and eng.debug_horizons(2, 2).shape == (4, 2, 2)
            # (a frame this small leaves no horizons: the pyramid's door says so in its own name; a context that prepares them on every
            #  frame hands back six levels over the 2 x 2 tiles, and refuses another count and NULL outputs)
            pyr, words = _buf(4 + 5, np.float32), _buf(24, np.int32)
            assert eng.L.gsr_debug_read_horizon_pyramid(eng.h, pyr.ctypes.data, 9, words.ctypes.data) == GSR_E_INVALID
            assert b"gsr_debug_read_horizon_pyramid" in eng.L.gsr_last_error()
            with pkg.Engine(0) as H:
                H.set_option(pkg.engine.OPT_OCCLUSION_CULL, 2)
                H.upload(s)
                assert H.L.gsr_debug_read_horizon_pyramid(H.h, pyr.ctypes.data, 9, words.ctypes.data) == GSR_E_INVALID, "no frame yet"
                assert_same_pixels(H.render(cam), first, "the frame that leaves horizons")
                levels, meta = H.debug_horizon_pyramid()
                assert [l.shape for l in levels] == [(2, 2)] + [(1, 1)] * 5 and all(l.dtype == np.float32 for l in levels)
                assert set(meta) == set(pkg.engine.PYRAMID_META_FIELDS) and meta["pyr_off"] == [0, 4, 5, 6, 7, 8]
                assert (meta["tiles_x"], meta["tiles_y"], meta["horizon_valid"], meta["rect_shift"]) == (2, 2, 1, 0)
                assert np.array_equal(levels[0].view(np.uint32), H.debug_horizons(2, 2)[0].view(np.uint32))
                for count, out, wd in ((8, pyr, words), (10, pyr, words), (9, None, words), (9, pyr, None)):
                    rc = H.L.gsr_debug_read_horizon_pyramid(H.h, None if out is None else out.ctypes.data, count, None if wd is None else wd.ctypes.data)
                    assert rc == GSR_E_INVALID, (count, out is None, wd is None)
                words[:] = 0                # (no output and no count: the words alone)
                assert H.L.gsr_debug_read_horizon_pyramid(H.h, None, 0, words.ctypes.data) == 0 and words[:3].tolist() == [2, 2, 0]
            assert set(eng.debug_last_plan()) == set(pkg.engine.PLAN_FIELDS)
            # the pipeline's sort on 1000 pairs, both forms
            rng = np.random.default_rng(5)
            keys = rng.integers(0, 1 << 20, 1000, dtype=np.uint64).astype(np.uint32)
            keys[:300] = keys[300:600]    # (ties: stability matters)
            vals = np.arange(1000, dtype=np.uint32)
            order = np.argsort(keys, kind="stable")
            for local in (None, (0, 10), (int(keys.min()), 11)):
                k, v = eng.debug_sort_pairs(keys, vals, 20, local=local)
                assert np.array_equal(k, keys[order]) and np.array_equal(v, vals[order]), local
            assert eng.L.gsr_debug_sort_pairs_local(eng.h, keys.ctypes.data, vals.ctypes.data, 1000, 20, 0, 32) == GSR_E_INVALID
            assert eng.L.gsr_debug_sort_pairs(eng.h, None, vals.ctypes.data, 1000, 20) == GSR_E_INVALID
            assert_same_pixels(eng.render(cam2), second, "the frame behind the read-backs")
