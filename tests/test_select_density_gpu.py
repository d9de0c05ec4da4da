"""Selection by density on the GPU (gsr_select_density): resident splats picked by how many neighbours they have in a grid of cells.

Everything is BIT-EXACT, so there are no tolerances.  What a mask, the counts and the result must hold comes from
gsr_select_density_eval (the rule on the host) over Engine.read() of the same context -- itself held to the uploaded arrays -- the numpy
restatement of density_cases.py, the numpy restatement of the op and a random prior mask with garbage behind n; never from the GPU
path.  Each case runs under both GSR_OPT_STORAGE_ORDER values."""
import ctypes as C

import numpy as np
import pytest

import density_cases as DC
import test_move_gpu as M
from helpers import HipBuffers

GSR_E_INVALID = -1
GUARD = 16                   # words on either side of every mask and every count array
FILL = 0xA5A5A5A5
NAMES = DC.case_names()


def _guarded(words):
    return np.concatenate([np.full(GUARD, FILL, np.uint32), words.astype(np.uint32), np.full(GUARD, FILL, np.uint32)])


def _select_raw(pkg, eng, hb, rule, prior_words, device, counts=True):
    """gsr_select_density through the C ABI into a guarded mask that holds prior_words and a guarded count array, both in device or
    both in host memory -> (words, counts, result fields, n_hit, n_set); asserts that the guard words in front of and behind both
    destinations are unchanged"""
    L, E = pkg.load_library(), pkg.engine
    n = eng.read_info()["n_splats"]
    buf, cbuf = _guarded(prior_words), _guarded(np.full(n, 0x5EED5EED, np.uint32))
    hit, nset, res = C.c_int64(-1), C.c_int64(-1), E.gsr_density_result()
    if device:
        base, cbase = hb.upload(buf), hb.upload(cbuf)
        rc = L.gsr_select_density(eng.h, C.byref(rule), C.c_void_p(base + 4 * GUARD), 1, C.c_void_p(cbase + 4 * GUARD) if counts else None, 1,
                                  C.byref(res), C.byref(hit), C.byref(nset))
        out, cout = hb.download(base, buf.shape, np.uint32), hb.download(cbase, cbuf.shape, np.uint32)
    else:
        out, cout = buf.copy(), cbuf.copy()
        rc = L.gsr_select_density(eng.h, C.byref(rule), out.ctypes.data + 4 * GUARD, 0, cout.ctypes.data + 4 * GUARD if counts else None, 0,
                                  C.byref(res), C.byref(hit), C.byref(nset))
    assert rc == 0, L.gsr_last_error()
    for a in (out, cout):
        assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all(), "a guard word changed"
    if not counts:
        assert (cout[GUARD:-GUARD] == 0x5EED5EED).all()
    return out[GUARD:-GUARD], cout[GUARD:-GUARD], res.fields(), hit.value, nset.value


def _check(pkg, eng, hb, make_rule, want, prior, words, label, ops=range(5)):
    """every op, into device memory and into host memory; make_rule(op) -> gsr_density_rule; want = (hit, counts, result fields)"""
    E = pkg.engine
    want_hit, want_cnt, want_res = want
    for op in ops:
        m = DC.apply_op(op, prior, want_hit)
        for device in (True, False):
            got, cnt, res, n_hit, n_set = _select_raw(pkg, eng, hb, make_rule(op), words, device)
            tag = f"{label} op {DC.OPS[op]} {'device' if device else 'host'} memory"
            assert np.array_equal(got, E.pack_mask(m)), tag                # (pack_mask leaves the bits at and behind n clear)
            assert np.array_equal(cnt, want_cnt), (tag, np.flatnonzero(cnt != want_cnt)[:10])
            assert res == want_res, (tag, res[:3], want_res[:3])
            assert (n_hit, n_set) == (int(want_hit.sum()), int(m.sum())), (tag, n_hit, n_set)


def _read_equals(R, s):
    """Engine.read() of a context holds the uploaded arrays the rule looks at, bit for bit"""
    assert np.array_equal(R.P.view(np.uint32), np.ascontiguousarray(s.P, np.float32).view(np.uint32))
    assert np.array_equal(R.alpha.view(np.uint32), np.ascontiguousarray(s.alpha, np.float32).view(np.uint32))


# ---- 1. per case and op ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_masks_counts_and_result_per_case_and_op(pkg, name, order):
    E = pkg.engine
    c = DC.case(pkg, name)
    prior, words = DC.prior_words(pkg, c.n, 40 + c.n)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats)
            assert U.get_select_density() == {"selects": 0, "hit_last": 0, "ms": [0.0] * 4}, "a context that never called the verb"
            R = U.read()
            _read_equals(R, c.splats)
            want = c.eval(pkg, cloud=R)
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op), want, prior, words, name)
            sel = U.get_select_density()
            assert sel["selects"] == 10 and sel["hit_last"] == int(want[0].sum()) and sel["ms"][0] > 0.0 and sel["ms"][2] > 0.0, sel
            assert sel["ms"][3] >= sel["ms"][0] + sel["ms"][2], sel
            assert U.get_select()["selects"] == 0 and U.get_select_attrs()["selects"] == 0, "a sibling's tally counted a density select"
            # counts_out NULL: the mask and the result alone
            got, _, res, n_hit, _ = _select_raw(pkg, U, hb, c.rule(pkg), words, True, counts=False)
            assert np.array_equal(got, E.pack_mask(want[0])) and res == want[2] and n_hit == int(want[0].sum())
            # the Python door: Engine.select_density and Engine.select_density_device
            mask, n_hit, n_set, res, cnt = U.select_density(c.rule(pkg, op=E.SELECT_TOGGLE), prior, counts=True)
            assert np.array_equal(mask, prior ^ want[0]) and (n_hit, n_set) == (int(want[0].sum()), int((prior ^ want[0]).sum()))
            assert np.array_equal(cnt, want[1]) and res.fields() == want[2]
            mask, n_hit, n_set, res = U.select_density(c.rule(pkg))
            assert np.array_equal(mask, want[0]) and res.fields() == want[2]
            dm, dc = hb.upload(words), hb.upload(np.zeros(c.n, np.uint32))
            n_hit, n_set, res = U.select_density_device(c.rule(pkg, op=E.SELECT_ADD), dm, dc)
            assert (n_hit, n_set) == (int(want[0].sum()), int((prior | want[0]).sum())) and res.fields() == want[2]
            assert np.array_equal(hb.download(dm, words.shape, np.uint32), E.pack_mask(prior | want[0]))
            assert np.array_equal(hb.download(dc, (c.n,), np.uint32), want[1])
    finally:
        hb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("n257_sh", "n4097_nosh", "faces_r2"))
def test_reach_and_ranges(pkg, name):
    """each reach, an empty range, the full range, no alpha floor, HIT_OUTSIDE: one context, the rule changes from call to call"""
    c = DC.case(pkg, name)
    prior, words = DC.prior_words(pkg, c.n, 11)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(c.splats)
            R = U.read()
            for over in DC.variants():
                want = c.eval(pkg, cloud=R, **over)
                assert np.array_equal(want[0], c.restate(**over)[0]), over
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, **over), want, prior, words, f"{name} {over}", ops=(0, 4))
    finally:
        hb.free()


# ---- 2. under a visibility in force ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, order):
    """without SKIP_HIDDEN a hidden splat counts with its TRUE alpha (its resident opacity is +0); with it, not at all"""
    E = pkg.engine
    c = DC.case(pkg, "n4097_sh")
    s = c.splats
    volumes = [E.crop_box((0.1, 0.0, 0.0), 0.4)]
    hide = np.arange(c.n) % 4 == 3
    vis_struct, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(vis_struct, s.P)
    assert (~visible).sum() > 500 and visible.sum() > 500
    prior, words = DC.prior_words(pkg, c.n, 77)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            base = c.eval(pkg)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA, hidden_count = U.debug_resident(E.RESIDENT_GEOA), U.get_visibility()[1]
            R = U.read()
            _read_equals(R, s)
            plain = c.eval(pkg, cloud=R, vis=vis_struct)
            skip = c.eval(pkg, cloud=R, vis=vis_struct, skip_hidden=True)
            assert plain[2] == base[2] and np.array_equal(plain[1], base[1]), "a hidden splat counts with its true alpha"
            assert np.array_equal(skip[0], c.restate(hidden=~visible, skip_hidden=True)[0]) and (skip[1][~visible] == 0).all() and skip[2][0] < plain[2][0]
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op), plain, prior, words, "visibility", ops=(0, 1, 4))
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, skip_hidden=True), skip, prior, words, "skip hidden", ops=(0, 2, 3))
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA) and U.get_visibility()[1] == hidden_count
            # a mask alone (no volume), then nothing in force: SKIP_HIDDEN hides nothing
            U.set_visibility(mask=hide)
            vm, keep2 = E.visibility_struct((), hide)
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, skip_hidden=True), c.eval(pkg, vis=vm, skip_hidden=True), prior, words, "a mask alone", ops=(0,))
            U.set_visibility()
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, skip_hidden=True), base, prior, words, "the visibility cleared", ops=(0,))
    finally:
        hb.free()


# ---- 3. after a remove and an add: the new index space -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_after_remove_and_add(pkg):
    E = pkg.engine
    c = DC.case(pkg, "n4097_nosh")
    gone = np.random.default_rng(8).random(c.n) < 0.3
    extra = DC.case(pkg, "n257_nosh").splats
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(c.splats)
            s = c.splats.subset(~gone)
            assert U.remove(gone) == s.n
            for label, cloud in (("after a remove", s), ("after an add", None)):
                if cloud is None:
                    cloud = s.concat(extra)
                    assert U.add(extra) == cloud.n
                want = c.eval(pkg, cloud=cloud)
                assert 0 < want[0].sum() < cloud.n and (cloud.n + 31) // 32 != (c.n + 31) // 32
                prior, words = DC.prior_words(pkg, cloud.n, 5)
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op), want, prior, words, label, ops=(0, 4))
    finally:
        hb.free()


# ---- 4. the clean-up workflow: select the floaters into a device mask, remove by it ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_floaters_go_from_the_device_mask(pkg, order):
    E = pkg.engine
    c = DC.case(pkg, "floaters")
    s, lone = c.splats, c.marks["lone"]
    assert np.array_equal(c.restate()[0], lone) and lone.sum() == DC.N_FLOATERS
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            dm = hb.upload(np.full((c.n + 31) // 32, 0xffffffff, np.uint32))
            n_hit, n_set, res = U.select_density_device(c.rule(pkg), dm)
            assert (n_hit, n_set) == (17, 17) and res.count_hist[0] == 17 and res.n_population == c.n
            assert np.array_equal(hb.download(dm, ((c.n + 31) // 32,), np.uint32), E.pack_mask(lone))
            assert U.remove_device(dm) == c.n - 17                        # nothing crossed the link in between
            got, R = M._planes(U), U.read()
        blob = s.subset(~lone)
        M._assert_same_planes(got, M._fresh_planes(pkg, blob, order, True), f"select_density + remove, order {order}")
        _read_equals(R, blob)
    finally:
        hb.free()


# ---- 5. nothing is invalidated ---------------------------------------------------------------------------------------------------------------
KEPT = ("uploads", "moves", "upload_ms", "move_ms")


@pytest.mark.gpu
def test_a_select_keeps_the_cached_order_and_the_stats(pkg):
    c = DC.case(pkg, "n4097_sh")
    cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        frame = U.render(cam).copy()
        U.render(cam)
        st = U.stats()
        assert st["sorts_skipped"] >= 1
        planes = M._planes(U)
        assert np.array_equal(U.select_density(c.rule(pkg))[0], c.eval(pkg)[0])
        assert U.stats() == st, "a select changed gsr_stats"
        again = U.render(cam)
        st2 = U.stats()
        assert st2["sorts_skipped"] == st["sorts_skipped"] + 1, "the select invalidated the cached depth order"
        assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
        for k in KEPT:
            assert st2[k] == st[k], (k, st[k], st2[k])
        M._assert_same_planes(M._planes(U), planes, "a select between frames")


@pytest.mark.gpu
def test_a_select_keeps_the_depth_horizons(pkg):
    """a cloud that fills the frame, culled against the previous frame's horizons (the scene of test_select_gpu): the frames around a
    density select are culled as those of a context that never selects, none is repaired, and gsr_get_stats is otherwise the same"""
    E = pkg.engine
    s = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    s.alpha[:] = 0.97
    s.alpha[::3] = 0.5
    cams = [pkg.camera.make_camera(200, 120, sh_order=3, frame=180 + k, step_deg=0.25, distance=2.2) for k in range(6)]
    lo, hi = s.P.min(axis=0), s.P.max(axis=0)
    origin, cell = E.density_grid(lo, hi, float((hi - lo).max()) / 40)
    rule = E.density_rule(cell, origin, reach=1, count=(1, 30), alpha_min=0.6)
    want, want_cnt = E.select_density_eval(rule, s.P, s.alpha, counts=True)
    assert 1000 < want.sum() < s.n - 1000

    def run(select):
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_OCCLUSION_CULL, 2)
            U.upload(s)
            out, stats = [], []
            for k, cam in enumerate(cams):
                if select and k == 3:
                    mask, n_hit, n_set, res, cnt = U.select_density(rule, counts=True)
                    assert np.array_equal(mask, want) and n_hit == n_set == int(want.sum()) and np.array_equal(cnt, want_cnt)
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


# ---- 6. refusals, with nothing written ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    import test_select_density as T
    E, L = pkg.engine, pkg.load_library()
    c = DC.case(pkg, "n257_sh")
    words = (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.upload(np.full(size // 4, FILL, np.uint32))
        croom = hb.upload(np.full(size // 4, FILL, np.uint32))
        host_mask, host_cnt = np.full(words + 2, FILL, np.uint32), np.full(c.n + 2, FILL, np.uint32)
        cnt = [C.c_int64(-7), C.c_int64(-7)]
        res = E.gsr_density_result()
        res.n_cells = -7
        ok = c.rule(pkg, op=E.SELECT_TOGGLE)

        def call(eng, rule=ok, mask=room, device=1, counts=croom, cdevice=1):
            return L.gsr_select_density(eng.h, C.byref(rule) if rule is not None else None, C.c_void_p(mask) if mask is not None else None, device,
                                        C.c_void_p(counts) if counts is not None else None, cdevice, C.byref(res), C.byref(cnt[0]), C.byref(cnt[1]))

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()                    # before any upload
            assert call(U, mask=host_mask.ctypes.data, device=0, counts=host_cnt.ctypes.data, cdevice=0) == GSR_E_INVALID
            U.upload(c.splats)
            cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
            frame = U.render(cam).copy()
            U.render(cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            cases = {"NULL rule": lambda: call(U, rule=None), "NULL mask": lambda: call(U, mask=None),
                     "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, device=1),
                     "misaligned mask": lambda: call(U, mask=room + 2),
                     "mask past its allocation": lambda: call(U, mask=room + size - (words * 4 - 4)),
                     "pageable counts": lambda: call(U, counts=host_cnt.ctypes.data, cdevice=1),
                     "misaligned counts": lambda: call(U, counts=croom + 2),
                     "counts past their allocation": lambda: call(U, counts=croom + size - (c.n * 4 - 4)),
                     "host mask, counts past their allocation": lambda: call(U, mask=host_mask.ctypes.data, device=0, counts=croom + size - 8)}
            for label, r in T._bad_rules(pkg):
                for device in (1, 0):
                    cases[f"{label}, {'device' if device else 'host'} memory"] = (
                        lambda r=r, device=device: call(U, rule=r, mask=room if device else host_mask.ctypes.data, device=device,
                                                        counts=croom if device else host_cnt.ctypes.data, cdevice=device))
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_select_density" in L.gsr_last_error(), label
                assert np.array_equal(U.render(cam), frame), label
                assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
            M._assert_same_planes(M._planes(U), planes, "refusals")
            assert cnt[0].value == -7 and cnt[1].value == -7 and res.n_cells == -7 and (host_mask == FILL).all() and (host_cnt == FILL).all()
            for base in (room, croom):
                assert (hb.download(base, (size // 4,), np.uint32) == FILL).all(), "a refused select wrote to device memory"
            assert U.get_select_density() == {"selects": 0, "hit_last": 0, "ms": [0.0] * 4}
            assert L.gsr_get_select_density(U.h, None, None, None) == 0   # every pointer may be NULL
            # the counts, the result and either count may be NULL
            assert L.gsr_select_density(U.h, C.byref(ok), C.c_void_p(room), 1, None, 0, None, None, None) == 0 and U.get_select_density()["selects"] == 1
            # an upload in progress
            assert L.gsr_upload_begin(U.h, c.n, 1, None) == 0
            assert call(U) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_upload_abort(U.h) == 0
    finally:
        hb.free()


# ---- 7. the empty cloud ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_cloud(pkg):
    E, L = pkg.engine, pkg.load_library()
    c = DC.case(pkg, "n65_nosh")
    host_mask, host_cnt = np.full(2, FILL, np.uint32), np.full(2, FILL, np.uint32)
    cnt = [C.c_int64(-7), C.c_int64(-7)]
    res = E.gsr_density_result()
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        assert U.remove(np.ones(c.n, bool)) == 0
        for op in range(5):
            r = c.rule(pkg, op=op)
            res.n_population = -7
            assert L.gsr_select_density(U.h, C.byref(r), host_mask.ctypes.data, 0, host_cnt.ctypes.data, 0, C.byref(res), C.byref(cnt[0]), C.byref(cnt[1])) == 0
            assert cnt[0].value == 0 and cnt[1].value == 0 and (host_mask == FILL).all() and (host_cnt == FILL).all()
            assert res.fields() == (0, 0, 0, (0,) * 64)
        mask, n_hit, n_set, res, counts = U.select_density(c.rule(pkg), counts=True)
        assert mask.shape == counts.shape == (0,) and (n_hit, n_set) == (0, 0)
        assert U.get_select_density()["selects"] == 0


# ---- 8. several ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_select_density(pkg):
    E = pkg.engine
    c = DC.case(pkg, "n4097_sh")
    prior, _ = DC.prior_words(pkg, c.n, 9)
    want = c.eval(pkg)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        single = [U.select_density(c.rule(pkg, op=op), prior, counts=True) for op in range(5)]
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(c.splats)
        for op in range(5):
            mask, n_hit, n_set, res, cnt = Mu.select_density(c.rule(pkg, op=op), prior, counts=True)
            m = DC.apply_op(op, prior, want[0])
            assert np.array_equal(mask, m) and np.array_equal(mask, single[op][0]) and (n_hit, n_set) == single[op][1:3], op
            assert res.fields() == want[2] == single[op][3].fields() and np.array_equal(cnt, want[1]) and np.array_equal(cnt, single[op][4]), op
        mask, n_hit, n_set, res = Mu.select_density(c.rule(pkg))
        assert np.array_equal(mask, want[0])
        assert [Mu.stats(r)["n_splats"] for r in range(2)] == [c.n, c.n]
