"""Selection by attribute on the GPU (gsr_select_attrs): resident splats picked by their true alpha, their scale halves, their base colour
and crop volumes.

Everything is BIT-EXACT, so there are no tolerances.  What a mask must hold comes from gsr_select_attrs_eval (the rule on the host) over
Engine.read() of the same context -- itself held to the uploaded arrays -- the numpy restatement of attr_select_cases.py, the numpy
restatement of the op and a random prior mask with garbage behind n; never from the GPU path.  Each case runs under both
GSR_OPT_STORAGE_ORDER values."""
import ctypes as C

import numpy as np
import pytest

import attr_select_cases as AC
import test_move_gpu as M
from helpers import HipBuffers

GSR_E_INVALID = -1
GUARD = 16                   # words on either side of every mask
FILL = 0xA5A5A5A5
NAMES = AC.case_names()
RULES = [AC.CLAUSES, ()] + [(k,) for k in AC.CLAUSES]       # every clause, none, each alone


def _guarded(words):
    return np.concatenate([np.full(GUARD, FILL, np.uint32), words.astype(np.uint32), np.full(GUARD, FILL, np.uint32)])


def _select_raw(pkg, eng, hb, rule, prior_words, device):
    """gsr_select_attrs through the C ABI into a guarded mask that holds prior_words, in device or host memory -> (words, n_hit, n_set);
    asserts that the guard words in front of and behind the destination are unchanged"""
    L = pkg.load_library()
    buf = _guarded(prior_words)
    hit, nset = C.c_int64(-1), C.c_int64(-1)
    if device:
        base = hb.upload(buf)
        rc = L.gsr_select_attrs(eng.h, C.byref(rule), C.c_void_p(base + 4 * GUARD), 1, C.byref(hit), C.byref(nset))
        out = hb.download(base, buf.shape, np.uint32)
    else:
        out = buf.copy()
        rc = L.gsr_select_attrs(eng.h, C.byref(rule), out.ctypes.data + 4 * GUARD, 0, C.byref(hit), C.byref(nset))
    assert rc == 0, L.gsr_last_error()
    assert (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all(), "a guard word changed"
    return out[GUARD:-GUARD], hit.value, nset.value


def _check(pkg, eng, hb, make_rule, want_hit, prior, words, label):
    """every op, into a device mask and into a host mask; make_rule(op) -> gsr_attr_rule"""
    E = pkg.engine
    for op in range(5):
        want = AC.apply_op(op, prior, want_hit)
        for device in (True, False):
            got, n_hit, n_set = _select_raw(pkg, eng, hb, make_rule(op), words, device)
            tag = f"{label} op {AC.OPS[op]} {'device' if device else 'host'} mask"
            assert np.array_equal(got, E.pack_mask(want)), tag          # (pack_mask leaves the bits at and behind n clear)
            assert (n_hit, n_set) == (int(want_hit.sum()), int(want.sum())), (tag, n_hit, n_set)


def _read_equals(R, s):
    """Engine.read() of a context holds the uploaded arrays the rule looks at, bit for bit"""
    assert np.array_equal(R.P.view(np.uint32), np.ascontiguousarray(s.P, np.float32).view(np.uint32))
    assert np.array_equal(R.alpha.view(np.uint32), np.ascontiguousarray(s.alpha, np.float32).view(np.uint32))
    assert np.array_equal(R.scale, s.scale) and np.array_equal(R.Cd, s.Cd)


# ---- 1. per case and op ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_masks_per_case_and_op(pkg, name, order):
    E = pkg.engine
    c = AC.case(pkg, name)
    prior, words = AC.prior_words(pkg, c.n, 40 + c.n)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats)
            R = U.read()
            _read_equals(R, c.splats)
            for only in RULES:
                want = c.eval(pkg, cloud=R, only=only)
                assert np.array_equal(want, c.restate(pkg, cloud=R, only=only)), only
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, only=only), want, prior, words, f"{name} {only}")
            sel = U.get_select_attrs()
            last = c.eval(pkg, cloud=R, only=RULES[-1])
            assert sel["selects"] == 10 * len(RULES) and sel["hit_last"] == int(last.sum()) and sel["ms"][0] > 0.0 and sel["ms"][3] >= sel["ms"][0], sel
            assert U.get_select()["selects"] == 0, "the screen-region tally counted an attribute select"
            # the Python door: Engine.select_attrs and Engine.select_attrs_device
            want = c.eval(pkg, cloud=R)
            mask, n_hit, n_set = U.select_attrs(c.rule(pkg, op=E.SELECT_TOGGLE), prior)
            assert np.array_equal(mask, prior ^ want) and (n_hit, n_set) == (int(want.sum()), int((prior ^ want).sum()))
            mask, n_hit, n_set = U.select_attrs(c.rule(pkg))
            assert np.array_equal(mask, want)
            dm = hb.upload(words)
            assert U.select_attrs_device(c.rule(pkg, op=E.SELECT_ADD), dm) == (int(want.sum()), int((prior | want).sum()))
            assert np.array_equal(hb.download(dm, words.shape, np.uint32), E.pack_mask(prior | want))
    finally:
        hb.free()


# ---- 2. under a visibility in force ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, order):
    """the alpha clause sees the TRUE alpha: a hidden splat of alpha 0.5 is hit by [0.4, 0.6] though its resident opacity is +0;
    SKIP_HIDDEN drops it (volumes and mask in force, through gsr_splat_visible)"""
    E = pkg.engine
    c = AC.case(pkg, "n357_sh")
    s = M._copy(pkg, c.splats)
    target = 7
    s.alpha[target] = np.float32(0.5)
    volumes = [E.crop_box((0.1, 0.0, 0.0), 0.4)]
    hide = np.arange(c.n) % 4 == 3
    hide[target] = True
    vis_struct, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(vis_struct, s.P)
    assert not visible[target] and (~visible).sum() > 50
    prior, words = AC.prior_words(pkg, c.n, 77)
    band = E.attr_rule(alpha=(0.4, 0.6))
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA, hidden_count = U.debug_resident(E.RESIDENT_GEOA), U.get_visibility()[1]
            R = U.read()
            _read_equals(R, s)
            for only in RULES:
                plain = E.select_attrs_eval(c.rule(pkg, only=only), R.P, R.alpha, R.scale, R.Cd, vis=vis_struct)
                skip = E.select_attrs_eval(c.rule(pkg, only=only, skip_hidden=True), R.P, R.alpha, R.scale, R.Cd, vis=vis_struct)
                assert np.array_equal(skip, plain & visible) and np.array_equal(skip, AC.restate(
                    pkg, AC.rule_params(pkg, only=only), R.P, R.alpha, R.scale, R.Cd, hidden=~visible, skip_hidden=True))
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, only=only), plain, prior, words, f"visibility {only}")
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, only=only, skip_hidden=True), skip, prior, words, f"skip hidden {only}")
            mask, n_hit, _ = U.select_attrs(band)
            assert mask[target] and np.array_equal(mask, (s.alpha >= np.float32(0.4)) & (s.alpha <= np.float32(0.6)))
            band.flags = E.ATTR_SKIP_HIDDEN
            mask, _, _ = U.select_attrs(band)
            assert not mask[target] and np.array_equal(mask, (s.alpha >= np.float32(0.4)) & (s.alpha <= np.float32(0.6)) & visible)
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA) and U.get_visibility()[1] == hidden_count
            # a mask alone (no volume), then nothing in force: SKIP_HIDDEN hides nothing
            U.set_visibility(mask=hide)
            mask, _, _ = U.select_attrs(band)
            assert np.array_equal(mask, (s.alpha >= np.float32(0.4)) & (s.alpha <= np.float32(0.6)) & ~hide)
            U.set_visibility()
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, skip_hidden=True), c.eval(pkg, cloud=s), prior, words, "the visibility cleared")
    finally:
        hb.free()


# ---- 3. after a remove and an add: the new index space -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_after_remove_and_add(pkg):
    E = pkg.engine
    c = AC.case(pkg, "n357_nosh")
    gone = np.random.default_rng(8).random(c.n) < 0.3
    extra = AC.case(pkg, "n65_nosh").splats
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
                assert 0 < want.sum() < cloud.n and (cloud.n + 31) // 32 != (c.n + 31) // 32
                prior, words = AC.prior_words(pkg, cloud.n, 5)
                for op in (E.SELECT_REPLACE, E.SELECT_TOGGLE):
                    for device in (True, False):
                        got, n_hit, n_set = _select_raw(pkg, U, hb, c.rule(pkg, op=op), words, device)
                        m = AC.apply_op(op, prior, want)
                        assert np.array_equal(got, E.pack_mask(m)) and (n_hit, n_set) == (int(want.sum()), int(m.sum())), (label, op, device)
    finally:
        hb.free()


# ---- 4. the prune workflow: select into a device mask, remove by it -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_prune_from_the_device_mask(pkg, order):
    E = pkg.engine
    c = AC.case(pkg, "n357_sh")
    prune = dict(alpha=(-np.inf, 0.2))                                   # the trainer's opacity prune ...
    rule = E.attr_rule(**prune)
    s = c.splats
    with np.errstate(invalid="ignore"):
        gone = s.alpha <= np.float32(0.2)                                # ... restated in numpy (a NaN alpha stays)
    assert 0 < gone.sum() < c.n
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            dm = hb.upload(np.full((c.n + 31) // 32, 0xffffffff, np.uint32))
            assert U.select_attrs_device(rule, dm) == (int(gone.sum()), int(gone.sum()))
            assert U.remove_device(dm) == int((~gone).sum())              # nothing crossed the link in between
            got, R = M._planes(U), U.read()
        left = s.subset(~gone)
        M._assert_same_planes(got, M._fresh_planes(pkg, left, order, True), f"select_attrs + remove, order {order}")
        _read_equals(R, left)
        assert np.array_equal(R.orient, left.orient)
        for k in ("shx", "shy", "shz"):                                  # (index 15 is not resident: it reads back as 0)
            assert np.array_equal(getattr(R, k)[:, :15], getattr(left, k)[:, :15]), k
    finally:
        hb.free()


# ---- 5. nothing is invalidated ---------------------------------------------------------------------------------------------------------------
KEPT = ("uploads", "moves", "upload_ms", "move_ms")


@pytest.mark.gpu
def test_a_select_keeps_the_cached_order_and_the_stats(pkg):
    c = AC.case(pkg, "n357_sh")
    cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        frame = U.render(cam).copy()
        U.render(cam)
        st = U.stats()
        assert st["sorts_skipped"] >= 1
        planes = M._planes(U)
        assert np.array_equal(U.select_attrs(c.rule(pkg))[0], c.eval(pkg))
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
    select are culled as those of a context that never selects, none is repaired, and gsr_get_stats is otherwise the same"""
    E = pkg.engine
    s = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    s.alpha[:] = 0.97
    s.alpha[::3] = 0.5
    cams = [pkg.camera.make_camera(200, 120, sh_order=3, frame=180 + k, step_deg=0.25, distance=2.2) for k in range(6)]
    rule = E.attr_rule(alpha=(0.4, 0.6), volumes=[E.crop_ellipsoid((0.0, 0.0, 0.0), 0.6)])
    want = E.select_attrs_eval(rule, s.P, s.alpha)
    assert 1000 < want.sum() < s.n - 1000

    def run(select):
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_OCCLUSION_CULL, 2)
            U.upload(s)
            out, stats = [], []
            for k, cam in enumerate(cams):
                if select and k == 3:
                    mask, n_hit, n_set = U.select_attrs(rule)
                    assert np.array_equal(mask, want) and n_hit == n_set == int(want.sum())
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
    import test_select_attrs as T
    E, L = pkg.engine, pkg.load_library()
    c = AC.case(pkg, "n357_sh")
    words = (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.upload(np.full(size // 4, FILL, np.uint32))
        host_mask = np.full(words + 2, FILL, np.uint32)
        cnt = [C.c_int64(-7), C.c_int64(-7)]
        ok = c.rule(pkg, op=E.SELECT_TOGGLE)

        def call(eng, rule=ok, mask=room, device=1):
            return L.gsr_select_attrs(eng.h, C.byref(rule) if rule is not None else None, C.c_void_p(mask) if mask is not None else None,
                                      device, C.byref(cnt[0]), C.byref(cnt[1]))

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()                    # before any upload
            assert call(U, mask=host_mask.ctypes.data, device=0) == GSR_E_INVALID
            U.upload(c.splats)
            cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
            frame = U.render(cam).copy()
            U.render(cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            cases = {"NULL rule": lambda: call(U, rule=None), "NULL mask": lambda: call(U, mask=None),
                     "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, device=1),
                     "misaligned mask": lambda: call(U, mask=room + 2),
                     "mask past its allocation": lambda: call(U, mask=room + size - (words * 4 - 4))}
            for label, r in T._bad_rules(pkg):
                for device in (1, 0):
                    cases[f"{label}, {'device' if device else 'host'} mask"] = (lambda r=r, device=device:
                                                                                 call(U, rule=r, mask=room if device else host_mask.ctypes.data, device=device))
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_select_attrs" in L.gsr_last_error(), label
                assert np.array_equal(U.render(cam), frame), label
                assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
            M._assert_same_planes(M._planes(U), planes, "refusals")
            assert cnt[0].value == -7 and cnt[1].value == -7 and (host_mask == FILL).all()
            assert (hb.download(room, (size // 4,), np.uint32) == FILL).all(), "a refused select wrote to device memory"
            assert U.get_select_attrs() == {"selects": 0, "hit_last": 0, "ms": [0.0] * 4}
            assert L.gsr_get_select_attrs(U.h, None, None, None) == 0   # every pointer may be NULL
            # either count may be NULL
            assert L.gsr_select_attrs(U.h, C.byref(ok), C.c_void_p(room), 1, None, None) == 0 and U.get_select_attrs()["selects"] == 1
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
    c = AC.case(pkg, "n33_nosh")
    host_mask = np.full(2, FILL, np.uint32)
    cnt = [C.c_int64(-7), C.c_int64(-7)]
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        assert U.remove(np.ones(c.n, bool)) == 0
        for op in range(5):
            r = c.rule(pkg, op=op)
            assert L.gsr_select_attrs(U.h, C.byref(r), host_mask.ctypes.data, 0, C.byref(cnt[0]), C.byref(cnt[1])) == 0
            assert cnt[0].value == 0 and cnt[1].value == 0 and (host_mask == FILL).all()
        mask, n_hit, n_set = U.select_attrs(E.attr_rule())
        assert mask.shape == (0,) and (n_hit, n_set) == (0, 0)
        assert U.get_select_attrs()["selects"] == 0


# ---- 8. several ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_select_attrs(pkg):
    E = pkg.engine
    c = AC.case(pkg, "n357_sh")
    prior, _ = AC.prior_words(pkg, c.n, 9)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        single = [U.select_attrs(c.rule(pkg, op=op), prior) for op in range(5)]
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(c.splats)
        for op in range(5):
            mask, n_hit, n_set = Mu.select_attrs(c.rule(pkg, op=op), prior)
            want = AC.apply_op(op, prior, c.eval(pkg))
            assert np.array_equal(mask, want) and np.array_equal(mask, single[op][0]) and (n_hit, n_set) == single[op][1:], op
        assert [Mu.stats(r)["n_splats"] for r in range(2)] == [c.n, c.n]
