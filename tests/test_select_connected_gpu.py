"""Selection by connectivity on the GPU (gsr_select_connected): resident splats picked by the connected clump of occupied cells they
lie in.

Everything is BIT-EXACT, so there are no tolerances.  What a mask, the labels, the sizes and the result must hold comes from
gsr_select_connected_eval (the rule on the host) over Engine.read() of the same context -- itself held to the uploaded arrays -- the
breadth-first restatement of connect_cases.py, the numpy restatement of the op and a random prior mask with garbage behind n; never
from the GPU path.  Each case runs under both GSR_OPT_STORAGE_ORDER values."""
import ctypes as C

import numpy as np
import pytest

import connect_cases as CC
import test_move_gpu as M
from helpers import HipBuffers

GSR_E_INVALID = -1
GUARD = 16                   # words on either side of every mask, label array and size array
FILL = 0xA5A5A5A5
ABSENT = 0x5EED5EED          # what an output array holds before the call
NAMES = CC.case_names()
ZERO_TALLY = {"selects": 0, "hit_last": 0, "ms": [0.0] * 4}


def _guarded(words):
    return np.concatenate([np.full(GUARD, FILL, np.uint32), words.astype(np.uint32), np.full(GUARD, FILL, np.uint32)])


def _select_raw(pkg, eng, hb, rule, prior_words, device, seed_words=None, outs=True):
    """gsr_select_connected through the C ABI into a guarded mask that holds prior_words and guarded label and size arrays, all in
    device or all in host memory (the seed words too) -> (words, labels, sizes, result fields, n_hit, n_set); asserts that the guard
    words in front of and behind the three destinations are unchanged, and absent outputs untouched"""
    L, E = pkg.load_library(), pkg.engine
    n = eng.read_info()["n_splats"]
    bufs = [_guarded(prior_words), _guarded(np.full(n, ABSENT, np.uint32)), _guarded(np.full(n, ABSENT, np.uint32))]
    hit, nset, res = C.c_int64(-1), C.c_int64(-1), E.gsr_connect_result()
    seed = None if seed_words is None else np.ascontiguousarray(seed_words, np.uint32)
    if device:
        base = [hb.upload(b) for b in bufs]
        at = [C.c_void_p(b + 4 * GUARD) for b in base]
        dseed = None if seed is None else C.c_void_p(hb.upload(seed))
        rc = L.gsr_select_connected(eng.h, C.byref(rule), dseed, 1, at[0], 1, at[1] if outs else None, at[2] if outs else None, 1,
                                    C.byref(res), C.byref(hit), C.byref(nset))
        out = [hb.download(b, a.shape, np.uint32) for b, a in zip(base, bufs)]
    else:
        out = [b.copy() for b in bufs]
        at = [o.ctypes.data + 4 * GUARD for o in out]
        rc = L.gsr_select_connected(eng.h, C.byref(rule), seed.ctypes.data if seed is not None else None, 0, at[0], 0, at[1] if outs else None,
                                    at[2] if outs else None, 0, C.byref(res), C.byref(hit), C.byref(nset))
    assert rc == 0, L.gsr_last_error()
    for a in out:
        assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all(), "a guard word changed"
    if not outs:
        assert (out[1][GUARD:-GUARD] == ABSENT).all() and (out[2][GUARD:-GUARD] == ABSENT).all()
    return out[0][GUARD:-GUARD], out[1][GUARD:-GUARD], out[2][GUARD:-GUARD], res.fields(), hit.value, nset.value


def _check(pkg, eng, hb, make_rule, want, prior, words, label, ops=range(5), seed=None, memories=(True, False)):
    """every op, into device memory and into host memory; make_rule(op) -> gsr_connect_rule; want = (hit, labels, sizes, fields)"""
    E = pkg.engine
    want_hit, want_lab, want_siz, want_res = want
    seed_words = None if seed is None else E.pack_mask(seed)
    for op in ops:
        m = CC.apply_op(op, prior, want_hit)
        for device in memories:
            got, lab, siz, res, n_hit, n_set = _select_raw(pkg, eng, hb, make_rule(op), words, device, seed_words)
            tag = f"{label} op {CC.OPS[op]} {'device' if device else 'host'} memory"
            assert np.array_equal(got, E.pack_mask(m)), tag               # (pack_mask leaves the bits at and behind n clear)
            assert np.array_equal(lab, want_lab), (tag, "labels", np.flatnonzero(lab != want_lab)[:10])
            assert np.array_equal(siz, want_siz), (tag, "sizes", np.flatnonzero(siz != want_siz)[:10])
            assert res == want_res, (tag, res[:6], want_res[:6])
            assert (n_hit, n_set) == (int(want_hit.sum()), int(m.sum())), (tag, n_hit, n_set)


def _read_equals(R, s):
    """Engine.read() of a context holds the uploaded arrays the rule looks at, bit for bit"""
    assert np.array_equal(R.P.view(np.uint32), np.ascontiguousarray(s.P, np.float32).view(np.uint32))
    assert np.array_equal(R.alpha.view(np.uint32), np.ascontiguousarray(s.alpha, np.float32).view(np.uint32))


# ---- 1. per case and op ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_masks_labels_sizes_and_result_per_case_and_op(pkg, name, order):
    E = pkg.engine
    c = CC.case(pkg, name)
    prior, words = CC.prior_words(pkg, c.n, 40 + c.n)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(c.splats)
            assert U.get_select_connected() == ZERO_TALLY, "a context that never called the verb"
            R = U.read()
            _read_equals(R, c.splats)
            want = c.eval(pkg, cloud=R)
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op), want, prior, words, name)
            sel = U.get_select_connected()
            assert sel["selects"] == 10 and sel["hit_last"] == int(want[0].sum()) and sel["ms"][0] > 0.0 and sel["ms"][2] > 0.0, sel
            assert sel["ms"][3] >= sel["ms"][0] + sel["ms"][2], sel
            assert U.get_select_density()["selects"] == 0 and U.get_select()["selects"] == 0, "a sibling's tally counted a connected select"
            # every reach, with and without a seed clause, into device memory
            for reach in (0, 1, 2):
                seed = CC.seed_of(c, reach, 5)
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=reach), c.eval(pkg, cloud=R, reach=reach), prior, words, f"{name} reach {reach}",
                       ops=(0,), memories=(True,))
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=reach, size=CC.FULL), c.eval(pkg, cloud=R, reach=reach, size=CC.FULL, seed=seed),
                       prior, words, f"{name} reach {reach} seeded", ops=(4,), seed=seed, memories=(True, False) if reach == 1 else (True,))
            # labels_out and sizes_out NULL: the mask and the result alone, the absent arrays untouched
            got, _, _, res, n_hit, _ = _select_raw(pkg, U, hb, c.rule(pkg), words, True, outs=False)
            assert np.array_equal(got, E.pack_mask(want[0])) and res == want[3] and n_hit == int(want[0].sum())
            # the Python door: Engine.select_connected and Engine.select_connected_device
            mask, n_hit, n_set, res, lab, siz = U.select_connected(c.rule(pkg, op=E.SELECT_TOGGLE), prior, outputs=True)
            assert np.array_equal(mask, prior ^ want[0]) and (n_hit, n_set) == (int(want[0].sum()), int((prior ^ want[0]).sum()))
            assert np.array_equal(lab, want[1]) and np.array_equal(siz, want[2]) and res.fields() == want[3]
            mask, n_hit, n_set, res = U.select_connected(c.rule(pkg))
            assert np.array_equal(mask, want[0]) and res.fields() == want[3]
            dm, dl, ds = hb.upload(words), hb.upload(np.zeros(c.n, np.uint32)), hb.upload(np.zeros(c.n, np.uint32))
            n_hit, n_set, res = U.select_connected_device(c.rule(pkg, op=E.SELECT_ADD), dm, labels_ptr=dl, sizes_ptr=ds)
            assert (n_hit, n_set) == (int(want[0].sum()), int((prior | want[0]).sum())) and res.fields() == want[3]
            assert np.array_equal(hb.download(dm, words.shape, np.uint32), E.pack_mask(prior | want[0]))
            assert np.array_equal(hb.download(dl, (c.n,), np.uint32), want[1]) and np.array_equal(hb.download(ds, (c.n,), np.uint32), want[2])
            assert len(U.select_connected_stages()) == 6 and min(U.select_connected_stages()) >= 0.0
    finally:
        hb.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("n257_sh", "n4097_nosh", "faces_r2", "bounds_hit_outside"))
def test_reach_and_ranges(pkg, name):
    """each reach, an empty range, the full range, no alpha floor, HIT_OUTSIDE: one context, the rule changes from call to call"""
    c = CC.case(pkg, name)
    prior, words = CC.prior_words(pkg, c.n, 11)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(c.splats)
            R = U.read()
            for over in CC.variants():
                want = c.eval(pkg, cloud=R, **over)
                assert np.array_equal(want[0], c.restate(**over)[0]), over
                _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, **over), want, prior, words, f"{name} {over}", ops=(0, 4))
    finally:
        hb.free()


# ---- 2. what the special cases are there for, on the device ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reach", (1, 2))
def test_snake_and_comb_join_into_one_root(pkg, reach):
    """the longest parent chains and the most contended root: the structure the restatement finds, not only equality with the eval"""
    for name in (f"snake_r{reach}", f"snake_r{reach}_cut", "comb"):
        c = CC.case(pkg, name)
        over = dict(size=CC.FULL) if name != "comb" else dict(size=CC.FULL, reach=1)
        want = c.restate(**over)
        with pkg.Engine(0) as U:
            U.upload(c.splats)
            mask, n_hit, n_set, res, lab, siz = U.select_connected(c.rule(pkg, **over), outputs=True)
        assert res.fields() == want[3] and np.array_equal(lab, want[1]) and np.array_equal(siz, want[2]) and mask.all(), name
        if name == f"snake_r{reach}":
            assert (res.n_components, res.largest) == (1, 4097) and (lab == 0).all()
        elif name == "comb":
            assert (res.n_components, res.largest) == (2, 4000) and sorted(set(lab)) == sorted((c.marks["a"].min(), c.marks["b"].min()))
        else:
            path = c.marks["path"]
            assert (res.n_components, res.largest) == (2, 2048) and (lab[path[:2048]] == path[:2048].min()).all() and (lab[path[2048:]] == path[2048:].min()).all()


@pytest.mark.gpu
def test_seeds(pkg):
    E = pkg.engine
    c = CC.case(pkg, "clumps")
    clump_of, fl = c.marks["clump_of"], c.marks["floater"]
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(c.splats)
            # one seed bit in one clump selects exactly that clump; seed and size clauses apply together
            seed = np.zeros(c.n, bool)
            seed[np.flatnonzero(clump_of == 3)[2]] = True
            mask, n_hit, n_set, res = U.select_connected(c.rule(pkg, size=CC.FULL), seed=seed)
            assert np.array_equal(mask, clump_of == 3) and (n_hit, res.n_seeded) == (5, 1)
            seed[np.flatnonzero(~fl)[5]] = True
            mask, n_hit, n_set, res = U.select_connected(c.rule(pkg), seed=seed)
            assert np.array_equal(mask, clump_of == 3) and res.n_seeded == 2, "the blob is seeded and too large"
            assert np.array_equal(U.select_connected(c.rule(pkg, size=CC.FULL), seed=seed)[0], (clump_of == 3) | ~fl)
            assert not U.select_connected(c.rule(pkg), seed=np.zeros(c.n, bool))[0].any(), "an empty seed hits nothing"
            # seed bits behind n set to garbage change nothing
            words = E.pack_mask(seed)
            garbage = words.copy()
            garbage[-1] |= np.uint32((0xffffffff << (c.n % 32)) & 0xffffffff)
            assert c.n % 32 and np.array_equal(U.select_connected(c.rule(pkg, size=CC.FULL), seed=garbage)[0], (clump_of == 3) | ~fl)
            # seed == mask with op ADD grows the selection in place, in device and in host memory, and equals the non-aliased call
            picked = np.zeros(c.n, bool)
            picked[np.flatnonzero(clump_of == 11)[0]] = picked[np.flatnonzero(clump_of == 2)[4]] = True
            grown = (clump_of == 11) | (clump_of == 2)
            add = c.rule(pkg, op=E.SELECT_ADD, size=CC.FULL)
            apart, n_hit, n_set, _ = U.select_connected(add, picked, seed=picked)
            assert np.array_equal(apart, grown) and (n_hit, n_set) == (10, 10)
            dm = hb.upload(_guarded(E.pack_mask(picked)))
            assert U.select_connected_device(add, dm + 4 * GUARD, seed_ptr=dm + 4 * GUARD)[:2] == (10, 10)
            assert np.array_equal(hb.download(dm, (2 * GUARD + (c.n + 31) // 32,), np.uint32), _guarded(E.pack_mask(grown)))
            host = _guarded(E.pack_mask(picked))
            at = host.ctypes.data + 4 * GUARD
            rule = add
            assert pkg.load_library().gsr_select_connected(U.h, C.byref(rule), at, 0, at, 0, None, None, 0, None, None, None) == 0
            assert np.array_equal(host, _guarded(E.pack_mask(grown)))
        # a seed on a splat that is not population seeds nothing: below alpha_min, outside, hidden under SKIP_HIDDEN
        c = CC.case(pkg, "n4097_sh")
        s = c.splats
        with pkg.Engine(0) as U:
            U.upload(s)
            siz = c.eval(pkg, size=CC.FULL)[2]
            passes = s.alpha >= np.float32(0.2)
            for label, at in (("below alpha_min", np.flatnonzero(~passes)[:7]), ("outside", np.flatnonzero((siz == 0) & passes)[:7])):
                seed = np.zeros(c.n, bool)
                seed[at] = True
                mask, n_hit, n_set, res = U.select_connected(c.rule(pkg, size=CC.FULL), seed=seed)
                assert at.size == 7 and not mask.any() and (n_hit, res.n_seeded) == (0, 0), label
            hide = np.arange(c.n) % 5 == 1
            U.set_visibility(mask=hide)
            vis, keep = E.visibility_struct((), hide)
            seed = np.zeros(c.n, bool)
            seed[np.flatnonzero(hide & (siz > 0))[:9]] = True
            mask, n_hit, n_set, res, lab, sz = U.select_connected(c.rule(pkg, size=CC.FULL), seed=seed, outputs=True)
            want = c.eval(pkg, size=CC.FULL, seed=seed, vis=vis)
            assert mask.any() and np.array_equal(mask, want[0]) and res.fields() == want[3], "without the flag a hidden splat is population and seeds"
            mask, n_hit, n_set, res, lab, sz = U.select_connected(c.rule(pkg, size=CC.FULL, flags=CC.SKIP_HIDDEN), seed=seed, outputs=True)
            want = c.eval(pkg, size=CC.FULL, seed=seed, vis=vis, flags=CC.SKIP_HIDDEN)
            assert not mask.any() and res.n_seeded == 0 and res.fields() == want[3] and np.array_equal(lab, want[1]) and np.array_equal(sz, want[2])
    finally:
        hb.free()


@pytest.mark.gpu
def test_size_edges(pkg):
    c = CC.case(pkg, "clumps")
    fl = c.marks["floater"]
    none, every = np.zeros(c.n, bool), np.ones(c.n, bool)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        for lo, hi, want in ((5, 5, fl), (6, 3000, ~fl), (5, 2999, fl), (1, 4, none), (5, 3000, every), (3000, 3000, ~fl), (3001, CC.FULL[1], none),
                             (2999, 2999, none), (0, 0, none), (9, 4, none), (0x80000000, 0xffffffff, none)):
            mask, n_hit, n_set, res = U.select_connected(c.rule(pkg, size=(lo, hi)))
            assert np.array_equal(mask, want) and n_hit == int(want.sum()), (lo, hi, n_hit)


# ---- 3. under a visibility in force ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_under_a_visibility(pkg, order):
    """without SKIP_HIDDEN a hidden splat is population with its TRUE alpha (its resident opacity is +0); with it, not at all"""
    E = pkg.engine
    c = CC.case(pkg, "n4097_sh")
    s = c.splats
    volumes = [E.crop_box((0.1, 0.0, 0.0), 0.4)]
    hide = np.arange(c.n) % 4 == 3
    vis_struct, keep = E.visibility_struct(volumes, hide)
    visible = E.visibility_eval(vis_struct, s.P)
    assert (~visible).sum() > 500 and visible.sum() > 500
    prior, words = CC.prior_words(pkg, c.n, 77)
    seed = CC.seed_of(c, 9, 40)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            base = c.eval(pkg, reach=1)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA, hidden_count = U.debug_resident(E.RESIDENT_GEOA), U.get_visibility()[1]
            R = U.read()
            _read_equals(R, s)
            plain = c.eval(pkg, cloud=R, vis=vis_struct, reach=1)
            skip = c.eval(pkg, cloud=R, vis=vis_struct, reach=1, flags=CC.SKIP_HIDDEN)
            assert plain[3] == base[3] and np.array_equal(plain[1], base[1]), "a hidden splat is population with its true alpha"
            assert np.array_equal(skip[0], c.restate(hidden=~visible, reach=1, flags=CC.SKIP_HIDDEN)[0]) and (skip[2][~visible] == 0).all() and skip[3][0] < plain[3][0]
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=1), plain, prior, words, "visibility", ops=(0, 1, 4))
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=1, flags=CC.SKIP_HIDDEN), skip, prior, words, "skip hidden", ops=(0, 2, 3))
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=1, flags=CC.SKIP_HIDDEN),
                   c.eval(pkg, cloud=R, vis=vis_struct, reach=1, flags=CC.SKIP_HIDDEN, seed=seed), prior, words, "skip hidden, seeded", ops=(1,), seed=seed)
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA) and U.get_visibility()[1] == hidden_count
            U.set_visibility()
            _check(pkg, U, hb, lambda op: c.rule(pkg, op=op, reach=1, flags=CC.SKIP_HIDDEN), base, prior, words, "the visibility cleared", ops=(0,))
    finally:
        hb.free()


# ---- 4. the clean-up workflow: select the clumped floaters into a device mask, remove by it -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
def test_clumped_floaters_go_from_the_device_mask(pkg, order):
    E = pkg.engine
    c = CC.case(pkg, "clumps")
    s, fl = c.splats, c.marks["floater"]
    dens = E.select_density_eval(E.density_rule(c.params["cell"], c.params["origin"], reach=1, count=(1, 3)), s.P, s.alpha)
    assert fl.sum() == 85 and not dens[fl].any(), "the existing density rule hits none of the clumped floaters"
    assert np.array_equal(c.restate()[0], fl)
    cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
    blob = s.subset(~fl)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(s)
            dm = hb.upload(np.full((c.n + 31) // 32, 0xffffffff, np.uint32))
            n_hit, n_set, res = U.select_connected_device(c.rule(pkg), dm)
            assert (n_hit, n_set) == (85, 85) and (res.n_components, res.largest, res.comp_hist[2], res.splat_hist[2]) == (18, 3000, 17, 85)
            assert np.array_equal(hb.download(dm, ((c.n + 31) // 32,), np.uint32), E.pack_mask(fl))
            assert U.remove_device(dm) == c.n - 85                        # nothing crossed the link in between
            got, R, frame = M._planes(U), U.read(), U.render(cam).copy()
        M._assert_same_planes(got, M._fresh_planes(pkg, blob, order, True), f"select_connected + remove, order {order}")   # (cluster bounds among them)
        _read_equals(R, blob)
        with pkg.Engine(0) as F:
            F.set_option(E.OPT_STORAGE_ORDER, order)
            F.upload(blob)
            assert np.array_equal(F.render(cam).view(np.uint32), frame.view(np.uint32)), "the frame after the clean-up is a fresh upload's"
    finally:
        hb.free()


# ---- 5. nothing depends on the schedule; nothing is invalidated ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("n65537_sh", "n65537_nosh", "comb", "snake_r2"))
def test_two_calls_agree(pkg, name):
    """follows from exactness; asserted to document that no stored value depends on the order the waves run in"""
    c = CC.case(pkg, name)
    seed = CC.seed_of(c, 5, 50)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        a = U.select_connected(c.rule(pkg, reach=1), seed=seed, outputs=True)
        b = U.select_connected(c.rule(pkg, reach=1), seed=seed, outputs=True)
    assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3] and a[3].fields() == b[3].fields() and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    want = c.eval(pkg, reach=1, seed=seed)
    assert np.array_equal(a[0], want[0]) and a[3].fields() == want[3]


KEPT = ("uploads", "moves", "upload_ms", "move_ms")


@pytest.mark.gpu
def test_a_select_keeps_the_cached_order_and_the_stats(pkg):
    c = CC.case(pkg, "n4097_sh")
    cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        frame = U.render(cam).copy()
        U.render(cam)
        st = U.stats()
        assert st["sorts_skipped"] >= 1 and U.get_select_connected() == ZERO_TALLY
        planes = M._planes(U)
        want = c.eval(pkg)
        assert np.array_equal(U.select_connected(c.rule(pkg))[0], want[0])
        assert U.stats() == st, "a select changed gsr_stats"
        sel = U.get_select_connected()
        assert sel["selects"] == 1 and sel["hit_last"] == int(want[0].sum()) and sel["ms"][3] > 0.0, sel
        again = U.render(cam)
        st2 = U.stats()
        assert st2["sorts_skipped"] == st["sorts_skipped"] + 1, "the select invalidated the cached depth order"
        assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
        for k in KEPT:
            assert st2[k] == st[k], (k, st[k], st2[k])
        M._assert_same_planes(M._planes(U), planes, "a select between frames")


# ---- 6. refusals, with nothing written ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    import test_select_connected as T
    E, L = pkg.engine, pkg.load_library()
    c = CC.case(pkg, "n257_sh")
    words = (c.n + 31) // 32
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room, sroom, lroom, zroom = (hb.upload(np.full(size // 4, FILL, np.uint32)) for _ in range(4))
        host_mask, host_seed = np.full(words + 2, FILL, np.uint32), np.full(words + 2, FILL, np.uint32)
        host_lab, host_siz = np.full(c.n + 2, FILL, np.uint32), np.full(c.n + 2, FILL, np.uint32)
        cnt = [C.c_int64(-7), C.c_int64(-7)]
        res = E.gsr_connect_result()
        res.n_cells = -7
        ok = c.rule(pkg, op=E.SELECT_TOGGLE)
        vp = lambda p: C.c_void_p(p) if p is not None else None

        def call(eng, rule=ok, seed=sroom, sdev=1, mask=room, device=1, labels=lroom, sizes=zroom, odev=1):
            return L.gsr_select_connected(eng.h, C.byref(rule) if rule is not None else None, vp(seed), sdev, vp(mask), device, vp(labels), vp(sizes), odev,
                                          C.byref(res), C.byref(cnt[0]), C.byref(cnt[1]))

        def host_call(eng, rule=ok):
            return call(eng, rule, host_seed.ctypes.data, 0, host_mask.ctypes.data, 0, host_lab.ctypes.data, host_siz.ctypes.data, 0)

        with pkg.Engine(0) as U:
            assert call(U) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()                    # before any upload
            assert host_call(U) == GSR_E_INVALID
            U.upload(c.splats)
            cam = pkg.camera.make_camera(96, 64, sh_order=3, frame=2, near=0.01, far=50.0)
            frame = U.render(cam).copy()
            U.render(cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            cases = {"NULL rule": lambda: call(U, rule=None), "NULL mask": lambda: call(U, mask=None),
                     "pageable mask": lambda: call(U, mask=host_mask.ctypes.data, device=1),
                     "misaligned mask": lambda: call(U, mask=room + 2),
                     "mask past its allocation": lambda: call(U, mask=room + size - (words * 4 - 4)),
                     "pageable seed": lambda: call(U, seed=host_seed.ctypes.data, sdev=1),
                     "misaligned seed": lambda: call(U, seed=sroom + 2),
                     "seed past its allocation": lambda: call(U, seed=sroom + size - (words * 4 - 4)),
                     "pageable labels": lambda: call(U, labels=host_lab.ctypes.data, odev=1),
                     "pageable sizes": lambda: call(U, sizes=host_siz.ctypes.data, odev=1),
                     "misaligned labels": lambda: call(U, labels=lroom + 2),
                     "labels past their allocation": lambda: call(U, labels=lroom + size - (c.n * 4 - 4)),
                     "sizes past their allocation": lambda: call(U, sizes=zroom + size - (c.n * 4 - 4)),
                     "host mask, sizes past their allocation": lambda: call(U, mask=host_mask.ctypes.data, device=0, sizes=zroom + size - 8)}
            for label, r in T._bad_rules(pkg):
                cases[f"{label}, device memory"] = lambda r=r: call(U, rule=r)
                cases[f"{label}, host memory"] = lambda r=r: host_call(U, r)
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_select_connected" in L.gsr_last_error(), label
                assert np.array_equal(U.render(cam), frame), label
                assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
            M._assert_same_planes(M._planes(U), planes, "refusals")
            assert cnt[0].value == -7 and cnt[1].value == -7 and res.n_cells == -7
            for a in (host_mask, host_seed, host_lab, host_siz):
                assert (a == FILL).all()
            for base in (room, sroom, lroom, zroom):
                assert (hb.download(base, (size // 4,), np.uint32) == FILL).all(), "a refused select wrote to device memory"
            assert U.get_select_connected() == ZERO_TALLY, "a refused call launched or counted something"
            assert U.select_connected_stages() == [0.0] * 6
            assert L.gsr_get_select_connected(U.h, None, None, None) == 0   # every pointer may be NULL
            # the seed, the outputs, the result and either count may be NULL
            assert L.gsr_select_connected(U.h, C.byref(ok), None, 0, C.c_void_p(room), 1, None, None, 0, None, None, None) == 0
            assert U.get_select_connected()["selects"] == 1
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
    c = CC.case(pkg, "n65_nosh")
    host = [np.full(2, FILL, np.uint32) for _ in range(4)]
    cnt = [C.c_int64(-7), C.c_int64(-7)]
    res = E.gsr_connect_result()
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        assert U.remove(np.ones(c.n, bool)) == 0
        for op in range(5):
            r = c.rule(pkg, op=op)
            res.n_population = -7
            assert L.gsr_select_connected(U.h, C.byref(r), host[0].ctypes.data, 0, host[1].ctypes.data, 0, host[2].ctypes.data, host[3].ctypes.data, 0,
                                          C.byref(res), C.byref(cnt[0]), C.byref(cnt[1])) == 0
            assert cnt[0].value == 0 and cnt[1].value == 0 and all((h == FILL).all() for h in host)
            assert res.fields() == (0,) * 6 + ((0,) * 32,) * 2
        mask, n_hit, n_set, res, lab, siz = U.select_connected(c.rule(pkg), outputs=True)
        assert mask.shape == lab.shape == siz.shape == (0,) and (n_hit, n_set) == (0, 0)
        assert U.get_select_connected()["selects"] == 0


# ---- 8. several ranks ---------------------------------------------------------------------------------------------------------------------------------
def _multi(pkg, devices):
    E = pkg.engine
    c = CC.case(pkg, "n4097_sh")
    prior, _ = CC.prior_words(pkg, c.n, 9)
    seed = CC.seed_of(c, 2, 30)
    want, seeded = c.eval(pkg), c.eval(pkg, seed=seed, size=CC.FULL)
    with pkg.Engine(0) as U:
        U.upload(c.splats)
        single = [U.select_connected(c.rule(pkg, op=op), prior, outputs=True) for op in range(5)]
    with pkg.MultiEngine(devices, E.TRANSPORT_COPY) as Mu:
        Mu.upload(c.splats)
        for op in range(5):
            mask, n_hit, n_set, res, lab, siz = Mu.select_connected(c.rule(pkg, op=op), prior, outputs=True)
            m = CC.apply_op(op, prior, want[0])
            assert np.array_equal(mask, m) and np.array_equal(mask, single[op][0]) and (n_hit, n_set) == single[op][1:3], op
            assert res.fields() == want[3] == single[op][3].fields() and np.array_equal(lab, want[1]) and np.array_equal(siz, want[2]), op
        mask, n_hit, n_set, res = Mu.select_connected(c.rule(pkg, size=CC.FULL), seed=seed)
        assert np.array_equal(mask, seeded[0]) and res.fields() == seeded[3]
        assert [Mu.stats(r)["n_splats"] for r in range(len(devices))] == [c.n] * len(devices)


@pytest.mark.gpu
def test_multi_select_connected(pkg):
    _multi(pkg, [0, 0])


@pytest.mark.gpu
def test_multi_select_connected_two_gpus(pkg):
    if pkg.load_library().gsr_device_count() < 2:
        pytest.skip("one GPU")
    _multi(pkg, [0, 1])
