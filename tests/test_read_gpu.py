"""Reading the resident cloud back in upload order on the GPU (gsr_read, gsr_read_device).

Everything is BIT-EXACT, there is no tolerance anywhere; the one exception is the header's NaN rule for the device form (a NaN half
becomes a NaN float with unspecified sign and payload).  The expected values are always the HOST arrays the test uploaded and edited,
never anything read from the code under test.  The cloud is test_move_gpu's: 357 splats = five full clusters of 64 and one of 37, with
its helpers; index 15 of the x / y / z rows, which is not resident, is zero in it (scenes.make_scene) and must read back as zero."""
import ctypes as C

import numpy as np
import pytest

import test_move_gpu as M
from helpers import NAN_PATTERNS, HipBuffers, pixels_differ

N = M.N
GSR_E_INVALID = -1
NAMES = ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz")
ROW = {"P": (np.float32, 3), "Cd": (np.uint16, 3), "alpha": (np.float32, 1), "scale": (np.uint16, 3), "orient": (np.uint16, 4),
       "shx": (np.uint16, 16), "shy": (np.uint16, 16), "shz": (np.uint16, 16)}
DEV_WIDTH = {"P": 3, "Cd": 3, "alpha": 1, "scale": 3, "orient": 4}
GUARD = 64                   # bytes on either side of every destination
FILL = 0xA5


def _names(sh):
    return tuple(k for k in NAMES if sh or k not in M.SH3)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]).reshape(len(a), -1)


def _assert_rows(got, want, first, n, names, label):
    """got (a Splats of n rows) holds the rows [first, first + n) of want in every array of names, as bits; the others are None"""
    for k in NAMES:
        g = getattr(got, k)
        if k not in names:
            assert g is None, (label, k)
            continue
        w = getattr(want, k)[first:first + n]
        assert g is not None and g.dtype == w.dtype and len(g) == n, (label, k)
        gb, wb = _bits(g) if n else g.reshape(0, 1), _bits(w) if n else w.reshape(0, 1)
        if not np.array_equal(gb, wb):
            at = tuple(int(v) for v in np.argwhere(gb != wb)[0])
            raise AssertionError(f"{label}: {k} differs in {int((gb != wb).sum())} values, first at row {at[0]} value {at[1]}: "
                                 f"got {int(gb[at]):#x}, want {int(wb[at]):#x}")


def _read_guarded(pkg, eng, first, n, names):
    """gsr_read through the C ABI into destinations that sit between guard bytes -> {name: array}; the guards are checked"""
    E, L = pkg.engine, pkg.load_library()
    r, raw, out = E.gsr_read_arrays(), {}, {}
    for k in names:
        dtype, width = ROW[k]
        nbytes = n * width * np.dtype(dtype).itemsize
        raw[k] = np.full(GUARD + nbytes + GUARD, FILL, np.uint8)
        setattr(r, k, raw[k].ctypes.data + GUARD)
    E._check(L.gsr_read(eng.h, first, n, C.byref(r)))
    for k in names:
        dtype, width = ROW[k]
        body = raw[k][GUARD:len(raw[k]) - GUARD]
        assert (raw[k][:GUARD] == FILL).all() and (raw[k][len(raw[k]) - GUARD:] == FILL).all(), f"{k}: a guard byte changed"
        out[k] = body.view(dtype).reshape((n, width) if width > 1 else (n,)).copy()
    return pkg.scenes.Splats(*[out.get(k) for k in NAMES])


def _half_floats(h):
    """float32 of exactly the binary16 values whose bits h holds"""
    return np.ascontiguousarray(h).view(np.float16).astype(np.float32)


def _sh_floats(s, vpp):
    """(n, vpp, 3) float32: coefficient slot j, channel c of row t = the half at index j of the x / y / z row (slot 15: not resident, 0)"""
    sh = np.stack([_half_floats(s.shx), _half_floats(s.shy), _half_floats(s.shz)], axis=2)      # (n, 16, 3)
    sh[:, 15, :] = 0.0
    return np.ascontiguousarray(sh[:, :vpp, :])


def _device_want(s, first, n, sh, vpp):
    sl = slice(first, first + n)
    want = {"P": s.P[sl], "alpha": s.alpha[sl], "Cd": _half_floats(s.Cd[sl]), "scale": _half_floats(s.scale[sl]), "orient": _half_floats(s.orient[sl])}
    if sh:
        want["sh"] = _sh_floats(s.subset(sl), vpp)
    return {k: np.ascontiguousarray(v, np.float32).reshape(n, -1) for k, v in want.items()}


def _read_device_guarded(eng, hb, first, n, names, vpp=None):
    """read_device into device buffers with guard bytes on either side -> {name: float32 (n, width)}; the guards are checked"""
    width = {k: (3 * vpp if k == "sh" else DEV_WIDTH[k]) for k in names}
    base = {k: hb.upload(np.full(GUARD + n * width[k] * 4 + GUARD, FILL, np.uint8)) for k in names}
    assert eng.read_device({k: base[k] + GUARD for k in names}, first, n, sh_vec3_per_point=vpp if "sh" in names else None) == n
    out = {}
    for k in names:
        raw = hb.download(base[k], (GUARD + n * width[k] * 4 + GUARD,), np.uint8)
        assert (raw[:GUARD] == FILL).all() and (raw[len(raw) - GUARD:] == FILL).all(), f"{k}: a guard byte changed"
        out[k] = raw[GUARD:len(raw) - GUARD].view(np.float32).reshape(n, width[k]).copy()
    return out


def _assert_device(got, want, label, nan_rule=False):
    assert got.keys() == want.keys(), label
    for k in want:
        diff = pixels_differ(got[k], want[k]) if nan_rule else got[k].view(np.uint32) != want[k].view(np.uint32)
        if diff.any():
            at = tuple(int(v) for v in np.argwhere(diff)[0])
            raise AssertionError(f"{label}: {k} differs in {int(diff.sum())} values, first at row {at[0]} value {at[1]}: "
                                 f"got {int(got[k].view(np.uint32)[at]):#x}, want {int(want[k].view(np.uint32)[at]):#x}")


def _order(eng, n=N):
    return eng.debug_storage_order(n).astype(np.int64)


# ---- 1. rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rng", M.RANGES, ids=lambda r: f"{r[0]}+{r[1]}")
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_rows(pkg, sh, order, rng):
    A = M._cloud(pkg, 11, sh=sh)
    if sh:
        assert not A.shx[:, 15].any() and not A.shy[:, 15].any() and not A.shz[:, 15].any()
    first, n = rng
    label = f"[{first}, {first + n}) order {order} sh {sh}"
    names = _names(sh)
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        U.upload(A)
        perm = _order(U)
        if order == 1:
            assert not np.array_equal(perm, np.arange(N)), "the upload is not permuted: the case tests nothing"
        else:
            assert np.array_equal(perm, np.arange(N))
        planes = M._planes(U, sh)
        _assert_rows(U.read(first, n), A, first, n, names, label)
        _assert_rows(_read_guarded(pkg, U, first, n, names), A, first, n, names, label + " (guarded)")
        subsets = [("P",), ("alpha",), ("Cd", "orient"), ("scale",)] + ([M.SH3, ("Cd",) + M.SH3] if sh else [])
        for sub in subsets:
            _assert_rows(U.read(first, n, names=sub), A, first, n, sub, f"{label} names {sub}")
            _assert_rows(_read_guarded(pkg, U, first, n, sub), A, first, n, sub, f"{label} names {sub} (guarded)")
        assert U.get_read() == {**U.get_read(), "reads": 2 + 2 * len(subsets), "rows_last": n}
        M._assert_same_planes(M._planes(U, sh), planes, label + ": a read changed a resident bit")
    if first == 0 and n == N:
        with pkg.Engine(0) as U:                                    # n = None reads to the end
            U.upload(A)
            assert U.read(300).P.shape == (57, 3)
            _assert_rows(U.read(300), A, 300, 57, names, "to the end")


# ---- 2. the device form ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rng", M.RANGES, ids=lambda r: f"{r[0]}+{r[1]}")
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_device_form(pkg, sh, order, rng):
    A = M._cloud(pkg, 11, sh=sh)
    first, n = rng
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
            U.upload(A)
            if order == 1:
                assert not np.array_equal(_order(U), np.arange(N)), "the upload is not permuted: the case tests nothing"
            names = ("P", "Cd", "alpha", "scale", "orient") + (("sh",) if sh else ())
            for vpp in (16, 15, 3) if sh else (None,):
                label = f"[{first}, {first + n}) order {order} sh {sh} vpp {vpp}"
                got = _read_device_guarded(U, hb, first, n, names, vpp)
                _assert_device(got, _device_want(A, first, n, sh, vpp), label)
                assert U.get_read()["rows_last"] == n and U.get_read()["ms"][1] == 0.0
            subsets = [("P",), ("alpha",), ("Cd", "scale")] + ([("sh",), ("sh", "orient")] if sh else [])
            for sub in subsets:
                got = _read_device_guarded(U, hb, first, n, sub, 15)
                want = _device_want(A, first, n, sh, 15)
                _assert_device(got, {k: want[k] for k in sub}, f"[{first}, {first + n}) order {order} sh {sh} names {sub}")
    finally:
        hb.free()


# ---- 3. all binary16 patterns ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_binary16_patterns(pkg):
    n = 1366                                                        # 1366 * 48 = 65568 >= 65536
    A = M._copy(pkg, M._cloud(pkg, 31, n=n))
    h = (np.arange(n * 48, dtype=np.uint32) % 65536).astype(np.uint16).reshape(n, 48)
    assert len(np.unique(h)) == 65536
    A.Cd[:] = h[:, 0:3]
    A.shx[:, :15], A.shy[:, :15], A.shz[:, :15] = h[:, 3:18], h[:, 18:33], h[:, 33:48]
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:                                    # (never rendered)
            U.upload(A)
            assert not np.array_equal(_order(U, n), np.arange(n))
            _assert_rows(U.read(), A, 0, n, NAMES, "all binary16 patterns")
            got = _read_device_guarded(U, hb, 0, n, ("Cd", "sh"), 16)
            want = _device_want(A, 0, n, True, 16)
            # numpy's float16 -> float32: denormals, +-inf and -0 exact; NaN <-> NaN under the NaN rule
            _assert_device(got, {k: want[k] for k in ("Cd", "sh")}, "all binary16 patterns, device form", nan_rule=True)
            allv = np.concatenate([want["Cd"].reshape(-1), want["sh"][:, :45].reshape(-1)])
            assert np.isnan(allv).sum() >= 2 * 1023 and np.isinf(allv).sum() >= 2 and (allv == 0).sum() >= 2
            for k in ("Cd", "sh"):                                  # (everything that is not NaN: the same bits)
                keep = ~np.isnan(want[k])
                assert np.array_equal(got[k].view(np.uint32)[keep], want[k].view(np.uint32)[keep]), k
    finally:
        hb.free()


# ---- 4. raw position and alpha bits ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_raw_position_and_alpha_bits(pkg, sh):
    A = M._copy(pkg, M._cloud(pkg, 11, sh=sh))
    odd = np.concatenate([NAN_PATTERNS.view(np.uint32), np.array([0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000], np.uint32)])
    Pb, ab = A.P.view(np.uint32), A.alpha.view(np.uint32)
    for k, bits in enumerate(odd):
        Pb[5 + 20 * k, k % 3] = bits                                # rows across all six clusters
        ab[9 + 20 * k] = bits
    Pb[350] = odd[:3]
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            assert np.array_equal(_order(U), np.arange(N))          # a box that is not finite means upload order
            _assert_rows(U.read(), A, 0, N, _names(sh), "odd P and alpha bits")
            _assert_rows(_read_guarded(pkg, U, 3, 300, ("P", "alpha")), A, 3, 300, ("P", "alpha"), "odd P and alpha bits, a range")
            got = _read_device_guarded(U, hb, 0, N, ("P", "alpha"))
            _assert_device(got, {"P": A.P.reshape(N, 3), "alpha": A.alpha.reshape(N, 1)}, "odd P and alpha bits, device form")
        B = M._copy(pkg, M._cloud(pkg, 11, sh=sh))                  # ... and the finite ones among them under a Morton order
        Bb, bb = B.P.view(np.uint32), B.alpha.view(np.uint32)
        for k, bits in enumerate(odd[10:]):
            Bb[5 + 20 * k, k % 3] = bits
            bb[9 + 20 * k] = bits
        with pkg.Engine(0) as U:
            U.upload(B)
            assert not np.array_equal(_order(U), np.arange(N))
            _assert_rows(U.read(), B, 0, N, _names(sh), "-0 and denormals, ordered")
            got = _read_device_guarded(U, hb, 0, N, ("P", "alpha"))
            _assert_device(got, {"P": B.P.reshape(N, 3), "alpha": B.alpha.reshape(N, 1)}, "-0 and denormals, ordered, device form")
    finally:
        hb.free()


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_round_trip(pkg, sh, order):
    A = M._cloud(pkg, 11, sh=sh)
    E = pkg.engine
    origin = (0.25, 0.5, -0.125)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A, origin)
            mine = M._planes(U, sh)
            info = U.read_info()
            assert info == {"n_splats": N, "has_sh": sh, "origin": origin}
            back = U.read()
            M._assert_same_planes(M._fresh_planes(pkg, back, order, sh, origin=info["origin"]), mine, f"upload(read()), order {order} sh {sh}")
            names = ("P", "Cd", "alpha", "scale", "orient") + (("sh",) if sh else ())
            width = {**DEV_WIDTH, "sh": 48}
            ptrs = {k: hb.alloc(N * width[k] * 4) for k in names}
            assert U.read_device(ptrs, 0, N, sh_vec3_per_point=16 if sh else None) == N
            with pkg.Engine(0) as F:
                F.set_option(E.OPT_STORAGE_ORDER, order)
                F.upload_device(ptrs, info["origin"], n=N, sh_vec3_per_point=16 if sh else None)
                assert F.read_info() == info
                M._assert_same_planes(M._planes(F, sh), mine, f"upload_device(read_device()), order {order} sh {sh}")
    finally:
        hb.free()


# ---- 6. after an edit chain --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_after_an_edit_chain(pkg, sh):
    A, B, Cc = M._cloud(pkg, 11, sh=sh), M._cloud(pkg, 12, sh=sh), M._cloud(pkg, 13, sh=sh)
    names = _names(sh)
    rng = np.random.default_rng(8)

    def check(U, s, label):
        assert U.read_info()["n_splats"] == s.n, label
        _assert_rows(U.read(), s, 0, s.n, names, label)
        if s.n > 120:
            _assert_rows(U.read(100, 20, names=("P", "Cd")), s, 100, 20, ("P", "Cd"), label + ", a range")

    with pkg.Engine(0) as U:
        U.upload(A)
        check(U, A, "uploaded")
        s = M._copy(pkg, A)
        rows = {k: np.ascontiguousarray(getattr(B, k)[40:240]) for k in names if k != "P"}
        assert U.update_attrs(40, **rows) == 200
        for k, v in rows.items():
            getattr(s, k)[40:240] = v
        check(U, s, "update_attrs")
        s = M._move(pkg, U, s, Cc.P[50:200], 50, Cc, ("Cd", "alpha"))
        check(U, s, "move")
        gone = rng.random(N) < 0.3
        assert U.remove(gone) == int((~gone).sum())
        s = s.subset(~gone)
        check(U, s, "remove")
        new = M._copy(pkg, B.subset(slice(0, 200)))
        s = s.concat(new)
        assert s.n > N and U.add(new) == s.n and U.get_add()["grows"] == 1
        check(U, s, "add past the capacity")
        s = M._move(pkg, U, s, M._mirror(s.P), 0)
        check(U, s, "move again")
        assert U.stats()["uploads"] == 1 and U.stats()["moves"] == 2


# ---- 7. under a visibility ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_under_a_visibility(pkg, sh):
    E = pkg.engine
    A, Cc = M._cloud(pkg, 11, sh=sh), M._cloud(pkg, 13, sh=sh)
    names = _names(sh)
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = np.arange(N) % 3 == 0
    vis = E.visibility_eval(E.visibility_struct(volumes, hide)[0], A.P).astype(bool)
    assert (~vis).sum() > 20 and vis.sum() > 20, "the visibility does not hide some and not all: the case tests nothing"
    assert (~vis & (A.alpha != 0)).any()
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            U.set_visibility(volumes=volumes, mask=hide)
            assert U.get_visibility()[1] == int((~vis).sum())
            geoA = U.debug_resident(E.RESIDENT_GEOA)
            perm = _order(U)
            resident = geoA.view(np.uint32).reshape(N, 4)[:, 3]
            assert np.array_equal(resident, np.where(vis[perm], A.alpha.view(np.uint32)[perm], 0)), "the resident alphas are not the rule's"
            _assert_rows(U.read(), A, 0, N, names, "under a visibility")                 # the TRUE alpha of every splat
            _assert_rows(U.read(50, 150, names=("alpha",)), A, 50, 150, ("alpha",), "under a visibility, alpha alone")
            got = _read_device_guarded(U, hb, 0, N, ("alpha", "P"))
            _assert_device(got, {"alpha": A.alpha.reshape(N, 1), "P": A.P.reshape(N, 3)}, "under a visibility, device form")
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA), "the read changed geoA"
            assert U.get_visibility()[1] == int((~vis).sum())
            # an alpha updated while hidden reads back updated
            first, cnt = 100, 60
            assert (~vis[first:first + cnt]).any() and vis[first:first + cnt].any()
            s = M._copy(pkg, A)
            s.alpha[first:first + cnt] = Cc.alpha[first:first + cnt]
            assert not np.array_equal(s.alpha[first:first + cnt][~vis[first:first + cnt]], A.alpha[first:first + cnt][~vis[first:first + cnt]])
            assert U.update_attrs(first, alpha=s.alpha[first:first + cnt]) == cnt
            _assert_rows(U.read(), s, 0, N, names, "an alpha updated while hidden")
            resident = U.debug_resident(E.RESIDENT_GEOA).view(np.uint32).reshape(N, 4)[:, 3]
            assert np.array_equal(resident, np.where(vis[perm], s.alpha.view(np.uint32)[perm], 0))
            # what is hidden removed: the read equals the survivors
            assert U.remove(hidden=True) == int(vis.sum())
            s = s.subset(vis)
            assert U.read_info()["n_splats"] == s.n
            _assert_rows(U.read(), s, 0, s.n, names, "the hidden removed")
            U.set_visibility()
            _assert_rows(U.read(), s, 0, s.n, names, "the visibility cleared")
    finally:
        hb.free()


# ---- 8. nothing is invalidated -----------------------------------------------------------------------------------------------
KEPT = ("uploads", "moves", "upload_ms", "move_ms")


@pytest.mark.gpu
def test_a_read_keeps_the_cached_order(pkg):
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [2])[0]
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            frame = U.render(cam).copy()
            assert (frame[..., 3] > 0).sum() > 100
            U.render(cam)
            st = U.stats()
            assert st["sorts_skipped"] >= 1
            planes = M._planes(U)
            _assert_rows(U.read(), A, 0, N, NAMES, "between two frames")
            ptrs = {"P": hb.alloc(N * 12), "sh": hb.alloc(N * 180)}
            assert U.read_device(ptrs, 0, N, sh_vec3_per_point=15) == N
            again = U.render(cam)
            st2 = U.stats()
            assert st2["sorts_skipped"] == st["sorts_skipped"] + 1, "the read invalidated the cached depth order"
            assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
            for k in KEPT:
                assert st2[k] == st[k], (k, st[k], st2[k])
            assert U.get_read()["reads"] == 2
            M._assert_same_planes(M._planes(U), planes, "a read between frames")
    finally:
        hb.free()


@pytest.mark.gpu
def test_a_read_keeps_the_depth_horizons(pkg):
    """a cloud that fills the frame, culled against the previous frame's horizons (the scene of test_frame_constants_gpu): the frames
    around a read are culled as those of a context that never reads, and none is repaired"""
    E = pkg.engine
    s = pkg.scenes.make_scene(60000, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
    s.alpha[:] = 0.97
    cams = [pkg.camera.make_camera(200, 120, sh_order=3, frame=180 + k, step_deg=0.25, distance=2.2) for k in range(6)]

    def run(read):
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_OCCLUSION_CULL, 2)
            U.upload(s)
            out, stats = [], []
            for k, c in enumerate(cams):
                if read and k == 3:
                    _assert_rows(U.read(names=("P", "alpha", "Cd")), s, 0, s.n, ("P", "alpha", "Cd"), "between culled frames")
                out.append(U.render(c).copy())
                stats.append(U.stats())
            return out, stats

    want, st0 = run(False)
    got, st1 = run(True)
    print("frames_culled", [t["frames_culled"] for t in st0], [t["frames_culled"] for t in st1], "repaired", st0[-1]["frames_repaired"], st1[-1]["frames_repaired"])
    assert st0[2]["frames_culled"] >= 1, "no frame was culled before the read: the case tests nothing"
    assert [t["frames_culled"] for t in st1] == [t["frames_culled"] for t in st0]
    assert st1[-1]["frames_culled"] > st1[2]["frames_culled"], "culling stopped at the read"
    assert st1[-1]["frames_repaired"] == 0 and st0[-1]["frames_repaired"] == 0
    for k in KEPT:
        assert st1[-1][k] == st1[0][k], k
    for k in range(len(cams)):
        assert np.array_equal(got[k], want[k]), k


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_and_the_destinations_alone(pkg):
    A = M._cloud(pkg, 11)
    E, L = pkg.engine, pkg.load_library()
    cam = M._cams(pkg, [2])[0]
    hb = HipBuffers()
    try:
        size = 2 << 20                                              # (a multiple of any granularity the allocator may round to)
        room = hb.upload(np.full(size, FILL, np.uint8))
        host = {k: np.full(N * ROW[k][1] * np.dtype(ROW[k][0]).itemsize, FILL, np.uint8).view(ROW[k][0]).reshape(N, ROW[k][1]) for k in NAMES}

        def arrays(**kw):
            r = E.gsr_read_arrays()
            for k, v in kw.items():
                setattr(r, k, v.ctypes.data)
            return r

        def dev(vpp=15, reserved=0, **kw):
            d = E.gsr_device_out()
            for k, v in kw.items():
                setattr(d, k, v)
            d.sh_vec3_per_point, d.reserved_ = vpp, reserved
            return d

        everything = arrays(**host)
        with pkg.Engine(0) as U:
            assert L.gsr_read(U.h, 0, 0, C.byref(everything)) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()      # before any upload
            assert L.gsr_read_device(U.h, 0, 1, C.byref(dev(P=room))) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()
            assert L.gsr_read_info(U.h, None, None, None) == GSR_E_INVALID
            with pytest.raises(E.GsrError):
                U.read()
            U.upload(A)
            frame = U.render(cam).copy()
            U.render(cam)
            planes, skipped = M._planes(U), U.stats()["sorts_skipped"]
            short = room + size - (N * 12 - 4)                      # one word short of the end of its allocation
            pageable = np.zeros((N, 3), np.float32)
            for label, ptr, nbytes in (("pageable", pageable.ctypes.data, N * 12), ("misaligned", room + 2, N * 12), ("short", short, N * 12)):
                assert not U.check_device_source(ptr, nbytes), label     # (the pure query first: no verb is handed a pointer it would take)
            cases = {
                "first < 0": lambda: L.gsr_read(U.h, -1, 1, C.byref(everything)),
                "n < 0": lambda: L.gsr_read(U.h, 0, -1, C.byref(everything)),
                "past the end": lambda: L.gsr_read(U.h, N - 1, 2, C.byref(everything)),
                "first past the end": lambda: L.gsr_read(U.h, N + 1, 0, C.byref(everything)),
                "a huge n": lambda: L.gsr_read(U.h, 1, 2 ** 63 - 1, C.byref(everything)),
                "NULL struct": lambda: L.gsr_read(U.h, 0, N, None),
                "one SH array of three": lambda: L.gsr_read(U.h, 0, N, C.byref(arrays(P=host["P"], shy=host["shy"]))),
                "two SH arrays of three": lambda: L.gsr_read(U.h, 0, N, C.byref(arrays(shx=host["shx"], shz=host["shz"]))),
                "device: past the end": lambda: L.gsr_read_device(U.h, 1, N, C.byref(dev(P=room))),
                "device: n < 0": lambda: L.gsr_read_device(U.h, 0, -1, C.byref(dev(P=room))),
                "device: NULL struct": lambda: L.gsr_read_device(U.h, 0, N, None),
                "device: vpp 0": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(vpp=0, sh=room))),
                "device: vpp 17": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(vpp=17, sh=room))),
                "device: reserved_ = 1": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(reserved=1, P=room))),
                "device: pageable host memory": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(P=pageable.ctypes.data))),
                "device: misaligned by 2 bytes": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(alpha=room, P=room + 4096 + 2))),
                "device: 4 bytes short of its rows": lambda: L.gsr_read_device(U.h, 0, N, C.byref(dev(alpha=room, P=short))),
            }
            reads = U.get_read()["reads"]
            for n_case, (label, fn) in enumerate(cases.items()):
                assert fn() == GSR_E_INVALID, label
                assert b"gsr_read" in L.gsr_last_error(), label
                M._assert_same_planes(M._planes(U), planes, label)
                assert np.array_equal(U.render(cam), frame), label
                assert U.stats()["sorts_skipped"] == skipped + 1 + n_case, f"{label}: the cached order did not survive the refusal"
            assert all((a.view(np.uint8) == FILL).all() for a in host.values()), "a refused read wrote to a host destination"
            assert not pageable.any()
            assert (hb.download(room, (size,), np.uint8) == FILL).all(), "a refused read wrote to a device destination"
            # nothing asked for, and no rows: GSR_OK, nothing happens and nothing is counted
            assert L.gsr_read(U.h, 0, N, C.byref(arrays())) == 0
            assert L.gsr_read(U.h, 17, 0, C.byref(everything)) == 0 and L.gsr_read(U.h, N, 0, C.byref(everything)) == 0
            assert L.gsr_read_device(U.h, 0, N, C.byref(dev())) == 0 and L.gsr_read_device(U.h, 0, 0, C.byref(dev(P=room))) == 0
            assert U.get_read() == {"reads": reads, "rows_last": 0, "ms": [0.0] * 4} and reads == 0
            assert all((a.view(np.uint8) == FILL).all() for a in host.values()), "a read of nothing wrote"
            assert L.gsr_get_read(U.h, None, None, None) == 0       # every pointer may be NULL
            assert U.read(N, 0).P.shape == (0, 3)
            # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
            assert L.gsr_upload_begin(U.h, N, 1, None) == 0
            assert L.gsr_read(U.h, 0, 1, C.byref(everything)) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_read_device(U.h, 0, 1, C.byref(dev(P=room))) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
            assert L.gsr_read_info(U.h, None, None, None) == GSR_E_INVALID
            assert L.gsr_upload_abort(U.h) == 0
            assert all((a.view(np.uint8) == FILL).all() for a in host.values())
            # the empty cloud reads 0 rows
            U.upload(A)
            assert U.remove(np.ones(N, bool)) == 0
            assert U.read_info()["n_splats"] == 0 and U.read().P.shape == (0, 3) and U.read().shx.shape == (0, 16)
            assert L.gsr_read(U.h, 0, 1, C.byref(everything)) == GSR_E_INVALID
            assert U.get_read()["reads"] == 0
        with pkg.Engine(0) as V:                                    # SH destinations for a cloud without SH
            V.upload(M._cloud(pkg, 11, sh=False))
            planes = M._planes(V, sh=False)
            assert L.gsr_read(V.h, 0, N, C.byref(everything)) == GSR_E_INVALID and b"without SH" in L.gsr_last_error()
            assert L.gsr_read_device(V.h, 0, N, C.byref(dev(sh=room))) == GSR_E_INVALID and b"without SH" in L.gsr_last_error()
            with pytest.raises(E.GsrError):
                V.read(names=("P", "shx", "shy", "shz"))
            M._assert_same_planes(M._planes(V, sh=False), planes, "SH destinations without SH")
            assert V.read().shx is None and V.get_read()["reads"] == 1
            assert all((a.view(np.uint8) == FILL).all() for a in host.values())
    finally:
        hb.free()


# ---- 10. several ranks -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_read(pkg):
    A = M._cloud(pkg, 11)
    E = pkg.engine
    gone = np.random.default_rng(3).random(N) < 0.3
    s = A.subset(~gone)
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as Mu:
        Mu.upload(A)
        Mu.render(M._cams(pkg, [1])[0])
        assert Mu.remove(gone) == s.n
        _assert_rows(Mu.read(), s, 0, s.n, NAMES, "MultiEngine.read after a remove")
        _assert_rows(Mu.read(10, 100, names=("P", "scale")), s, 10, 100, ("P", "scale"), "MultiEngine.read, a range")
        assert [Mu.stats(r)["n_splats"] for r in range(2)] == [s.n, s.n]
