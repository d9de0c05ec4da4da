"""Device sources on the GPU (gsr_upload_append_device, gsr_update_device, gsr_move_device): float32 arrays in device memory.

Everything is BIT-EXACT, so there are no tolerances.  Every comparison is between a context U -- upload of cloud A, then a device-source
verb fed FLOAT rows from raw device buffers -- and a fresh context F that was uploaded the same rows quantised on the host with
gsplat_quantize_half: the resident planes, the storage order and every later frame are the same bytes.

The cloud, the ranges and the helpers are those of test_attr_update_gpu / test_move_gpu: 357 splats = five full clusters of 64 and one
of 37; frames of 96 x 64 on the parity orbit.  The float sources are fresh float32 draws, not halves widened to float, and every test
that quantises asserts so (_rounds): otherwise the rounding would not be under test.  No verb is ever handed a pointer that could fault
if its check were missing: pageable-host and past-the-end pointers go to check_device_source, a pure query, only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import test_attr_update_gpu as T
import test_move_gpu as M
from helpers import HipBuffers

N, W, H = T.N, T.W, T.H
RANGES = T.RANGES
GSR_E_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH3 = T.SH3
DEV_ATTRS = ("Cd", "alpha", "scale", "orient", "sh")
FLOATS_PER_ROW = {"P": 3, "Cd": 3, "alpha": 1, "scale": 3, "orient": 4}


# ---- float sources and their host-quantised twins ----------------------------------------------------------------------------
def _floats(seed, n=N, vpp=15):
    """float32 point attributes as a trainer holds them, activations applied: fresh draws, nothing pre-rounded to a half"""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 1.0, (n, 4))
    f = dict(P=rng.uniform(-1.0, 1.0, (n, 3)), Cd=rng.uniform(0.0, 1.0, (n, 3)), alpha=rng.uniform(0.05, 1.0, n),
             scale=np.exp(rng.uniform(-3.5, -2.0, (n, 3))), orient=q / np.linalg.norm(q, axis=1, keepdims=True),
             sh=rng.normal(0.0, 0.1, (n, vpp, 3)))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in f.items()}


def _widen(h):
    return h.view(np.float16).astype(np.float32)


def _rounds(pkg, a):
    """the source is not already a half: quantising it changes it"""
    a = np.ascontiguousarray(a, np.float32)
    assert not np.array_equal(a, _widen(pkg.engine.quantize_half(a))), "the float source holds halves only: the rounding is not under test"


def _sh_rows(pkg, sh):
    """(n, vpp, 3) float32 -> shx, shy, shz (n, 16) halves: coefficient j in slot j, the slots behind vpp zero"""
    n, vpp = sh.shape[0], sh.shape[1]
    q = pkg.engine.quantize_half(sh)
    out = [np.zeros((n, 16), np.uint16) for _ in range(3)]
    for ch in range(3):
        out[ch][:, :vpp] = q[:, :, ch]
    return out


def _halves(pkg, rows):
    """float rows keyed by DEV_ATTRS -> the rows of the half layout (test_attr_update_gpu.ATTRS), quantised on the host"""
    out = {}
    for k, v in rows.items():
        if k == "sh":
            out["shx"], out["shy"], out["shz"] = _sh_rows(pkg, v)
        elif k in ("alpha", "P"):
            out[k] = v
        else:
            out[k] = pkg.engine.quantize_half(v)
    return out


def _dev_names(names):
    return tuple(k for k in DEV_ATTRS if k in names or (k == "sh" and any(s in names for s in SH3)))


def _rows(pkg, f, names, first, n):
    rows = {k: np.ascontiguousarray(f[k][first:first + n]) for k in names}
    for k, v in rows.items():
        if k not in ("alpha", "P"):
            _rounds(pkg, v)
    return rows


def _apply(pkg, s, rows, first, n):
    out = T._copy(pkg, s)
    for k, v in _halves(pkg, rows).items():
        getattr(out, k)[first:first + n] = v
    return out


def _edit(pkg, hb, eng, s, f, names, first, n):
    """update the engine's splats [first, first + n) from DEVICE float rows of f; returns the edited cloud, quantised on the host"""
    rows = _rows(pkg, f, names, first, n)
    ptrs = {k: hb.upload(v) for k, v in rows.items()}
    vpp = rows["sh"].shape[1] if "sh" in rows else None
    assert eng.update_attrs_device(first, n=n, sh_vec3_per_point=vpp, **ptrs) == n
    return _apply(pkg, s, rows, first, n)


def _move(pkg, hb, eng, s, f, names, first, n, origin=None):
    rows = _rows(pkg, f, ("P",) + tuple(names), first, n)
    ptrs = {k: hb.upload(v) for k, v in rows.items()}
    vpp = rows["sh"].shape[1] if "sh" in rows else None
    assert eng.move_device(first, ptrs.pop("P"), origin=origin, n=n, sh_vec3_per_point=vpp, **ptrs) == n
    return _apply(pkg, s, rows, first, n)


@pytest.fixture(scope="module")
def clouds(pkg):
    """A (what is uploaded, halves), its twin without SH, and the float cloud the new values come from"""
    return T._cloud(pkg, 11), T._cloud(pkg, 11, sh=False), _floats(21)


@pytest.fixture()
def hb():
    b = HipBuffers()
    yield b
    b.free()


# ---- 1. update: resident bits --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("subset", list(T.SUBSETS))
def test_update_resident_bits(pkg, clouds, hb, subset, order):
    A, _, f = clouds
    E = pkg.engine
    names = _dev_names(T.SUBSETS[subset])
    for first, n in RANGES:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = T._planes(U)
            edited = _edit(pkg, hb, U, A, f, names, first, n)
            got = T._planes(U)
            st = U.stats()
            assert st["uploads"] == 1 and st["upload_ms"][4] == 0.0      # not an upload, and nothing crossed the link
        T._assert_same_planes(got, T._fresh_planes(pkg, edited, order), f"{subset} [{first}, {first + n}) order {order}")
        assert any(not np.array_equal(before[k], got[k]) for k in got), "the update changed nothing: the case tests nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("subset", ("alpha", "Cd", "scale+orient"))
def test_update_resident_bits_without_sh(pkg, clouds, hb, subset, order):
    _, A, f = clouds
    E = pkg.engine
    for first, n in RANGES:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            before = T._planes(U, sh=False)
            edited = _edit(pkg, hb, U, A, f, _dev_names(T.SUBSETS[subset]), first, n)
            got = T._planes(U, sh=False)
            assert U.stats()["upload_ms"][4] == 0.0
        T._assert_same_planes(got, T._fresh_planes(pkg, edited, order, sh=False), f"no SH, {subset} [{first}, {first + n}) order {order}")
        assert any(not np.array_equal(before[k], got[k]) for k in got)


# ---- 2. SH width ---------------------------------------------------------------------------------------------------------------
def _colour_halves(planes):
    """the 48 colour halves of every slot, (n, 48): Cd.rgb, sh1.rgb, ..., sh15.rgb"""
    col = T._live(planes)["col"]
    return np.ascontiguousarray(col.reshape(6, -1, 16).transpose(1, 0, 2)).view(np.uint16).reshape(-1, 48)


@pytest.mark.gpu
@pytest.mark.parametrize("vpp", (1, 15, 16))
def test_sh_width(pkg, clouds, hb, vpp):
    A = clouds[0]
    f = _floats(22, vpp=vpp)
    for first, n in ((0, N), (50, 150)):
        with pkg.Engine(0) as U:
            U.upload(A)
            edited = _edit(pkg, hb, U, A, f, ("sh",), first, n)
            got = T._planes(U)
            slots = np.isin(U.debug_storage_order(N), np.arange(first, first + n))
        T._assert_same_planes(got, T._fresh_planes(pkg, edited), f"vpp {vpp} [{first}, {first + n})")
        h = _colour_halves(got)[slots]
        assert h.shape == (n, 48) and h[:, 3:3 * (min(vpp, 15) + 1)].any()
        assert not h[:, 3 * (min(vpp, 15) + 1):].any(), "a slot behind sh_vec3_per_point is not a zero half"


# ---- 3. quantisation edges -----------------------------------------------------------------------------------------------------
EDGES = np.array([1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11,      # exact ties between two halves: to the even one
                  1e-6, -3e-7,                                    # half subnormals
                  0.0, -0.0, 65504.0, 65519.99], np.float32)      # signed zeros; the largest half; the last value that does not overflow
OVERFLOW = np.array([65520.0, np.inf, -np.inf], np.float32)       # the first value that overflows; infinities (Cd and sh only)


@pytest.mark.gpu
def test_quantisation_edges(pkg, clouds, hb):
    A, _, f = clouds
    with np.errstate(over="ignore"):
        both = np.concatenate([EDGES, OVERFLOW])
        want_bits = both.astype(np.float16).view(np.uint16)
    assert np.array_equal(pkg.engine.quantize_half(both), want_bits)
    assert want_bits[:2].tolist() == [0x3c00, 0x3c02] and want_bits[6:].tolist() == [0x7bff, 0x7bff, 0x7c00, 0x7c00, 0xfc00]
    g = {k: v.copy() for k, v in f.items()}
    ne = len(both)
    g["Cd"].reshape(-1)[:ne] = both
    g["Cd"].reshape(-1)[-ne:] = both[::-1]
    g["sh"].reshape(-1)[:ne] = both                                # (splat 0: coefficients 0..3)
    g["sh"][N - 1, 11:15, :].reshape(-1)[:ne] = both[::-1]          # (the last splat of the partial cluster: its last coefficients)
    g["scale"].reshape(-1)[3:3 + len(EDGES)] = EDGES                # (splats 1..3)
    g["scale"][200] = (65504.0, 1e-6, -0.0)
    for order in (1, 0):
        with pkg.Engine(0) as U:
            U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
            U.upload(A)
            edited = _edit(pkg, hb, U, A, g, ("Cd", "scale", "sh"), 0, N)
            got = T._planes(U)
        T._assert_same_planes(got, T._fresh_planes(pkg, edited, order), f"quantisation edges, order {order}")


# ---- 4. move: resident bits and the storage order ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("attrs", (False, True))
def test_move_resident_bits(pkg, clouds, hb, attrs, order):
    A, _, f = clouds
    E = pkg.engine
    names = DEV_ATTRS if attrs else ()
    for first, n in RANGES:
        for origin in (None, (0.25, -0.5, 0.125)):
            label = f"move [{first}, {first + n}) attrs {attrs} order {order} origin {origin}"
            with pkg.Engine(0) as U:
                U.set_option(E.OPT_STORAGE_ORDER, order)
                U.upload(A)
                before = M._planes(U)
                edited = _move(pkg, hb, U, A, f, names, first, n, origin)
                got = M._planes(U)
                st = U.stats()
                assert st["uploads"] == 1 and st["moves"] == 1 and st["move_ms"][0] == 0.0, label
            M._assert_same_planes(got, M._fresh_planes(pkg, edited, order, origin=origin or (0.0, 0.0, 0.0)), label)
            assert not np.array_equal(before["geoA"], got["geoA"]), "the move changed nothing: the case tests nothing"
            if order == 1 and n == N:
                assert not np.array_equal(before["order"], got["order"]), "the storage order did not change: the case tests nothing"


# ---- 5. upload -----------------------------------------------------------------------------------------------------------------
def _raw_planes(pkg, attrs):
    """the planes of a fresh context after upload_raw of the same float arrays from the HOST"""
    raw = {("sh_coefficients" if k == "sh" else k): v for k, v in attrs.items()}
    with pkg.Engine(0) as F:
        F.upload_raw(raw)
        return M._planes(F, sh="sh" in attrs)


@pytest.mark.gpu
@pytest.mark.parametrize("missing", (None, "Cd", "alpha", "scale", "orient", "sh"))
def test_upload_device_matches_upload_raw(pkg, clouds, hb, missing):
    f = clouds[2]
    attrs = {k: v for k, v in f.items() if k != missing}
    for k in ("Cd", "scale", "orient", "sh"):
        if k in attrs:
            _rounds(pkg, attrs[k])
    ptrs = {k: hb.upload(v) for k, v in attrs.items()}
    with pkg.Engine(0) as U:
        assert U.upload_device(ptrs, n=N, sh_vec3_per_point=15 if "sh" in attrs else None) == N
        got = M._planes(U, sh="sh" in attrs)
        assert U.stats()["uploads"] == 1
    M._assert_same_planes(got, _raw_planes(pkg, attrs), f"upload_device without {missing}")


@pytest.mark.gpu
def test_upload_mixes_host_and_device_entries(pkg, clouds, hb):
    """one upload of two entries: the first appended from the host (halves), the second from device memory (floats)"""
    A, _, f = clouds
    E = pkg.engine
    L = pkg.load_library()
    cut = 200
    a = E._Arrays(A.subset(slice(0, cut)))
    rows = _rows(pkg, f, ("P",) + DEV_ATTRS, cut, N - cut)
    d, n, _ = E.device_attrs_struct(n=N - cut, sh_vec3_per_point=15, **{k: hb.upload(v) for k, v in rows.items()})
    with pkg.Engine(0) as U:
        E._check(L.gsr_upload_begin(U.h, N, 1, None))
        E._check(L.gsr_upload_append(U.h, a.n, *a.ptrs()))
        E._check(L.gsr_upload_append_device(U.h, n, C.byref(d)))
        E._check(L.gsr_upload_end(U.h))
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, _apply(pkg, A, rows, cut, N - cut)), "host entry + device entry")


# ---- 6. frames -----------------------------------------------------------------------------------------------------------------
def _option_sets(E):
    return {"defaults": (), "cull 0": ((E.OPT_OCCLUSION_CULL, 0),), "cull 3": ((E.OPT_OCCLUSION_CULL, 3),),
            "lazy 2, two in flight": ((E.OPT_LAZY_COLOUR, 2), (E.OPT_FRAMES_IN_FLIGHT, 2))}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("defaults", "cull 0", "cull 3", "lazy 2, two in flight"))
def test_frames_after_update_and_move(pkg, clouds, hb, mode):
    A, _, f = clouds
    opts = _option_sets(pkg.engine)[mode]
    cams = T._cams(pkg, range(9))
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        U.upload(A)
        for c in cams[:3]:
            U.render(c)
        s1 = _edit(pkg, hb, U, A, f, DEV_ATTRS, 0, N)
        got1 = [U.render(c).copy() for c in cams[3:6]]
        s2 = _move(pkg, hb, U, s1, f, (), 0, N)
        got2 = [U.render(c).copy() for c in cams[6:9]]
    for label, got, edited, stale, cs in (("update", got1, s1, A, cams[3:6]), ("move", got2, s2, s1, cams[6:9])):
        want = T._fresh_frames(pkg, edited, cs, opts)
        old = T._fresh_frames(pkg, stale, cs, opts)
        for k in range(3):
            assert not np.array_equal(want[k], old[k]), f"{mode}, {label}: the edit does not show in frame {k}: the case tests nothing"
            assert np.array_equal(got[k], want[k]), (f"{mode}, {label}: frame {k} differs from a fresh upload's in "
                                                     f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
def test_colour_only_edit_keeps_policies_and_horizons(pkg, clouds, hb):
    A, _, f = clouds
    E = pkg.engine
    cams = T._cams(pkg, range(5))
    with pkg.Engine(0) as U:
        U.set_option(E.OPT_OCCLUSION_CULL, 2)
        U.upload(A)
        for c in cams[:3]:
            U.render(c)
        st = U.stats()
        p0, h0 = U.policy_state(), U.debug_horizons(st["tiles_x"], st["tiles_y"]).view(np.uint32).copy()
        assert p0["vis_unculled"] > 0
        s1 = _edit(pkg, hb, U, A, f, ("Cd", "sh"), 0, N)
        assert U.policy_state() == p0
        assert np.array_equal(U.debug_horizons(st["tiles_x"], st["tiles_y"]).view(np.uint32), h0)
        got = [U.render(c).copy() for c in cams[3:]]
        want = T._fresh_frames(pkg, s1, cams[3:], ((E.OPT_OCCLUSION_CULL, 2),))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        _edit(pkg, hb, U, s1, f, ("alpha",), 0, N)                  # ... and anything else is a new cloud to them
        assert U.policy_state()["vis_unculled"] == 0


# ---- 7. the pointer check, and the refusals ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_check_device_source(pkg, hb):
    size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
    p = hb.alloc(size)
    host = np.zeros(1024, np.float32)
    with pkg.Engine(0) as U:
        assert U.check_device_source(p, size) and U.check_device_source(p + 1024, size - 1024) and U.check_device_source(p + 1024, 16)
        assert not U.check_device_source(p + 2, 16)                 # not 4-byte aligned
        assert not U.check_device_source(host.ctypes.data, host.nbytes)          # pageable host memory
        assert b"gsr_debug_check_device_source" in pkg.load_library().gsr_last_error()
        assert not U.check_device_source(p, size + 1) and not U.check_device_source(p + 1024, size - 1024 + 1)
        assert U.check_device_source(p, size)                       # (a failed query leaves nothing behind)


@pytest.mark.gpu
def test_refusals_leave_the_context_alone(pkg, clouds, hb):
    A, Anosh, f = clouds
    E = pkg.engine
    L = pkg.load_library()
    roomy = hb.alloc(N * 17 * 12 + 64)                              # room for any array of N rows, 17 vec3 per point included
    P = hb.upload(f["P"])

    def attrs(**kw):
        kw.setdefault("n", N)
        return E.device_attrs_struct(**kw)[0]

    def update(eng, first, n, a):
        return L.gsr_update_device(eng.h, first, n, C.byref(a))

    def move(eng, first, n, a):
        return L.gsr_move_device(eng.h, first, n, None, C.byref(a))

    with pkg.Engine(0) as U:
        assert update(U, 0, 1, attrs(Cd=roomy)) == GSR_E_INVALID    # before any upload
        assert b"no geometry" in L.gsr_last_error()
        assert move(U, 0, 1, attrs(P=P)) == GSR_E_INVALID and b"no geometry" in L.gsr_last_error()
        U.upload(A)
        planes = M._planes(U)
        cases = {
            "update: NULL struct": lambda: L.gsr_update_device(U.h, 0, 1, None),
            "move: NULL struct": lambda: L.gsr_move_device(U.h, 0, 1, None, None),
            "update: misaligned": lambda: update(U, 0, N, attrs(Cd=roomy + 2)),
            "move: misaligned P": lambda: move(U, 0, N, attrs(P=roomy + 2)),
            "move: misaligned attribute": lambda: move(U, 0, N, attrs(P=P, alpha=roomy + 1)),
            "update: P given": lambda: update(U, 0, N, attrs(P=P, Cd=roomy)),
            "move: no P": lambda: move(U, 0, N, attrs(Cd=roomy)),
            "update: vpp 0": lambda: update(U, 0, N, attrs(sh=roomy, sh_vec3_per_point=0)),
            "update: vpp 17": lambda: update(U, 0, N, attrs(sh=roomy, sh_vec3_per_point=17)),
            "move: vpp 17": lambda: move(U, 0, N, attrs(P=P, sh=roomy, sh_vec3_per_point=17)),
            "update: first < 0": lambda: update(U, -1, 2, attrs(Cd=roomy)),
            "update: n < 0": lambda: update(U, 0, -1, attrs(Cd=roomy)),
            "update: beyond the cloud": lambda: update(U, N - 1, 2, attrs(Cd=roomy)),
            "move: beyond the cloud": lambda: move(U, N - 1, 2, attrs(P=P)),
            "move: first beyond the cloud": lambda: move(U, N + 1, 0, attrs(P=P)),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            M._assert_same_planes(M._planes(U), planes, label)
        # nothing to do is not an error, and does nothing
        assert update(U, 0, 0, attrs(Cd=roomy)) == 0 and update(U, 5, 10, attrs()) == 0 and move(U, 5, 0, attrs(P=P)) == 0
        M._assert_same_planes(M._planes(U), planes, "empty calls")
        assert U.stats()["moves"] == 0
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: the refusal and its text are what can be held)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        assert update(U, 0, 1, attrs(Cd=roomy)) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
        assert move(U, 0, 1, attrs(P=P)) == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error()
        app = lambda n, a: L.gsr_upload_append_device(U.h, n, C.byref(a))
        for label, rc in {"append: no P": app(N, attrs(Cd=roomy, sh=roomy, sh_vec3_per_point=15)),
                          "append: misaligned": app(N, attrs(P=P, Cd=roomy + 2, sh=roomy, sh_vec3_per_point=15)),
                          "append: SH announced, none given": app(N, attrs(P=P)),
                          "append: vpp 17": app(N, attrs(P=P, sh=roomy, sh_vec3_per_point=17)),
                          "append: vpp 0": app(N, attrs(P=P, sh=roomy, sh_vec3_per_point=0)),
                          "append: too many": app(N + 1, attrs(P=P, sh=roomy, sh_vec3_per_point=15)),
                          "append: NULL struct": L.gsr_upload_append_device(U.h, N, None)}.items():
            assert rc == GSR_E_INVALID, label
        assert L.gsr_upload_abort(U.h) == 0
        assert L.gsr_upload_append_device(U.h, 1, C.byref(attrs(P=P))) == GSR_E_INVALID        # no upload in progress
        # (the refused appends wrote nothing: a complete upload afterwards is the fresh upload)
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "after the refused appends")
    with pkg.Engine(0) as V:                                        # sh for a cloud uploaded without SH
        V.upload(Anosh)
        planes = M._planes(V, sh=False)
        assert update(V, 0, N, attrs(sh=roomy, sh_vec3_per_point=15)) == GSR_E_INVALID
        assert update(V, 0, N, attrs(Cd=roomy, sh=roomy, sh_vec3_per_point=15)) == GSR_E_INVALID
        assert move(V, 0, N, attrs(P=P, sh=roomy, sh_vec3_per_point=15)) == GSR_E_INVALID
        M._assert_same_planes(M._planes(V, sh=False), planes, "sh without SH")
        assert L.gsr_upload_begin(V.h, N, 0, None) == 0              # ... and an upload that announced none
        assert L.gsr_upload_append_device(V.h, N, C.byref(attrs(P=P, sh=roomy, sh_vec3_per_point=15))) == GSR_E_INVALID
        assert L.gsr_upload_abort(V.h) == 0


# ---- 7b. pinned host memory is a source too --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pinned_host_sources(pkg, clouds, hb):
    """hipHostMalloc memory passes the check and serves all three verbs: the kernels read it through the same pointer"""
    A, _, f = clouds
    pinned = []

    def pin(a):
        p = C.c_void_p()
        assert hb.hip.hipHostMalloc(C.byref(p), C.c_size_t(a.nbytes), 0) == 0
        pinned.append(p)
        C.memmove(p.value, a.ctypes.data, a.nbytes)
        return p.value

    try:
        rows = _rows(pkg, f, ("P",) + DEV_ATTRS, 0, N)
        ptrs = {k: pin(v) for k, v in rows.items()}
        with pkg.Engine(0) as U:
            assert all(U.check_device_source(ptrs[k], rows[k].nbytes) for k in ptrs)
            assert not U.check_device_source(ptrs["alpha"] + 2, 4)
            assert U.upload_device(ptrs, n=N, sh_vec3_per_point=15) == N
            M._assert_same_planes(M._planes(U), _raw_planes(pkg, rows), "upload_device from pinned host memory")
            U.upload(A)
            attrs = {k: v for k, v in ptrs.items() if k != "P"}
            assert U.update_attrs_device(50, n=150, sh_vec3_per_point=15, **attrs) == 150     # (rows 0..149 of the arrays onto splats 50..199)
            s1 = _apply(pkg, A, {k: v[:150] for k, v in rows.items() if k != "P"}, 50, 150)
            M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s1), "update_attrs_device from pinned host memory")
            assert U.move_device(0, ptrs["P"], n=N, Cd=ptrs["Cd"]) == N
            s2 = _apply(pkg, s1, {"P": rows["P"], "Cd": rows["Cd"]}, 0, N)
            M._assert_same_planes(M._planes(U), M._fresh_planes(pkg, s2), "move_device from pinned host memory")
            st = U.stats()
            assert st["upload_ms"][4] == 0.0 and st["move_ms"][0] == 0.0
    finally:
        for p in pinned:
            hb.hip.hipHostFree(p)


# ---- 8. ordering: a producer queued on the context's public stream ---------------------------------------------------------------
def _ordering_worker(q):
    """In a process of its own, torch imported first, as a torch caller has it: the library then shares torch's HIP runtime, so the
    pointer check knows torch's allocations and the stream handle is one runtime's.  Reports through q: ("skip" | "ok" | "error", text)."""
    try:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            q.put(("skip", "torch sees no GPU"))
            return
        import __graft_entry__ as ge
        pkg = ge.load_package()
        A = T._cloud(pkg, 11)
        f = _floats(23)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        names = ("Cd", "alpha", "scale", "orient", "sh")
        base = {k: torch.from_numpy(f[k]).to(dev) for k in ("P",) + names}
        src = {k: torch.zeros_like(v) for k, v in base.items()}     # (what a verb that did not wait would read: zeros)
        big = torch.ones(1 << 26, device=dev)
        torch.cuda.synchronize()
        with pkg.Engine(0) as U:
            U.upload(A)
            U.set_stream(stream.cuda_stream)
            done = torch.cuda.Event()
            with torch.cuda.stream(stream):
                for _ in range(300):                                 # ~150 GB of traffic in front of the sources
                    big.mul_(1.0)
                for k in src:
                    src[k].copy_(base[k] * big[:base[k].numel()].view(base[k].shape))
                done.record(stream)
            assert not done.query(), "the sources were ready before the call: the case tests nothing"
            assert U.update_attrs_device(0, **{k: src[k] for k in names}) == N      # (no torch synchronisation)
            got1 = T._planes(U)
            with torch.cuda.stream(stream):
                for _ in range(300):
                    big.mul_(1.0)
                src["P"].copy_(base["P"].flip(0) * big[:3 * N].view(N, 3))
            assert U.move_device(0, src["P"]) == N
            got2 = M._planes(U)
        rows = {k: src[k].cpu().numpy() for k in names}
        for k in ("Cd", "scale", "orient", "sh"):
            _rounds(pkg, rows[k])
            assert np.array_equal(rows[k], f[k])
        s1 = _apply(pkg, A, rows, 0, N)
        T._assert_same_planes(got1, T._fresh_planes(pkg, s1), "update_attrs_device behind a producer on the public stream")
        s2 = _apply(pkg, s1, {"P": np.ascontiguousarray(f["P"][::-1])}, 0, N)
        M._assert_same_planes(got2, M._fresh_planes(pkg, s2), "move_device behind a producer on the public stream")
        q.put(("ok", "the sources were not ready when update_attrs_device was called"))
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))


@pytest.mark.gpu
def test_ordering_behind_the_public_stream():
    """(Why a process of its own, and why it is the child that looks for the GPU: by now this process has loaded the library against
    the system's HIP runtime, and torch's wheel brings a second copy.  Initialising that copy here -- torch.cuda.is_available() does
    -- would leave two runtimes driving one GPU from one process, and the library's pointer check would not know torch's allocations.
    The child imports torch first, so both bind to one runtime; only importing torch, as here, initialises nothing.)"""
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ordering_worker, args=(q,))
    p.start()
    try:
        kind, text = q.get(timeout=300)
    finally:
        p.join(60)
        if p.is_alive():
            p.terminate()
    if kind == "skip":
        pytest.skip(text)
    assert kind == "ok", text
    print(text)
