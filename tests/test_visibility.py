"""Visibility on the host: the rule of gsr_set_visibility as gsr_visibility_eval states it (no context, no GPU), the refusals that
need no GPU, the struct layouts and the helpers that build crop volumes.

The rule's yardstick is a plain numpy float32 restatement.  Its inputs are chosen so that every product and sum is exact --
positions that are multiples of 1/8 (or one float beside such a value, under matrix entries 0 and 1), matrix entries that are powers
of two -- so fused and unfused evaluation agree and the restatement needs no fmaf."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ONE_UP = np.nextafter(np.float32(1.0), np.float32(2.0))
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
# q = (2 (x - 0.25), 4 (y + 0.5), z / 2): powers of two only
DYADIC = np.array([2, 0, 0, -0.5, 0, 4, 0, 2, 0, 0, 0.5, 0], np.float32)


def _ref(E, volumes, P, hidden=None, first=0):
    """numpy float32: q by the rule's chain (innermost term first), the comparison of the kind, invert, every volume, the mask"""
    P = np.asarray(P, np.float32).reshape(-1, 3)
    vis = np.ones(P.shape[0], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for kind, invert, m in volumes:
            m = np.asarray(m, np.float32).reshape(3, 4)
            q = m[:, 2] * P[:, 2:3] + m[:, 3]
            q = m[:, 1] * P[:, 1:2] + q
            q = m[:, 0] * P[:, 0:1] + q
            assert q.dtype == np.float32
            if kind == E.VOL_BOX:
                inside = np.max(np.abs(q), axis=1) <= 1                 # (np.max propagates a NaN: the comparison is then False)
            else:
                inside = (q[:, 0] * q[:, 0] + (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])) <= 1
            vis &= inside != bool(invert)
    if hidden is not None:
        vis &= ~np.asarray(hidden, bool)[first:first + P.shape[0]]
    return vis


def _eval(E, volumes, P, hidden=None, first=0):
    v, keep = E.visibility_struct(volumes, hidden)
    return E.visibility_eval(v, P, first)


def _grid():
    """every point of a 1/8 grid over [-1.5, 1.5]^3 thinned to ~2000"""
    g = np.arange(-12, 13, dtype=np.float32) / 8
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(P[::7])


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def test_faces_and_their_neighbours(pkg):
    E = pkg.engine
    one, up, dn = np.float32(1), ONE_UP, np.nextafter(np.float32(1), np.float32(0))
    P = np.array([[one, 0, 0], [up, 0, 0], [dn, 0, 0], [-one, 0, 0], [-up, 0, 0], [0, one, 0], [0, up, 0], [0, 0, -one], [0, 0, -up],
                  [one, one, one], [one, one, up], [0, 0, 0]], np.float32)
    want = np.array([1, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1], bool)
    box = [(E.VOL_BOX, 0, IDENT)]
    assert np.array_equal(_eval(E, box, P), want)                       # |q| == 1 is inside, the next float after 1 is outside
    assert np.array_equal(_ref(E, box, P), want)
    ell = [(E.VOL_ELLIPSOID, 0, IDENT)]
    want_e = want.copy()
    want_e[9] = False                                                   # the box's corner lies outside the ball
    assert np.array_equal(_eval(E, ell, P), want_e)
    assert np.array_equal(_ref(E, ell, P), want_e)
    # the same faces through a dyadic map: x = 0.75 -> q.x = 1, y = -0.75 -> q.y = -1, z = 2 -> q.z = 1 (the neighbours lie on the
    # side where the float spacing keeps 2 x - 0.5, 4 y + 2 and z / 2 exact)
    Q = np.array([[0.75, -0.5, 0], [np.nextafter(np.float32(0.75), np.float32(1)), -0.5, 0], [0.25, -0.75, 0],
                  [0.25, np.nextafter(np.float32(-0.75), np.float32(-1)), 0], [0.25, -0.5, 2], [0.25, -0.5, np.nextafter(np.float32(2), np.float32(3))]],
                 np.float32)
    for kind in (E.VOL_BOX, E.VOL_ELLIPSOID):
        got = _eval(E, [(kind, 0, DYADIC)], Q)
        assert np.array_equal(got, [1, 0, 1, 0, 1, 0]) and np.array_equal(got, _ref(E, [(kind, 0, DYADIC)], Q))


def test_nan_and_inf_positions_are_not_inside(pkg):
    E = pkg.engine
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    P = np.array([[nan, 0, 0], [0, nan, 0], [0, 0, nan], [inf, 0, 0], [0, -inf, 0], [0, 0, inf], [nan, inf, -inf], [0.25, -0.5, 0]], np.float32)   # (the last one lies inside under both maps)
    for kind in (E.VOL_BOX, E.VOL_ELLIPSOID):
        for m in (IDENT, DYADIC):
            assert np.array_equal(_eval(E, [(kind, 0, m)], P), [0] * 7 + [1])
            assert np.array_equal(_eval(E, [(kind, 1, m)], P), [1] * 7 + [0])           # ... and so passes an inverted volume
            assert np.array_equal(_ref(E, [(kind, 0, m)], P), [0] * 7 + [1])
    # a NaN matrix entry is the caller's data and follows the rule
    m = IDENT.copy()
    m[5] = nan
    assert not _eval(E, [(E.VOL_BOX, 0, m)], np.zeros((3, 3), np.float32)).any()


def test_grid_against_numpy(pkg):
    E = pkg.engine
    P = _grid()
    half = np.array([2, 0, 0, -1, 0, 0.5, 0, 0, 0, 0, 0.5, 0], np.float32)          # centre (0.5, 0, 0), half extents (0.5, 2, 2)
    cases = {
        "box": [(E.VOL_BOX, 0, DYADIC)], "ellipsoid": [(E.VOL_ELLIPSOID, 0, DYADIC)],
        "intersection": [(E.VOL_BOX, 0, IDENT), (E.VOL_BOX, 0, half)],
        "box minus ellipsoid": [(E.VOL_BOX, 0, IDENT), (E.VOL_ELLIPSOID, 1, DYADIC)],
        "four": [(E.VOL_BOX, 0, IDENT), (E.VOL_BOX, 0, half), (E.VOL_ELLIPSOID, 1, DYADIC), (E.VOL_ELLIPSOID, 0, IDENT)],
        "none": [],
    }
    for name, vols in cases.items():
        got, want = _eval(E, vols, P), _ref(E, vols, P)
        assert np.array_equal(got, want), name
        if vols:
            assert 0.02 < got.mean() < 0.98, (name, got.mean())
    a, b = _eval(E, cases["intersection"][:1], P), _eval(E, cases["intersection"][1:], P)
    assert np.array_equal(_eval(E, cases["intersection"], P), a & b)
    inside_e = _eval(E, [(E.VOL_ELLIPSOID, 0, DYADIC)], P)
    assert np.array_equal(_eval(E, cases["box minus ellipsoid"], P), a & ~inside_e)


def test_mask_bits_and_first(pkg):
    E = pkg.engine
    n = 100
    P = np.zeros((n, 3), np.float32)                                    # inside everything
    for idx in (0, 31, 32, n - 1):
        hidden = np.zeros(n, bool)
        hidden[idx] = True
        words = E.pack_mask(hidden)
        assert words.size == 4 and words[idx >> 5] == np.uint32(1) << np.uint32(idx & 31) and np.count_nonzero(words) == 1
        assert np.array_equal(_eval(E, [], P, hidden), ~hidden)          # n_volumes = 0, a mask only
        for first in (1, 30, 33):
            cnt = n - first
            got = _eval(E, [(E.VOL_BOX, 0, IDENT)], P[:cnt], hidden, first)
            assert np.array_equal(got, ~hidden[first:]), (idx, first)
    hidden = np.zeros(n, bool)
    hidden[[0, 31, 32, n - 1]] = True
    P2 = _grid()[:n - 7]
    box = [(E.VOL_BOX, 0, DYADIC)]
    assert np.array_equal(_eval(E, box, P2, hidden, 7), _ref(E, box, P2, hidden, 7))
    # rows beyond the mask are refused
    v, keep = E.visibility_struct([], hidden)
    with pytest.raises(E.GsrError) as ei:
        E.visibility_eval(v, P, 1)
    assert ei.value.code == INVALID
    assert E.visibility_eval(None, P).all()                             # no struct: everything visible


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _bad_structs(E):
    ok = [(E.VOL_BOX, 0, IDENT)]
    out = {}
    v, _ = E.visibility_struct(ok)
    v.n_volumes = -1
    out["n_volumes -1"] = v
    v, _ = E.visibility_struct(ok)
    v.n_volumes = E.VIS_MAX_VOLUMES + 1
    out["n_volumes 5"] = v
    for kind in (0, 3, -1):
        out[f"kind {kind}"] = E.visibility_struct([(E.VOL_BOX, 0, IDENT), (kind, 0, IDENT)])[0]
    for inv in (2, -1):
        out[f"invert {inv}"] = E.visibility_struct([(E.VOL_ELLIPSOID, inv, IDENT)])[0]
    v, _ = E.visibility_struct(ok)
    v.reserved_ = 1
    out["reserved_"] = v
    return out


def test_refusals_that_need_no_gpu(pkg):
    E = pkg.engine
    L = pkg.load_library()
    P = np.zeros((4, 3), np.float32)
    out = np.zeros(4, np.uint8)
    ok, _ = E.visibility_struct([(E.VOL_BOX, 0, IDENT)])
    assert L.gsr_visibility_eval(C.byref(ok), P.ctypes.data, 0, 4, out.ctypes.data) == 0 and out.all()
    for name, v in _bad_structs(E).items():
        assert L.gsr_visibility_eval(C.byref(v), P.ctypes.data, 0, 4, out.ctypes.data) == INVALID, name
        assert b"gsr_visibility_eval" in L.gsr_last_error()
        assert L.gsr_visibility_eval(C.byref(v), None, 0, 0, None) == INVALID, name      # (the struct is looked at before the rows)
    # a volume beyond n_volumes is not looked at
    v, _ = E.visibility_struct([(E.VOL_BOX, 0, IDENT)])
    v.volume[1].kind = 77
    assert L.gsr_visibility_eval(C.byref(v), P.ctypes.data, 0, 4, out.ctypes.data) == 0
    assert L.gsr_visibility_eval(C.byref(ok), None, 0, 4, out.ctypes.data) == INVALID
    assert L.gsr_visibility_eval(C.byref(ok), P.ctypes.data, -1, 4, out.ctypes.data) == INVALID
    assert L.gsr_visibility_eval(C.byref(ok), P.ctypes.data, 0, -1, out.ctypes.data) == INVALID
    # the verbs without a context
    assert L.gsr_set_visibility(None, C.byref(ok)) == INVALID and b"NULL" in L.gsr_last_error()
    assert L.gsr_set_visibility(None, None) == INVALID
    assert L.gsr_get_visibility(None, C.byref(E.gsr_visibility()), None) == INVALID
    assert L.gsr_multi_set_visibility(None, C.byref(ok)) == INVALID
    assert L.gsplat_renderer_set_visibility(None, C.byref(ok)) == INVALID


def test_dry_shim_takes_volumes_and_refuses_a_mask(pkg):
    E = pkg.engine
    R = pkg.GSplatRenderer(-1)
    try:
        ok, _ = E.visibility_struct([E.crop_box((0, 0, 0), 0.5)])
        assert R.setVisibility(ok) == 0
        assert R.setVisibility(None) == 0
        masked, keep = E.visibility_struct([E.crop_box((0, 0, 0), 0.5)], np.zeros(10, bool))
        assert R.setVisibility(masked) == INVALID
        for name, v in _bad_structs(E).items():
            assert R.setVisibility(v) == INVALID, name
    finally:
        R.close()


def test_structs_match_the_header(pkg):
    E = pkg.engine
    assert C.sizeof(E.gsr_crop_volume) == 56
    assert C.sizeof(E.gsr_visibility) == 8 + 4 * 56 + 8 + 8
    assert E.gsr_visibility.volume.offset == 8 and E.gsr_visibility.mask.offset == 232 and E.gsr_visibility.mask_splats.offset == 240
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    defs = dict(re.findall(r"#define\s+(GSR_VIS_MAX_VOLUMES|GSR_VOL_BOX|GSR_VOL_ELLIPSOID)\s+(\d+)", text))
    assert (int(defs["GSR_VIS_MAX_VOLUMES"]), int(defs["GSR_VOL_BOX"]), int(defs["GSR_VOL_ELLIPSOID"])) == \
        (E.VIS_MAX_VOLUMES, E.VOL_BOX, E.VOL_ELLIPSOID)
    for name, body in (("gsr_crop_volume", [n for n, _ in E.gsr_crop_volume._fields_]), ("gsr_visibility", [n for n, _ in E.gsr_visibility._fields_])):
        decl = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        names = [re.sub(r"\[.*\]", "", d.strip().split()[-1]).lstrip("*") for d in decl.split("{", 1)[1].split(";") if d.strip()]
        assert names == body, (name, names)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def test_crop_helpers_map_the_extents_onto_the_unit_volume(pkg):
    E = pkg.engine
    c, h = np.array([0.5, -0.25, 2.0]), np.array([0.5, 2.0, 0.125])
    for make, kind in ((E.crop_box, E.VOL_BOX), (E.crop_ellipsoid, E.VOL_ELLIPSOID)):
        k, inv, m = make(c, h)
        assert (k, inv) == (kind, 0) and m.dtype == np.float32 and m.shape == (12,)
        assert make(c, h, invert=True)[1] == 1
        M = m.reshape(3, 4).astype(np.float64)
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                p = c.copy()
                p[ax] += sgn * h[ax]
                q = M[:, :3] @ p + M[:, 3]
                want = np.zeros(3)
                want[ax] = sgn
                assert np.array_equal(q, want), (ax, sgn, q)            # dyadic extents: exactly +-1
                assert E.visibility_eval(E.visibility_struct([(k, 0, m)])[0], p[None].astype(np.float32))[0]
        assert np.array_equal(M[:, :3] @ c + M[:, 3], np.zeros(3))
    # a scalar half extent, and a rotated volume: the columns of the rotation are the volume's axes
    assert np.array_equal(E.crop_box((0, 0, 0), 0.5)[2], np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0], np.float32))
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    h = np.array([0.9, 0.5, 0.7])
    k, inv, m = E.crop_ellipsoid(c, h, R)
    M = m.reshape(3, 4).astype(np.float64)
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            want = np.zeros(3)
            want[ax] = sgn
            assert np.allclose(M[:, :3] @ (c + sgn * h[ax] * R[:, ax]) + M[:, 3], want, atol=2e-6)
    assert not np.allclose(M[0, :3], [1 / 0.9, 0, 0])                   # (the rotation is in it)
    with pytest.raises(ValueError):
        E.crop_box((0, 0), 1.0)
