"""The cluster cull's host models and cases, without a GPU: tests/cluster_cull_ref.py (the extent half and the cluster planes) held to
brute force, and tests/cull_edge_cases.py (the sweeps across every cull boundary) held to what test_cull_edges_gpu.py needs of them."""
import math

import numpy as np
import pytest

import cluster_cull_ref as R
import cull_edge_cases as K

f32 = np.float32


# ---- the extent half --------------------------------------------------------------------------------------------------------
def _kernel_mf(shape_bits):
    """gsr_extent_half restated in numpy float32, in the kernel's op order (no contraction), on the model's float32 rotation"""
    v = R.h2f(shape_bits)
    Rm = [[f32(x) for x in row] for row in R.f32_rotation(*v[3:])]
    s = [f32(x) for x in v[:3]]
    with np.errstate(over="ignore", under="ignore"):
        col = [(Rm[0][p] * Rm[0][p] + Rm[1][p] * Rm[1][p]) + Rm[2][p] * Rm[2][p] for p in range(3)]
        mf2 = ((s[0] * s[0]) * col[0] + (s[1] * s[1]) * col[1]) + (s[2] * s[2]) * col[2]
        mfv = np.sqrt(mf2) * f32(R.C1001)
    return R.ceil_half(float(mfv)), float(mfv)


def test_delta_is_the_derived_gamma():
    u = 2.0 ** -24
    assert R.DELTA == 6 * u / (1 - 6 * u) + 2.0 ** -50
    assert 2.0 ** -22 < R.DELTA < 2.0 ** -20
    assert R.C1001 == float(np.float32(1.001)) and R.C1001 != 1.001


def test_ceil_half_edges():
    assert R.ceil_half(0.0) == 0.0
    assert R.ceil_half(2.0 ** -30) == 2.0 ** -24
    assert R.ceil_half(1.0) == 1.0 and R.ceil_half(float(np.nextafter(f32(1.0), f32(2.0)))) == 1.0 + 2.0 ** -10
    assert R.ceil_half(65504.0) == 65504.0
    assert R.ceil_half(65504.0 + 2.0 ** -8) == math.inf and R.ceil_half(65519.0) == math.inf
    assert R.ceil_half(59968.0 + 1e-3) == 60000.0


def test_rotation_entries_match_float64_on_unit_quaternions():
    rng = np.random.default_rng(3)
    q = rng.normal(size=(200, 4))
    qh = R.h2f(R.f2h(q / np.linalg.norm(q, axis=1, keepdims=True)))
    for qi, qj, qk, qr in qh:
        got = np.array(R.f32_rotation(qi, qj, qk, qr))
        f = lambda x: float(np.float32(x))
        want = np.array([[f(1 - 2 * f(qj * qj + qk * qk)), 2 * f(qi * qj - qr * qk), 2 * f(qi * qk + qr * qj)],
                         [2 * f(qi * qj + qr * qk), f(1 - 2 * f(qi * qi + qk * qk)), 2 * f(qj * qk - qr * qi)],
                         [2 * f(qi * qk - qr * qj), 2 * f(qj * qk + qr * qi), f(1 - 2 * f(qi * qi + qj * qj))]])
        assert np.array_equal(got, want)
    # the identity and the zero quaternion give I exactly: the probes rely on it
    assert R.f32_rotation(0, 0, 0, 1) == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] == R.f32_rotation(0, 0, 0, 0)


def test_float32_chain_stays_inside_the_bracket(pkg):
    """the kernel's chain restated in float32 lands inside [lo, hi] on every bounds cloud row and on random halves of every binade"""
    rng = np.random.default_rng(4)
    rows = [np.concatenate([s.scale[i], s.orient[i]]) for s in (R.bounds_cloud(5, pkg.scenes), R.bounds_cloud(6, pkg.scenes))
            for i in range(s.n)]
    sc = R.f2h(np.exp2(rng.uniform(-24, 15.9, (3000, 3))) * rng.choice([-1, 1], (3000, 3)))
    q = R.f2h(rng.normal(size=(3000, 4)) * np.exp2(rng.uniform(-12, 8, (3000, 1))))
    rows += list(np.concatenate([sc, q], axis=1))
    checked = 0
    for b in rows:
        br = R.extent_bracket(b)
        if br is None:
            continue
        mf, _ = _kernel_mf(b)
        assert br[0] <= mf <= br[1], (R.h2f(b).tolist(), br, mf)
        checked += 1
    assert checked > 3000


def test_probes_land_where_they_say():
    """each probe's float32 extent is its target; sixteen steps away the bracket holds ONE half, the rounded-up one; one step away
    the bracket still holds the half the kernel must give"""
    assert len(R.probes()) == len(R.PROBE_HALVES) * len(R.PROBE_STEPS)
    for H, k, t, sb in R.probes():
        b = np.array(list(sb) + list(R.f2h(np.array([0.0, 0.0, 0.0, 1.0]))), np.uint16)
        mf, mfv = _kernel_mf(b)
        assert mfv == float(t)
        with np.errstate(over="ignore"):
            want = H if k < 0 else float(np.nextafter(np.float16(H), np.float16(np.inf)))      # (65504: +inf)
        assert mf == want, (H, k, mf, want)
        lo, hi = R.extent_bracket(b)
        assert lo <= want <= hi
        if abs(k) == 16:
            assert lo == hi == want, (H, k, lo, hi)
    # around the flag: 59968 stays below 6e4, 60000 does not
    flags = {(H, k): not (R.extent_bracket(np.array(list(sb) + [0, 0, 0, 0x3c00], np.uint16))[0] < R.FLAG_MF)
             for H, k, _, sb in R.probes()}
    assert not flags[(59968.0, -16)] and flags[(59968.0, 16)] and flags[(60000.0, -16)]


def test_bounds_cloud_reaches_every_edge(pkg):
    s = R.bounds_cloud(5, pkg.scenes)
    assert s.n == 5 * 64 + 17
    for name, hb in R.SCALE_EDGES.items():
        for ax in range(3):
            assert (s.scale[:, ax] == hb).any(), (name, ax)
    q = R.f2h(np.array([v for _, v in R.QUATS]))
    for k in range(len(q)):
        assert (s.orient == q[k]).all(axis=1).any(), R.QUATS[k][0]
    assert np.isnan(s.P).any() and np.isinf(s.P).any() and (np.abs(s.P) == np.float32(3.1e38)).any()
    assert ((s.P == 0) & np.signbit(s.P)).any()
    for _, _, _, sb in R.probes():
        assert (np.sort(s.scale, axis=1) == np.sort(np.array(sb, np.uint16))).all(axis=1).any()


def test_cluster_fold_model():
    P = np.zeros((70, 3), np.float32)
    P[:, 0] = np.arange(70)
    P[3, 1] = np.nan
    P[5, 2] = np.inf
    mf = np.full(70, 0.5, np.float32)
    mf[66] = 7.0
    mf[69] = np.inf                     # behind n: does not count
    A, B = R.cluster_planes(P, mf, 68)
    assert A.shape == (2, 4)
    assert A[0].tolist() == [0, 0, 0, 0.5] and B[0].tolist() == [63, 0, np.inf, 1.0]
    assert A[1].tolist() == [64, 0, 0, 7.0] and B[1].tolist() == [67, 0, 0, 0.0]
    A, B = R.cluster_planes(np.full((3, 3), np.nan, np.float32), np.zeros(3, np.float32), 3)
    assert np.array_equal(A[0, :3], np.full(3, R.FOLD_START)) and np.array_equal(B[0, :3], np.full(3, -R.FOLD_START))
    assert B[0, 3] == 1.0


# ---- the sweeps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.all_scenes(), ids=K.scene_id)
def test_sweep_scene(pkg, oracle, case):
    sc = K.scene(pkg, *case)
    s, cam = sc["splats"], sc["cam"]
    nc = sc["clumps"]
    assert s.n == nc * K.CLUMP <= 8192 and cam.width * cam.height <= 320 * 200
    assert set(s.alpha.tolist()) == {1.0, K.ALPHA_MIN} and np.float32(K.ALPHA_MIN) >= 1.0 / 255.0 > np.nextafter(np.float32(K.ALPHA_MIN), np.float32(0))
    # every clump fills exactly one cluster of the storage order.  (The oracle keeps the upload order of a cloud with a non-finite
    # position; the engine gives such a splat the largest Morton code.  So the NaN splat stands at its clump's place here: the
    # cloud's largest corner, which has that code.)
    nan_row = sc["flagged"]["NaN position off screen"] * K.CLUMP + K.CLUMP - 1
    Pm = s.P.copy()
    Pm[nan_row] = Pm[nan_row - 1]
    assert np.isfinite(Pm).all() and np.array_equal(Pm[nan_row], Pm.max(axis=0))
    order = oracle.storage_order(Pm)
    slot = np.empty(s.n, np.int64)
    slot[order] = np.arange(s.n)
    cl = (slot // K.CLUMP).reshape(nc, K.CLUMP)
    assert (cl == cl[:, :1]).all() and len(np.unique(cl[:, 0])) == nc
    # the spread clumps: one Morton cell; the probe splat (the first) carries the sweep's coordinate, lies on the inner face of the
    # clump's box along the swept axis, and every other splat lies further outside the boundary
    spread = sc["spread"]
    assert spread.shape == (nc,) and spread.any() == (case[3] == "spread")
    rows = s.P.reshape(nc, K.CLUMP, 3)
    assert (Pm.reshape(nc, K.CLUMP, 3)[~spread] == Pm.reshape(nc, K.CLUMP, 3)[~spread][:, :1]).all()      # every other clump is coincident
    for sw in sc["sweeps"] if spread.any() else ():
        ks = np.array(sw.clumps)
        sp = spread[ks]
        fine = np.array([k == "fine" for k in sw.kind])
        assert sp.sum() * 2 >= len(ks) and (sp & fine).sum() >= 3 and (sp & (sw.coord > 0)).sum() >= 2 and (sp & (sw.coord < 0)).sum() >= 3, (sw.boundary, sp)
        for k, c0 in zip(ks[sp], sw.coord[sp]):
            q = K.morton_cells(rows[k], Pm.min(axis=0), Pm.max(axis=0))[0]
            assert (q == q[0]).all(), (sw.boundary, k)
            c = K.boundary_coord(cam, rows[k].astype(np.float64), sw.boundary)
            assert c[0] == c0 and (c[1:] < c0).all(), (sw.boundary, k)
            along = (rows[k, 1:, sw.axis].astype(np.float64) - float(rows[k, 0, sw.axis])) * sw.out
            assert along.min() > 0 and along.max() >= 0.2 * K._spread_cap(sw.boundary, sw.grad), (sw.boundary, k, along.max())
    rec = oracle.preprocess(s, cam, origin=sc["origin"])
    for sw in sc["sweeps"]:
        c = sw.coord
        assert len(sw.clumps) == len(c) == len(sw.P)
        assert np.array_equal(K.boundary_coord(cam, s.P[np.array(sw.clumps) * K.CLUMP].astype(np.float64), sw.boundary), c)
        assert (np.diff(c) < 0).all(), f"{sw.boundary}: not monotone"
        assert (c > 0).sum() >= 3 and (c < 0).sum() >= 3, (sw.boundary, c)
        if sw.boundary in K.PLANES:
            v = rec["visible"][np.array(sw.clumps) * K.CLUMP]
            assert v[0] == 1 and v[-1] == 0 and (np.diff(v.astype(int)) <= 0).all(), (sw.boundary, v)
        # the nearest steps move one coordinate only: by one ulp of it, or by 1/64 px where that is more
        fine = np.array([i for i, k in enumerate(sw.kind) if k == "fine"])
        assert len(fine) == 7 and (np.diff(fine) == 1).all()
        d = np.diff(sw.P[fine].astype(np.float64), axis=0)
        assert ((d != 0).sum(axis=1) == 1).all()
        ulp = float(np.spacing(np.abs(sw.P[fine]).max(axis=0))[np.argmax(np.abs(d[0]))])
        step, dc = np.abs(d).max(axis=1), np.abs(np.diff(c[fine]))
        on_screen = not (sw.boundary in K.PLANES or sw.boundary.startswith("depth"))
        assert ((step == ulp) | (on_screen & (np.abs(dc - 1.0 / 64.0) <= dc / step * ulp + 1e-3 / 64.0))).all(), (sw.boundary, step, dc)
    # the flagged clumps: no per-splat rule keeps a splat of them
    for name, k in sc["flagged"].items():
        rows = slice(k * K.CLUMP, (k + 1) * K.CLUMP)
        X, Y, z, w = K.clip(cam, s.P[rows].astype(np.float64))
        fin = np.isfinite(X)
        gone = (rec["visible"][rows] == 0) | ~fin
        with np.errstate(invalid="ignore"):
            gone |= (X < -100) | (X > cam.width + 100) | (Y < -100) | (Y > cam.height + 100)
        assert gone.all(), name
    assert np.isnan(s.P[sc["flagged"]["NaN position off screen"] * K.CLUMP + K.CLUMP - 1]).any()
    assert (s.scale[sc["flagged"]["inf scale behind the eye"] * K.CLUMP + K.CLUMP - 1] == 0x7c00).any()
