"""The extent half of geoB and the cluster planes clusA / clusB on the GPU, held to the float64 model of tests/cluster_cull_ref.py.

The cloud is cluster_cull_ref.bounds_cloud: 5 x 64 + 17 splats (the last cluster is partly empty) whose scale halves, quaternions and
positions reach every edge of gsr_extent_half and of the cluster fold, and whose rounding probes land the float32 extent one and
sixteen float32 steps below and above a half value, around the 6e4 flag and around 65504.  Four paths write the planes: a host upload,
a device-source upload (float32 arrays in device memory, quantised on the GPU), a host upload in upload order (GSR_OPT_STORAGE_ORDER =
0), and an update of scale and orient in place (k_update + k_cluster_extents).  After each, for every live slot: the seven given halves
and the position are the input's, and the eighth half lies in the model's bracket (or, for a non-finite input half, is not < 6e4); for
every cluster: both planes equal the model's fold of the live slots, read back from the resident planes themselves."""
import numpy as np
import pytest

import cluster_cull_ref as R
from helpers import HipBuffers

pytestmark = pytest.mark.gpu

N = R.N_BOUNDS


def _same_or_both_nan_half(a, b):
    fa, fb = R.h2f(a), R.h2f(b)
    return np.where(np.isnan(fa) | np.isnan(fb), np.isnan(fa) == np.isnan(fb), a == b)


def _check(pkg, eng, s, label):
    E = pkg.engine
    n = s.n
    perm = eng.debug_storage_order(n).astype(np.int64)
    assert sorted(perm.tolist()) == list(range(n)), label
    geoA = eng.debug_resident(E.RESIDENT_GEOA).view(np.float32).reshape(-1, 4)[:n]
    geoB = eng.debug_resident(E.RESIDENT_GEOB).view(np.uint16).reshape(-1, 8)[:n]
    clusA = eng.debug_resident(E.RESIDENT_CLUSA).view(np.float32).reshape(-1, 4)
    clusB = eng.debug_resident(E.RESIDENT_CLUSB).view(np.float32).reshape(-1, 4)
    assert clusA.shape[0] == clusB.shape[0] == (n + 63) // 64, label
    # the given halves and the positions, slot by slot
    want7 = np.concatenate([s.scale, s.orient], axis=1)[perm]
    assert _same_or_both_nan_half(geoB[:, :7], want7).all(), f"{label}: the seven given halves"
    P = s.P[perm]
    assert np.array_equal(geoA[:, :3], P, equal_nan=True), f"{label}: positions"
    # the extent half against the bracket
    mf = R.h2f(geoB[:, 7])
    bad = []
    for j in range(n):
        br = R.extent_bracket(geoB[j, :7])
        if br is None:
            if mf[j] < R.FLAG_MF:
                bad.append((j, int(perm[j]), "non-finite input", float(mf[j])))
        elif not (br[0] <= mf[j] <= br[1]):
            bad.append((j, int(perm[j]), br, float(mf[j]), R.h2f(geoB[j, :7]).tolist()))
    assert not bad, f"{label}: {len(bad)} extent halves outside the model's bracket, first {bad[:4]}"
    # the two cluster planes against the fold of the live slots
    A, B = R.cluster_planes(geoA[:, :3], mf.astype(np.float32), n)
    for c in range(A.shape[0]):
        assert np.array_equal(clusA[c], A[c]), f"{label}: clusA[{c}] = {clusA[c].tolist()}, model {A[c].tolist()}"
        assert np.array_equal(clusB[c], B[c]), f"{label}: clusB[{c}] = {clusB[c].tolist()}, model {B[c].tolist()}"
    return B[:, 3]


@pytest.fixture(scope="module")
def clouds(pkg):
    """the cloud, and a second one whose scale / orient rows go into the first by update_attrs"""
    return R.bounds_cloud(5, pkg.scenes), R.bounds_cloud(6, pkg.scenes)


@pytest.mark.parametrize("order", (1, 0))
def test_upload_planes_against_model(pkg, clouds, order):
    s = clouds[0]
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, order)
        U.upload(s)
        flags = _check(pkg, U, s, f"upload, order {order}")
    assert flags.any(), "no cluster carries the never-cull flag: the edges were not reached"


def test_upload_device_planes_against_model(pkg, clouds):
    s = clouds[0]
    hb = HipBuffers()
    try:
        f32 = lambda h: np.ascontiguousarray(R.h2f(h), np.float32)
        attrs = dict(P=np.ascontiguousarray(s.P, np.float32), Cd=f32(s.Cd), alpha=np.ascontiguousarray(s.alpha, np.float32),
                     scale=f32(s.scale), orient=f32(s.orient))
        ptrs = {k: hb.upload(v) for k, v in attrs.items()}
        with pkg.Engine(0) as U:
            assert U.upload_device(ptrs, n=N) == N
            _check(pkg, U, s, "upload_device")
    finally:
        hb.free()


def test_update_scale_orient_planes_against_model(pkg, clouds):
    s, t = clouds
    with pkg.Engine(0) as U:
        U.upload(s)
        assert U.update_attrs(0, scale=t.scale, orient=t.orient) == N
        edited = pkg.scenes.Splats(s.P.copy(), s.Cd.copy(), s.alpha.copy(), t.scale.copy(), t.orient.copy(), None, None, None)
        _check(pkg, U, edited, "update_attrs scale + orient")
