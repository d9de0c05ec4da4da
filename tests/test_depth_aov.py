"""The depth AOV on the CPU: the resolve rule's known answers, the ABI, and the teeth of the oracle-side reference the GPU tests
(test_depth_aov_gpu.py) hold the plane to."""
import os

import numpy as np

import depth_aov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_resolve_depth_known_answers(pkg):
    """cov >= cov_min ? min(zsum / cov, 1) : 1, one IEEE division"""
    f = np.float32
    third = f(1.0) / f(3.0)
    plane = np.array([[0.1, 0.49999997],            # coverage just below cov_min: the far plane
                      [0.1, 0.5],                   # at cov_min: resolved
                      [0.3, 0.75],                  # above
                      [0.9, 0.8],                   # a quotient above 1 is clamped to the far plane
                      [0.0, 0.0],                   # nothing covers the pixel
                      [third, 1.0],                 # (division by 1 is exact)
                      [0.25, third]], np.float32)   # (a quotient that rounds: the correctly rounded one)
    got = pkg.engine.resolve_depth(plane, 0.5)
    want = np.array([1.0, f(0.1) / f(0.5), f(0.3) / f(0.75), 1.0, 1.0, third, 1.0], np.float32)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    low = pkg.engine.resolve_depth(plane, 0.25)
    assert low[0] == f(0.1) / f(0.49999997) and low[6] == f(0.25) / third and low[4] == 1.0
    # cov_min = 0 resolves every pixel; the empty one (0 / 0) still reads as the far plane
    assert pkg.engine.resolve_depth(plane, 0.0)[4] == 1.0
    # shapes pass through, [..., 2] -> [...]
    assert pkg.engine.resolve_depth(np.zeros((3, 5, 2), np.float32)).shape == (3, 5)
    assert pkg.engine.resolve_depth(np.zeros((0, 2), np.float32)).shape == (0,)


def test_resolve_depth_rejects_bad_arguments(pkg):
    L = pkg.load_library()
    a = np.zeros(8, np.float32)
    out = np.zeros(4, np.float32)
    assert L.gsr_resolve_depth(None, 4, 0.5, out.ctypes.data) == GSR_E_INVALID
    assert L.gsr_resolve_depth(a.ctypes.data, 4, 0.5, None) == GSR_E_INVALID
    assert L.gsr_resolve_depth(a.ctypes.data, -1, 0.5, out.ctypes.data) == GSR_E_INVALID
    assert b"gsr_resolve_depth" in L.gsr_last_error()
    assert L.gsr_resolve_depth(a.ctypes.data, 4, 0.5, out.ctypes.data) == 0
    # no context: the device form and the render verb refuse before they touch a GPU
    assert L.gsr_resolve_depth_device(None, a.ctypes.data, 4, 0.5, out.ctypes.data) == GSR_E_INVALID
    assert L.gsr_render_aov(None, None, None, 0, None, 0, pkg.engine.AOV_DEPTH, None) == GSR_E_INVALID


def test_abi_has_the_aov_verbs(pkg):
    L = pkg.load_library()
    for name in ("gsr_render_aov", "gsr_resolve_depth", "gsr_resolve_depth_device", "gsplat_renderer_set_aov_target"):
        assert hasattr(L, name), name
        assert name in pkg.engine.C_ABI_SYMBOLS
    assert pkg.engine.AOV_DEPTH == 1
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert "#define GSR_AOV_DEPTH 1" in hdr


def test_dry_shim_remembers_the_aov_target(pkg):
    R = pkg.GSplatRenderer(-1)
    plane = np.zeros((4, 4, 2), np.float32)
    assert R.setAovTarget(pkg.engine.AOV_DEPTH, plane.ctypes.data) == 0
    assert R.setAovTarget(0, None) == 0
    assert R.setAovTarget(7, plane.ctypes.data) == GSR_E_INVALID


def test_oracle_reference_has_teeth(pkg, oracle):
    """the reference of the GPU tests -- zwin in the records' red channel, composited by the oracle's contract pass -- separates a
    plane whose window depths are off by ONE place in depth order from the right one, on most covered pixels.  That needs a camera
    whose planes sit close around the cloud: with the stock planes (0.01, 1e5) every zwin lies in [0.9972, 0.9982], and the mutant
    hides inside the bound."""
    s = pkg.scenes.make_scene(4000, seed=197, sh=True)
    cam = ref.tight_camera(pkg)
    assert (cam.width, cam.height) == (72, 40)
    rec, perm = ref.records(oracle, s, cam)
    vis = rec["visible"] == 1
    z = rec["zwin"][vis]
    assert vis.sum() > 3000 and z.min() <= 0.2 and z.max() >= 0.8 and 0.0 <= z.min() and z.max() <= 1.0, (z.min(), z.max())
    zsum, cov, bz, bc = ref.reference(oracle, rec, perm, cam)
    # the coverage is the colour frame's alpha, bit for bit: the red channel is all that was swapped
    eo, _, bound, _ = oracle.render_contract(s, cam)
    assert np.array_equal(_bits(cov), _bits(eo[..., 3])) and np.array_equal(_bits(bc), _bits(bound[..., 3]))
    covered = cov > 0
    assert covered.mean() > 0.3
    assert np.isfinite(bz).all() and float(np.median(bz[covered])) <= 4e-6
    assert (zsum[~covered] == 0).all() and (zsum[covered] > 0).all()      # (every zwin is positive here)
    zm = ref.reference(oracle, ref.rotated_zwin(rec, perm), perm, cam)[0]
    outside = (np.abs(zm.astype(np.float64) - zsum) > bz) & covered
    print(f"rotated zwin: {int(outside.sum())} of {int(covered.sum())} covered pixels outside the bound")
    assert outside.sum() > 0.5 * covered.sum()
    # ... and with the stock planes it would not
    cam0 = pkg.camera.make_camera(72, 40, sh_order=3, frame=1)
    rec0, perm0 = ref.records(oracle, s, cam0)
    z0 = rec0["zwin"][rec0["visible"] == 1]
    assert z0.max() - z0.min() < 2e-3
