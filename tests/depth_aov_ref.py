"""The depth AOV's CPU reference, shared by test_depth_aov.py and test_depth_aov_gpu.py.

The oracle composites any records in any order and returns the early-out frame with its per-pixel bound (oracle.blend_contract,
DESIGN.md section 2).  A record carries its window depth `zwin`; written into the records' red channel, the oracle's red output IS
the AOV's zsum -- the same weights w = T * alpha on the same fragments, accumulated with the same fmaf -- its alpha the AOV's cov,
and the bound's red and alpha channels what a GPU plane may differ by."""
import numpy as np

TIGHT_NEAR, TIGHT_FAR = 3.6, 5.7      # planes close around the stock cloud at the stock orbit distance: zwin spreads over most of [0, 1]


def tight_camera(pkg, width=72, height=40, sh_order=3, frame=1):
    return pkg.camera.make_camera(width, height, sh_order=sh_order, frame=frame, near=TIGHT_NEAR, far=TIGHT_FAR)


def records(oracle, splats, cam, origin=(0, 0, 0)):
    """(records, depth order) of the frame, as the oracle draws it"""
    rec = oracle.preprocess(splats, cam, origin)
    return rec, oracle.argsort(rec, oracle.storage_order(splats.P))


def reference(oracle, rec, perm, cam, depth=None):
    """(zsum, cov, bound_zsum, bound_cov), float32 [H, W] each, from records whose zwin may have been tampered with"""
    rz = rec.copy()
    rz["r"] = rec["zwin"]
    eo, _, bound, _ = oracle.blend_contract(rz, perm, cam.width, cam.height, depth=depth)
    return eo[..., 0], eo[..., 3], bound[..., 0], bound[..., 3]


def rotated_zwin(rec, perm):
    """the mutant: every visible record carries the window depth of its predecessor in depth order (the nearest one the farthest's)"""
    vis = perm[rec["visible"][perm] == 1]
    out = rec.copy()
    out["zwin"][vis] = np.roll(rec["zwin"][vis], 1)
    return out
