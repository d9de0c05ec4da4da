"""The blend contract on the CPU: the oracle's one-pass frame (gso_render_contract) and its per-pixel bound.

A GPU frame may differ from the oracle's in two ways only: the blend kernel's per-pixel early-out (T < 2^-14),
which the oracle restates (out_eo), and 2^x (v_exp_f32 vs gso_exp2f), which out_bound covers.  These tests pin the pieces the
GPU tests rely on: the plain frame is the oracle's frame bit for bit, the bound holds when every alpha is perturbed by the eta it
assumes, and it is tight enough that a frame composited in a subtly wrong way falls outside it.
"""
import numpy as np
import pytest

from helpers import golden_names, load_golden, oracle_render_golden, stop_scene, veil_scene

SEEDS = (1, 2, 3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", golden_names())
def test_plain_and_untrimmed_frames_are_the_oracle_frame(oracle, name):
    d, s, c = load_golden(name)
    ref = oracle_render_golden(oracle, d, s, c)
    depth = d["depth"] if "depth" in d.files else None
    eo, plain, bound, st = oracle.render_contract(s, c, origin=d["origin"], depth=depth, t_min=0.0)
    assert np.array_equal(_bits(plain), _bits(ref))
    assert np.array_equal(_bits(eo), _bits(ref))          # t_min = 0: no early-out
    eo1, plain1, _, _ = oracle.render_contract(s, c, origin=d["origin"], depth=depth, threads=1)
    assert np.array_equal(_bits(plain1), _bits(ref))      # the plain frame never stops early, serial or not
    assert (bound >= 0).all() and np.isfinite(bound).all()


def test_depth_tested_frame_and_row_pieces_are_the_oracle_frame(pkg, oracle):
    s = pkg.scenes.make_scene(20000, seed=41, sh=True)
    cam = pkg.camera.make_camera(256, 192, sh_order=3, frame=2)
    depth = pkg.scenes.sphere_occluder_depth(cam, float(cam.meta["distance"]), 0.5)
    assert 0.03 < (depth < 1.0).mean() < 0.8
    ref = oracle.render_depth(s, cam, depth)
    eo, plain, _, _ = oracle.render_contract(s, cam, depth=depth, t_min=0.0)
    assert np.array_equal(_bits(plain), _bits(ref)) and np.array_equal(_bits(eo), _bits(ref))
    full = oracle.render_contract(s, cam)
    assert np.array_equal(_bits(full[1]), _bits(oracle.render(s, cam)))
    for lo, hi in ((0, 7), (5, 77), (100, 192)):
        part = oracle.render_contract(s, cam, rows=(lo, hi))
        for a, b in zip(part[:3], full[:3]):
            assert np.array_equal(_bits(a), _bits(b[lo:hi]))
        assert np.array_equal(_bits(part[1]), _bits(oracle.render_rows(s, cam, lo, hi)))


def _scenes(pkg):
    cam = pkg.camera.make_camera(320, 240, sh_order=3, frame=1)
    yield "stock", pkg.scenes.make_scene(20000, seed=197, sh=True), cam
    cam0 = pkg.camera.make_camera(200, 150, sh_order=0, frame=3)
    yield "veil", veil_scene(pkg, cam0, seed=5), cam0
    yield "colours", veil_scene(pkg, cam0, n=1500, seed=6, colours=(-2.0, 6.0)), cam0
    s = pkg.scenes.make_scene(20000, seed=198, sh=False)
    s.Cd[:] = pkg.scenes.f16bits(np.random.default_rng(7).uniform(-2.0, 6.0, (s.n, 3)))
    yield "stock colours", s, cam0
    yield "stop", stop_scene(pkg, cam0, seed=8), cam0


def test_bound_holds_when_every_alpha_is_off_by_eta(pkg, oracle):
    eta = oracle.contract_eta()
    assert 5e-7 < eta < 2e-6
    for label, s, cam in _scenes(pkg):
        eo, plain, bound, st = oracle.render_contract(s, cam)
        assert st["infinite"] == 0
        assert (bound > 0).any()
        if label in ("veil", "colours"):
            a = plain[..., 3]
            assert (a > 0.05).mean() > 0.5 and np.median(a[a > 0]) < 0.95, (label, (a > 0.05).mean(), np.median(a[a > 0]))    # deep and mostly unsaturated
        if label == "stop":
            assert st["ambiguous"] >= 20, st                                           # the stop-ambiguity term is taken
        worst = 0.0
        for seed in SEEDS:
            eo_p, plain_p, _, _ = oracle.render_contract(s, cam, eta=eta, seed=seed)
            assert not np.array_equal(eo_p, eo)
            err = np.abs(eo_p.astype(np.float64) - eo)
            assert (err <= bound).all(), (label, seed, float((err / np.maximum(bound, 1e-38)).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-38)).max()))
        print(f"{label}: worst perturbed err / bound = {worst:.3f}, median bound {np.median(bound[plain[..., 3] > 0]):.3e}")


def test_bound_is_infinite_only_where_a_colour_is_beyond_1e30(pkg, oracle):
    s = pkg.scenes.make_scene(3000, seed=9, sh=False)
    s.Cd[:10] = pkg.scenes.f16bits(np.full((10, 3), np.inf))
    cam = pkg.camera.make_camera(128, 96, sh_order=0, frame=0)
    eo, plain, bound, st = oracle.render_contract(s, cam)
    inf = ~np.isfinite(bound)
    assert st["infinite"] == int(inf.any(axis=2).sum()) > 0
    assert (inf.all(axis=2) == inf.any(axis=2)).all()
    assert (np.abs(eo[inf.any(axis=2)][:, :3]) > 1e30).any()


def _frame(pkg, oracle, n, w, h, order, frame):
    s = pkg.scenes.make_scene(n, seed=100 + n % 97, sh=True)
    cam = pkg.camera.make_camera(w, h, sh_order=order, frame=frame)
    rec = oracle.preprocess(s, cam)
    perm = oracle.argsort(rec, oracle.storage_order(s.P))
    return s, cam, rec, perm


@pytest.mark.parametrize("n,w,h,order,frame", [(20000, 320, 240, 2, 1), (100000, 640, 360, 3, 3)])
def test_bound_sees_frames_the_1e3_check_cannot(pkg, oracle, n, w, h, order, frame):
    """mutants of the oracle's own compositing leave the bound somewhere; two of them stay within 1e-3 of the frame everywhere"""
    s, cam, rec, perm = _frame(pkg, oracle, n, w, h, order, frame)
    eo, plain, bound, _ = oracle.blend_contract(rec, perm, w, h)
    ref = oracle.render_contract(s, cam)
    assert np.array_equal(_bits(eo), _bits(ref[0])) and np.array_equal(_bits(bound), _bits(ref[2]))
    covered = plain[..., 3] > 0
    assert covered.mean() > 0.2
    assert float(np.median(bound[covered][:, :3])) <= 4e-6       # colours <= 1.5: a few ulp of a pixel
    assert float(np.median(bound[covered][:, 3])) <= 4e-6

    def verdict(img):
        err = np.abs(img.astype(np.float64) - eo)
        return float(err.max()), int((err > bound).any(axis=2).sum())

    vis = perm[rec["visible"][perm] == 1]
    swapped = perm.copy()                                        # one adjacent pair of visible splats in every 500 drawn swapped
    pos = np.flatnonzero(rec["visible"][perm] == 1)
    for k in range(0, len(vis) - 1, 500):
        swapped[pos[k]], swapped[pos[k + 1]] = swapped[pos[k + 1]], swapped[pos[k]]
    dropped = rec.copy()                                         # one in ten of the faint records (opacity < 0.02) dropped
    faint = np.flatnonzero((rec["visible"] == 1) & (rec["opacity"] < 0.02))
    assert len(faint) > 100
    dropped["visible"][faint[::10]] = 0
    mutants = {
        "swapped pairs": oracle.blend_contract(rec, swapped, w, h)[0],
        "faint records dropped": oracle.blend_contract(dropped, perm, w, h)[0],
        "early-out at 2^-12": oracle.blend_contract(rec, perm, w, h, t_min=2.0 ** -12)[0],
    }
    for name, img in mutants.items():
        e, outside = verdict(img)
        print(f"{name}: max err {e:.3e}, {outside} pixels outside the bound")
        assert outside >= 1, name                                # the contract sees every one ...
        if name != "faint records dropped":
            assert e <= 1e-3, name                               # ... where the old check passes two of them
