"""gsr_transform on the host: the rule gsr_xform_prepare derives, and gsr_transform_eval -- the functions the kernel evaluates -- against a
numpy float64 model.  No GPU.  (tests/test_transform_gpu.py holds the kernel and the verb to gsr_transform_eval bit for bit.)

The bounds, all derived from the number formats (u32 = 2^-24: one float32 rounding, relative; u16 = 2^-11: one binary16 rounding):
  P'      three fmaf, so three float32 roundings of partial sums no larger than S = sum |A_rk p_k| + |t_r|:  |P' - v| <= 4 u32 S
  a half  h = f2h(chain): |h2f(h) - v| <= u16 |v| + L u32 T  (+ 2^-24 where |v| < 2^-14: the absolute spacing of half subnormals), with
          v the model value of the chain in float64 from the float32 rule and the input halves, T the sum of the magnitudes of the
          chain's terms and L its length in roundings: scale 1 (one product), orient 4 (one product under three fmaf), an SH band
          2l + 1 (one product under 2l fmaf)
  D_l     its entries are float64 values rounded to float32 once, |D| <= 1:  |Y_l(R d).(D_l c) - Y_l(d).c| <= (2l+1) u32 max|Y_l| max|c| + 1e-12
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import transform_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
U32, U16 = 2.0 ** -24, 2.0 ** -11


def h2f(a):
    return np.ascontiguousarray(a, np.uint16).view(np.float16).astype(np.float64)


def _cloud(pkg, sh=True, n=TC.N, seed=11):
    return pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-3.5, -2.0))


def _rotation(pkg, name):
    """(the float64 rotation matrix of a test transform, its rule)"""
    x = TC.make_xform(pkg, name)
    return TC.quat_matrix(np.array(list(x.rotate), np.float64)), pkg.engine.xform_prepare(x)


def _half_bound(v, T, length):
    v, T = np.asarray(v, np.float64), np.asarray(T, np.float64)
    return U16 * np.abs(v) + length * U32 * T + np.where(np.abs(v) < 2.0 ** -14, 2.0 ** -24, 0.0)


def _sh_model(rule, sh_halves):
    """(v, bound) float64 (n, 15) of one channel's row after the SH rule, from the float32 band matrices and the input halves"""
    c = h2f(sh_halves)[:, :15]
    v, b = np.zeros_like(c), np.zeros_like(c)
    for l in (1, 2, 3):
        D = rule["D%d" % l].astype(np.float64)
        v[:, TC.BAND[l]] = c[:, TC.BAND[l]] @ D.T
        b[:, TC.BAND[l]] = _half_bound(v[:, TC.BAND[l]], np.abs(c[:, TC.BAND[l]]) @ np.abs(D).T, 2 * l + 1)
    return v, b


# ---- 1. the SH matrices ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.ROTATIONS)
def test_sh_matrices_keep_the_colour(pkg, name):
    R, rule = _rotation(pkg, name)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for l in (1, 2, 3):
        D = rule["D%d" % l].astype(np.float64)
        assert np.abs(D).max() <= 1.0 + 1e-6
        c = rng.uniform(-1.0, 1.0, (200, 2 * l + 1))
        got = np.einsum("nm,nm->n", TC.sh_basis(l, d @ R.T), c @ D.T)
        want = np.einsum("nm,nm->n", TC.sh_basis(l, d), c)
        bound = (2 * l + 1) * U32 * TC.basis_max(l) * np.abs(c).max() + 1e-12
        err = float(np.abs(got - want).max())
        print(f"{name} band {l}: max |colour error| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, l, err, bound)


def test_sh_matrices_compose_and_the_identity_is_exact(pkg):
    E = pkg.engine
    q1 = np.array(list(TC.make_xform(pkg, "rotate").rotate), np.float64)
    q2 = np.array(list(TC.make_xform(pkg, "all").rotate), np.float64)
    r1, r2 = E.xform_prepare(E.xform(rotate=q1)), E.xform_prepare(E.xform(rotate=q2))
    # (the product is handed over in float32: a relative 2^-24 on a unit quaternion, the third of the three roundings the bound allows)
    r12 = E.xform_prepare(E.xform(rotate=TC.quat_mul(q1, q2)))
    for l in (1, 2, 3):
        k = "D%d" % l
        err = float(np.abs(r12[k].astype(np.float64) - r1[k].astype(np.float64) @ r2[k].astype(np.float64)).max())
        print(f"band {l}: max |D(q1 q2) - D(q1) D(q2)| {err:.3e}")
        assert err <= (2 * l + 1) * 3 * U32, (l, err)
    for x in (E.xform(), E.xform(rotate=(0.0, 0.0, 0.0, -3.0)), E.xform(scale=2.0, translate=(1, 2, 3), pivot=(4, 5, 6))):
        ident = E.xform_prepare(x)
        for l in (1, 2, 3):
            assert np.array_equal(ident["D%d" % l], np.eye(2 * l + 1, dtype=np.float32)), l
        assert np.array_equal(ident["A"], np.eye(3, dtype=np.float32) * np.float32(x.scale))


@pytest.mark.parametrize("name", list(TC.TRANSFORMS))
def test_the_rule_is_the_float32_of_the_float64_derivation(pkg, name):
    x = TC.make_xform(pkg, name)
    rule = pkg.engine.xform_prepare(x)
    q = np.array(list(x.rotate), np.float64)
    R, s = TC.quat_matrix(q), float(x.scale)
    piv, tr = np.array(list(x.pivot), np.float64), np.array(list(x.translate), np.float64)
    ulp = lambda v: np.maximum(np.abs(v), 1e-30) * 2.0 ** -23          # (one float32 step: the two float64 derivations may round apart)
    assert (np.abs(rule["A"] - s * R) <= ulp(s * R) + 1e-15).all()
    t = piv + tr - s * R @ piv
    assert (np.abs(rule["t"] - t) <= ulp(t) + 4e-16 * (np.abs(piv) + np.abs(tr) + np.abs(s * R) @ np.abs(piv))).all()
    assert rule["s"] == np.float32(x.scale)
    qn = q / np.linalg.norm(q)
    assert (np.abs(rule["q"] - qn) <= ulp(qn) + 1e-15).all()


# ---- 2. gsr_transform_eval against the float64 model --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.TRANSFORMS))
def test_eval_against_the_float64_model(pkg, name):
    E = pkg.engine
    A = _cloud(pkg)
    x = TC.make_xform(pkg, name)
    rule = E.xform_prepare(x)
    for mname, mask in TC.masks(pkg).items():
        sel = TC.selected(mask)
        out = E.transform_eval(x, A, mask)
        label = f"{name} / {mname}"
        # unselected rows, Cd, alpha and slot 15: bit for bit
        for k in ("P", "scale", "orient", "shx", "shy", "shz"):
            assert np.array_equal(getattr(out, k)[~sel].view(np.uint8), getattr(A, k)[~sel].view(np.uint8)), (label, k)
        assert np.array_equal(out.Cd, A.Cd) and np.array_equal(out.alpha.view(np.uint32), A.alpha.view(np.uint32)), label
        for k in ("shx", "shy", "shz"):
            assert np.array_equal(getattr(out, k)[:, 15], getattr(A, k)[:, 15]), (label, k)
        if not sel.any():
            continue
        # P
        A64, t64, p = rule["A"].astype(np.float64), rule["t"].astype(np.float64), A.P[sel].astype(np.float64)
        v = p @ A64.T + t64
        S = np.abs(p) @ np.abs(A64).T + np.abs(t64)
        assert (np.abs(out.P[sel].astype(np.float64) - v) <= 4 * U32 * S).all(), label
        # scale: one product
        v = float(rule["s"]) * h2f(A.scale[sel])
        assert (np.abs(h2f(out.scale[sel]) - v) <= _half_bound(v, np.abs(v), 1)).all(), label
        # orient: q (x) o, one product under three fmaf
        a, b = rule["q"].astype(np.float64), h2f(A.orient[sel])
        ai, aj, ak, ar = a
        bi, bj, bk, br = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        terms = [(ar * bi, ai * br, aj * bk, -ak * bj), (ar * bj, aj * br, ak * bi, -ai * bk),
                 (ar * bk, ak * br, ai * bj, -aj * bi), (ar * br, -ai * bi, -aj * bj, -ak * bk)]
        v = np.stack([sum(t) for t in terms], axis=1)
        T = np.stack([sum(np.abs(u) for u in t) for t in terms], axis=1)
        assert (np.abs(h2f(out.orient[sel]) - v) <= _half_bound(v, T, 4)).all(), label
        # SH: a chain of 2l + 1 per coefficient
        for k in ("shx", "shy", "shz"):
            v, bound = _sh_model(rule, getattr(A, k)[sel])
            assert (np.abs(h2f(getattr(out, k)[sel])[:, :15] - v) <= bound).all(), (label, k)


def test_eval_changes_what_it_should_and_nothing_else(pkg):
    E = pkg.engine
    A = _cloud(pkg)
    keep = E.transform_eval(E.xform(), A, None)                  # (a copy through the identity: P exactly, halves re-rounded to themselves)
    assert np.array_equal(keep.P, A.P) and np.array_equal(keep.scale, A.scale)
    x = TC.make_xform(pkg, "all")
    before = [getattr(A, k).copy() for k in ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz")]
    out = E.transform_eval(x, A, np.zeros(TC.N, bool))            # no bit set: everything comes back unchanged
    for k, b in zip(("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz"), before):
        assert np.array_equal(getattr(out, k).view(np.uint8), b.view(np.uint8)), k
        assert np.array_equal(getattr(A, k).view(np.uint8), b.view(np.uint8)), k       # the input is never written
    out = E.transform_eval(x, A, None)
    for k in ("P", "scale", "orient", "shx"):
        assert not np.array_equal(getattr(out, k), getattr(A, k)), k
    B = _cloud(pkg, sh=False)
    out = E.transform_eval(x, B, None)                            # a cloud without SH has no SH step
    assert out.shx is None and not np.array_equal(out.P, B.P)


# ---- 3. colour invariance per splat -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.ROTATIONS)
def test_a_rotated_splat_shows_the_colour_it_showed(pkg, name):
    """float64, from the eval'd halves: the SH colour at R d is that of the original halves at d, to within the half-rounding bound of
    test 2 weighted by |Y_m(R d)| and summed over the 15 coefficients, plus the bound of test 1 for the float32 rounding of D per band.
    A transposed or inverted D misses this by orders of magnitude."""
    E = pkg.engine
    A = _cloud(pkg)
    x = TC.make_xform(pkg, name)
    R, rule = _rotation(pkg, name)
    out = E.transform_eval(x, A, None)
    rng = np.random.default_rng(9)
    d = rng.normal(size=(TC.N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Yd = np.concatenate([TC.sh_basis(l, d) for l in (1, 2, 3)], axis=1)
    Yr = np.concatenate([TC.sh_basis(l, d @ R.T) for l in (1, 2, 3)], axis=1)
    worst = 0.0
    for k in ("shx", "shy", "shz"):
        c = h2f(getattr(A, k))[:, :15]
        _, b = _sh_model(rule, getattr(A, k))
        bound = (np.abs(Yr) * b).sum(axis=1) + sum((2 * l + 1) * U32 * TC.basis_max(l) * np.abs(c).max() + 1e-12 for l in (1, 2, 3))
        err = np.abs((Yr * h2f(getattr(out, k))[:, :15]).sum(axis=1) - (Yd * c).sum(axis=1))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (name, k, float(err.max()))
    print(f"{name}: worst colour error / bound = {worst:.3f}")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_gpu(pkg):
    E = pkg.engine
    L = pkg.load_library()
    A = _cloud(pkg, n=8)
    rule = E.gsr_xform_rule()
    arrays = lambda: [a.copy() for a in (A.P, A.scale, A.orient, A.shx, A.shy, A.shz)]
    ptrs = lambda arrs: [a.ctypes.data for a in arrs]

    def bad_transforms():
        for field, k in [("rotate", 0), ("rotate", 3), ("translate", 1), ("pivot", 2)]:
            for v in (np.nan, np.inf, -np.inf):
                x = E.xform()
                getattr(x, field)[k] = v
                yield x, f"{field}[{k}] = {v}"
        for v in (np.nan, np.inf, 0.0, -0.0, -1.0):
            x = E.xform()
            x.scale = v
            yield x, f"scale = {v}"
        yield E.xform(rotate=(0.0, 0.0, 0.0, 0.0)), "a zero quaternion"
        x = E.xform()
        x.reserved_ = 1
        yield x, "reserved_"

    for x, what in bad_transforms():
        assert L.gsr_xform_prepare(C.byref(x), C.byref(rule)) == GSR_E_INVALID, what
        assert b"gsr_xform_prepare" in L.gsr_last_error()
        arrs = arrays()
        assert L.gsr_transform_eval(C.byref(x), 8, None, *ptrs(arrs)) == GSR_E_INVALID, what
        for got, want in zip(arrs, arrays()):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what
        assert L.gsr_transform(None, None, 0, C.byref(x), None) == GSR_E_INVALID, what
    good = E.xform()
    assert L.gsr_xform_prepare(None, C.byref(rule)) == GSR_E_INVALID and L.gsr_xform_prepare(C.byref(good), None) == GSR_E_INVALID
    arrs = arrays()
    assert L.gsr_transform_eval(None, 8, None, *ptrs(arrs)) == GSR_E_INVALID
    assert L.gsr_transform_eval(C.byref(good), -1, None, *ptrs(arrs)) == GSR_E_INVALID
    for drop in (0, 1, 2):                                       # P, scale, orient are all needed
        p = ptrs(arrs)
        p[drop] = None
        assert L.gsr_transform_eval(C.byref(good), 8, None, *p) == GSR_E_INVALID, drop
    p = ptrs(arrs)
    p[4] = None                                                  # two SH arrays of three
    assert L.gsr_transform_eval(C.byref(good), 8, None, *p) == GSR_E_INVALID
    assert L.gsr_transform_eval(C.byref(good), 0, None, None, None, None, None, None, None) == 0     # no rows: nothing to look at
    assert L.gsr_transform(None, None, 0, C.byref(good), None) == GSR_E_INVALID and b"NULL" in L.gsr_last_error()
    assert L.gsr_get_transform(None, None, None, None) == GSR_E_INVALID
    assert L.gsr_multi_transform(None, None, C.byref(good), None) == GSR_E_INVALID
    with pytest.raises(pkg.GsrError):
        E.xform_prepare(E.xform(scale=-2.0))
    with pytest.raises(pkg.GsrError):
        E.transform_eval(E.xform(scale=0.0), A)
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for sym in ("gsr_xform_prepare", "gsr_transform_eval", "gsr_transform", "gsr_get_transform", "gsr_multi_transform"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr), sym
    assert C.sizeof(E.gsr_xform) == 48 and C.sizeof(E.gsr_xform_rule) == 400


def test_python_helpers(pkg):
    E = pkg.engine
    x = E.xform(axis_angle=((0.0, 0.0, 2.0), 90.0))
    assert np.allclose(list(x.rotate), [0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)], atol=1e-7)
    rule = E.xform_prepare(x)
    assert np.allclose(rule["A"], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-7)        # x -> y: a quarter turn about z
    P = np.array([[1.0, 0.0, 0.0]], np.float32)
    s = pkg.scenes.Splats(P, np.zeros((1, 3), np.uint16), np.ones(1, np.float32), np.full((1, 3), 0x3c00, np.uint16),
                          np.array([[0, 0, 0, 0x3c00]], np.uint16))
    out = E.transform_eval(E.xform(axis_angle=((0, 0, 1), 90.0), scale=2.0, translate=(0, 0, 5), pivot=(1, 1, 0)), s)
    assert np.allclose(out.P, [[3.0, 1.0, 5.0]], atol=1e-6)                                  # (1,0,0) - pivot = (0,-1,0) -> 2 (1,0,0) + pivot + t
    assert np.array_equal(out.scale, np.full((1, 3), 0x4000, np.uint16))                     # 2.0
    assert np.allclose(h2f(out.orient), [[0, 0, np.sqrt(0.5), np.sqrt(0.5)]], atol=1e-3)


# ---- 5. the kernel uses no scratch ------------------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): neither instantiation of k_transform spills,
    the SH one keeps k_update's LDS rows (64 rows of 112 bytes) and the plain one has none"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    for prefix, lds_max in (("_Z11k_transformILb0E", 0), ("_Z11k_transformILb1E", 64 * 112), ("_Z12k_mask_count", 0)):
        hit = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, sorted(rows))
        vg, sg, lds, scratch = hit[0]
        print(f"{prefix}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0 and lds <= lds_max, (prefix, hit[0])
