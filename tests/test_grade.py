"""gsr_grade on the host: the rule gsr_grade_prepare derives, and gsr_grade_eval -- the functions the kernel evaluates -- against a numpy
float64 model.  No GPU.  (tests/test_grade_gpu.py holds the kernel and the verb to gsr_grade_eval bit for bit.)

The bounds, all derived from the number formats (u32 = 2^-24: one float32 rounding, relative; u16 = 2^-11: one binary16 rounding), in
tests/test_transform.py's form:
  a half  h = f2h(chain): |h2f(h) - v| <= u16 |v| + 3 u32 T  (+ 2^-24 where |v| < 2^-14: the absolute spacing of half subnormals), with
          v the float64 value of the chain from the float32 rule and the input halves, T the sum of the magnitudes of its terms
          (|M_r0 R| + |M_r1 G| + |M_r2 B| + |b_r|), and 3 its length in float32 roundings (one product or fmaf under two fmaf)
  alpha   one fmaf: |alpha' - clamp(ag a + ab)| <= u32 (|ag a| + |ab|) (the clamp moves no two values apart)
  a rule  each entry is a float64 value rounded to float32 once; the test's own float64 composition may round apart from the library's
          by one float32 step

The kernel kept is the REGISTER form (no LDS): test_kernel_resources holds both instantiations to 0 bytes of LDS and of scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import grade_cases as GC
import transform_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
U32, U16 = 2.0 ** -24, 2.0 ** -11
ARRAYS = ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz")


def h2f(a):
    return np.ascontiguousarray(a, np.uint16).view(np.float16).astype(np.float64)


def _half_bound(v, T, length):
    v, T = np.asarray(v, np.float64), np.asarray(T, np.float64)
    return U16 * np.abs(v) + length * U32 * T + np.where(np.abs(v) < 2.0 ** -14, 2.0 ** -24, 0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _triples(s):
    """float64 (n, 16, 3): coefficient 0 = Cd, 1..15 = slots 0..14 of the SH rows, channels last; None without SH: (n, 1, 3)"""
    cd = h2f(s.Cd)[:, None, :]
    if s.shx is None:
        return cd
    sh = np.stack([h2f(s.shx)[:, :15], h2f(s.shy)[:, :15], h2f(s.shz)[:, :15]], axis=2)
    return np.concatenate([cd, sh], axis=1)


def _colour_model(rule, s):
    """(v, bound), float64 (n, 16 or 1, 3): every coefficient through M, Cd with b, from the float32 rule and the input halves"""
    M, b = rule["M"].astype(np.float64), rule["b"].astype(np.float64)
    c = _triples(s)
    v = c @ M.T
    T = np.abs(c) @ np.abs(M).T
    v[:, 0] += b
    T[:, 0] += np.abs(b)
    return v, _half_bound(v, T, 3)


# ---- 1. prepare -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.PARAMS))
def test_the_rule_is_the_float32_of_the_float64_composition(pkg, name):
    rule = GC.make_rule(pkg, name)
    M, b = GC.compose64(**GC.PARAMS[name])
    ulp = lambda v: np.maximum(np.abs(v), 2.0 ** -126) * 2.0 ** -23     # (one float32 step: the two float64 derivations may round apart)
    assert rule["M"].shape == (3, 3) and rule["b"].shape == (3,)
    assert (np.abs(rule["M"].astype(np.float64) - M) <= ulp(M)).all(), (name, rule["M"], M)
    assert (np.abs(rule["b"].astype(np.float64) - b) <= ulp(b) + 1e-16).all(), (name, rule["b"], b)
    p = GC.PARAMS[name]
    assert rule["ag"] == np.float32(p.get("alpha_gain", 1.0)) and rule["ab"] == np.float32(p.get("alpha_offset", 0.0))
    assert rule["flags"] == GC.FLAGS[name], name


def test_neutral_parameters_and_own_matrices(pkg):
    E = pkg.engine
    rule = E.grade_prepare(E.grade_params())
    assert rule["flags"] == 0 and np.array_equal(rule["M"], np.eye(3, dtype=np.float32)) and not rule["b"].any()
    assert E.grade_prepare(E.grade_params(pivot=0.2, contrast=1.0))["flags"] == 0          # any pivot is neutral under contrast 1
    assert E.grade_prepare(E.grade_params(alpha_offset=1e-3))["flags"] == GC.GRADE_ALPHA
    swap = GC.make_rule(pkg, "channel_swap")
    assert swap["flags"] == GC.GRADE_COLOUR and np.array_equal(swap["M"], np.asarray(GC.MATRICES["channel_swap"], np.float32))
    assert E.grade_rule(np.eye(3))["flags"] == 0
    assert E.grade_rule(np.eye(3), b=(0.0, 0.1, 0.0), alpha_gain=0.5)["flags"] == GC.GRADE_COLOUR | GC.GRADE_ALPHA
    m2 = E.grade_prepare(E.grade_params(exposure=1.0))["M"]
    assert np.array_equal(m2, 2.0 * np.eye(3, dtype=np.float32))                            # exact, its zeros included


def test_refusals_need_no_gpu(pkg):
    E = pkg.engine
    L = pkg.load_library()
    out = E.gsr_grade_rule()
    for field, k in [("exposure", None), ("gain", 1), ("saturation", None), ("contrast", None), ("pivot", None), ("offset", 2),
                     ("alpha_gain", None), ("alpha_offset", None)]:
        for v in (np.nan, np.inf, -np.inf):
            p = E.grade_params()
            if k is None:
                setattr(p, field, v)
            else:
                getattr(p, field)[k] = v
            assert L.gsr_grade_prepare(C.byref(p), C.byref(out)) == GSR_E_INVALID, (field, v)
            assert b"gsr_grade_prepare" in L.gsr_last_error()
    assert L.gsr_grade_prepare(C.byref(E.grade_params(exposure=200.0)), C.byref(out)) == GSR_E_INVALID      # 2^200 is no float32
    good = E.grade_params(exposure=1.0)
    assert L.gsr_grade_prepare(None, C.byref(out)) == GSR_E_INVALID and L.gsr_grade_prepare(C.byref(good), None) == GSR_E_INVALID
    assert L.gsr_grade_prepare(C.byref(good), C.byref(out)) == 0
    # gsr_grade_eval: a rule with an unknown flag bit or a float that is not finite, and arrays that are missing
    A = GC.cloud(pkg, n=8)
    arrays = lambda: [a.copy() for a in (A.Cd, A.alpha, A.shx, A.shy, A.shz)]
    ptrs = lambda arrs: [a.ctypes.data for a in arrs]

    def bad_rules():
        r = E._grade_rule_struct(GC.make_rule(pkg, "all"))
        r.flags = 4
        yield r, "an unknown flag bit"
        for field, k in (("M", 4), ("b", 0), ("ag", None), ("ab", None)):
            for v in (np.nan, np.inf):
                r = E._grade_rule_struct(GC.make_rule(pkg, "all"))
                if k is None:
                    setattr(r, field, v)
                else:
                    getattr(r, field)[k] = v
                yield r, f"{field} = {v}"

    for r, what in bad_rules():
        arrs = arrays()
        assert L.gsr_grade_eval(C.byref(r), 8, None, 1, *ptrs(arrs)) == GSR_E_INVALID, what
        assert b"gsr_grade_eval" in L.gsr_last_error()
        for got, want in zip(arrs, arrays()):
            assert np.array_equal(_bits(got), _bits(want)), what
        assert L.gsr_grade(None, None, 0, C.byref(r), None) == GSR_E_INVALID, what
    r = E._grade_rule_struct(GC.make_rule(pkg, "all"))
    arrs = arrays()
    assert L.gsr_grade_eval(None, 8, None, 1, *ptrs(arrs)) == GSR_E_INVALID
    assert L.gsr_grade_eval(C.byref(r), -1, None, 1, *ptrs(arrs)) == GSR_E_INVALID
    for drop in (0, 1, 3):                                       # Cd, alpha, one SH array of three
        p = ptrs(arrs)
        p[drop] = None
        assert L.gsr_grade_eval(C.byref(r), 8, None, 1, *p) == GSR_E_INVALID, drop
    assert L.gsr_grade_eval(C.byref(r), 0, None, 1, None, None, None, None, None) == 0       # no rows: nothing to look at
    assert L.gsr_grade(None, None, 0, C.byref(r), None) == GSR_E_INVALID and b"NULL" in L.gsr_last_error()
    assert L.gsr_get_grade(None, None, None, None) == GSR_E_INVALID
    assert L.gsr_multi_grade(None, None, C.byref(r), None) == GSR_E_INVALID
    with pytest.raises(pkg.GsrError):
        E.grade_prepare(E.grade_params(saturation=np.nan))
    bad = GC.make_rule(pkg, "all")
    bad["M"][1, 1] = np.nan
    with pytest.raises(pkg.GsrError):
        E.grade_eval(bad, A)


# ---- 2. gsr_grade_eval against the float64 model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", (True, False))
@pytest.mark.parametrize("name", GC.RULES)
def test_eval_against_the_float64_model(pkg, name, sh):
    E = pkg.engine
    A = GC.cloud(pkg, sh=sh)
    rule = GC.make_rule(pkg, name)
    colour, alph = rule["flags"] & GC.GRADE_COLOUR, rule["flags"] & GC.GRADE_ALPHA
    before = {k: None if getattr(A, k) is None else getattr(A, k).copy() for k in ARRAYS}
    v_all, bound_all = _colour_model(rule, A)
    ag, ab = float(rule["ag"]), float(rule["ab"])
    a64 = A.alpha.astype(np.float64)
    worst = 0.0
    for mname, mask in GC.masks(pkg).items():
        sel = GC.selected(mask)
        out = E.grade_eval(rule, A, mask)
        label = f"{name} / {mname} sh {sh}"
        assert (out.shx is None) == (not sh), label
        for k in ARRAYS:                                         # the input is never written; P, scale, orient and unselected rows: bit for bit
            if before[k] is None:
                continue
            assert np.array_equal(_bits(getattr(A, k)), _bits(before[k])), (label, k)
            keep = slice(None) if k in ("P", "scale", "orient") else ~sel
            assert np.array_equal(_bits(getattr(out, k)[keep]), _bits(before[k][keep])), (label, k)
        if sh:
            for k in ("shx", "shy", "shz"):
                assert np.array_equal(getattr(out, k)[:, 15], before[k][:, 15]), (label, k, "slot 15")
        if not colour:
            for k in ("Cd", "shx", "shy", "shz"):
                assert before[k] is None or np.array_equal(getattr(out, k), before[k]), (label, k, "the colour step did not run")
        if not alph:
            assert np.array_equal(_bits(out.alpha), _bits(before["alpha"])), (label, "the alpha step did not run")
        if not sel.any():
            continue
        if colour:
            err = np.abs(_triples(out)[sel] - v_all[sel])
            worst = max(worst, float((err / bound_all[sel]).max()))
            assert (err <= bound_all[sel]).all(), (label, float((err / bound_all[sel]).max()))
        if alph:
            want = np.clip(ag * a64[sel] + ab, 0.0, 1.0)
            err = np.abs(out.alpha[sel].astype(np.float64) - want)
            assert (err <= U32 * (np.abs(ag * a64[sel]) + abs(ab))).all(), (label, float(err.max()))
            assert (out.alpha[sel] >= 0.0).all() and (out.alpha[sel] <= 1.0).all(), label
    if colour:
        changed = E.grade_eval(rule, A, None)
        assert not np.array_equal(changed.Cd, A.Cd), f"{name}: the rule changes no Cd half: the case tests nothing"
    if name == "alpha_lift":
        assert (E.grade_eval(rule, A, None).alpha == 1.0).any(), "alpha_lift does not reach the clamp: the case tests nothing"
    print(f"{name} sh {sh}: worst colour error / bound = {worst:.3f}")


def test_alpha_edge_values(pkg):
    E = pkg.engine
    A = GC.cloud(pkg, n=8)
    A.alpha[:] = np.array([np.nan, -0.0, 0.0, 1.0, 2.0, -1.0, np.inf, 0.5], np.float32)
    out = E.grade_eval(E.grade_rule(np.eye(3), alpha_gain=0.5), A).alpha
    assert np.array_equal(out.view(np.uint32), np.array([0.0, 0.0, 0.0, 0.5, 1.0, 0.0, 1.0, 0.25], np.float32).view(np.uint32))


# ---- 3. the colour in front of the clamp is mapped affinely ---------------------------------------------------------------------------
def test_the_colour_before_the_clamp_is_mapped_affinely(pkg):
    """float64, from the eval'd halves and 200 random unit directions: Cd' + sum_k Y_k(d) sh'_k = M (Cd + sum_k Y_k(d) sh_k) + b per
    channel, to within sum_k |Y_k(d)| times the half bound of each coefficient (Y_0 = 1 for Cd) -- derived, not measured.  A map that
    put b on an SH coefficient or mixed coefficients misses this by orders of magnitude."""
    E = pkg.engine
    A = GC.cloud(pkg)
    rule = GC.make_rule(pkg, "all")
    out = E.grade_eval(rule, A, None)
    M, b = rule["M"].astype(np.float64), rule["b"].astype(np.float64)
    v, bound = _colour_model(rule, A)
    rng = np.random.default_rng(9)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = np.concatenate([np.ones((200, 1))] + [TC.sh_basis(l, d) for l in (1, 2, 3)], axis=1)     # (200, 16)
    before = np.einsum("dk,nkc->ndc", Y, _triples(A))            # (n, 200, 3): the colour in front of the clamp
    after = np.einsum("dk,nkc->ndc", Y, _triples(out))
    want = before @ M.T + b
    limit = np.einsum("dk,nkc->ndc", np.abs(Y), bound)
    err = np.abs(after - want)
    print(f"worst |colour - (M colour + b)| / bound = {float((err / limit).max()):.3f}, max |err| {float(err.max()):.3e}")
    assert (err <= limit + 1e-12).all(), float((err / limit).max())
    assert float(np.abs(after - before).max()) > 1e-2, "the rule changes no colour: the case tests nothing"


# ---- 4. exactness ---------------------------------------------------------------------------------------------------------------------
def test_channel_swap_twice_is_the_identity(pkg):
    E = pkg.engine
    rule = GC.make_rule(pkg, "channel_swap")
    for sh in (True, False):
        A = GC.cloud(pkg, sh=sh)
        once = E.grade_eval(rule, A, None)
        assert np.array_equal(once.Cd[:, 0], A.Cd[:, 2]) and np.array_equal(once.Cd[:, 2], A.Cd[:, 0]) and np.array_equal(once.Cd[:, 1], A.Cd[:, 1])
        if sh:
            assert np.array_equal(once.shx[:, :15], A.shz[:, :15]) and np.array_equal(once.shz[:, :15], A.shx[:, :15])
        twice = E.grade_eval(rule, once, None)
        for k in ARRAYS:
            if getattr(A, k) is not None:
                assert np.array_equal(_bits(getattr(twice, k)), _bits(getattr(A, k))), (sh, k)


def test_exposure_up_then_down_restores_the_halves(pkg):
    """M = 2 I then M = I / 2: every half that is normal and below half the largest half comes back bit for bit"""
    E = pkg.engine
    A = GC.cloud(pkg)
    up, down = GC.make_rule(pkg, "exposure +1"), GC.make_rule(pkg, "exposure -1")
    back = E.grade_eval(down, E.grade_eval(up, A, None), None)
    held = 0
    for k in ("Cd", "shx", "shy", "shz"):
        a, r = getattr(A, k), getattr(back, k)
        mag = np.abs(h2f(a))
        ok = (mag >= 2.0 ** -14) & (mag < 65504.0 / 2.0)
        if k != "Cd":
            ok[:, 15] = False
        held += int(ok.sum())
        assert np.array_equal(r[ok], a[ok]), k
    assert held > 0.9 * GC.N * 48, "few halves are normal: the case tests little"


# ---- 5. the structs ---------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_symbols(pkg):
    E = pkg.engine
    L = pkg.load_library()
    assert C.sizeof(E.gsr_grade_rule) == 15 * 4 and C.sizeof(E.gsr_grade_params) == 12 * 4
    assert E.gsr_grade_rule.b.offset == 36 and E.gsr_grade_rule.ag.offset == 48 and E.gsr_grade_rule.flags.offset == 56
    assert E.gsr_grade_params.offset.offset == 28 and E.gsr_grade_params.alpha_offset.offset == 44
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for sym in ("gsr_grade_prepare", "gsr_grade_eval", "gsr_grade", "gsr_get_grade", "gsr_multi_grade"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr), sym
    edit = open(os.path.join(ROOT, "houdini-gsplat-renderer_amd", "csrc", "gsr_resident_edit.h")).read()
    assert re.search(r"static_assert\(sizeof\(gsr_grade_rule\) == sizeof\(GsrGradeRule\)", edit), "the public rule is held to the kernel's at compile time"
    p = E.grade_params()
    assert (p.exposure, list(p.gain), p.saturation, p.contrast, list(p.offset), p.alpha_gain, p.alpha_offset) == (0.0, [1.0] * 3, 1.0, 1.0, [0.0] * 3, 1.0, 0.0)


# ---- 6. the kernels' resources ------------------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): each instantiation of k_grade appears once,
    spills nothing, and -- the REGISTER form is the one kept -- has no LDS"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    for prefix in ("_Z7k_gradeILb0E", "_Z7k_gradeILb1E"):
        hit = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, sorted(rows))
        vg, sg, lds, scratch = hit[0]
        print(f"{prefix}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0 and lds == 0, (prefix, hit[0])
