"""A float64 model of what the cluster cull reads: the extent half of geoB and the two cluster planes.  The rules are
restated from csrc/k_resident.h (gsr_extent_half, gsr_lane_bounds, gsr_cluster_fold); tests/test_cull_edges.py holds the model to
brute force on the CPU, tests/test_cluster_bounds_gpu.py holds the upload, device-upload and update kernels to the model.

  extent_bracket   the halves the stored extent bound may take for a slot's seven halves
  cluster_planes   clusA / clusB of a storage-ordered cloud
  bounds_cloud     the 5 x 64 + 17 splats whose halves and positions reach every edge of both rules

THE EXTENT HALF.  gsr_extent_half forms the nine entries of R(q) in float32 (products of two halves are exact in float32, so each entry
is one rounded fma, then a doubling and for the diagonal a subtraction from 1: f32_rotation below does exactly that, with exact
rational arithmetic), then

    mf2 = sx^2 (r00^2 + r10^2 + r20^2) + sy^2 (r01^2 + r11^2 + r21^2) + sz^2 (r02^2 + r12^2 + r22^2),   mfv = sqrt(mf2) * 1.001f

in float32 with -ffp-contract=off (csrc/build.py), and stores the smallest half >= mfv (+inf above 65504): mf = ceil_half(mfv).  The
model forms F = sqrt(sum_p s_p^2 sum_r R_rp^2) from the SAME float32 entries, in exact arithmetic, and bounds mfv around F * 1.001f.

DELTA, the relative error of the float32 chain.  u = 2^-24.  Every one of the nine terms s_p^2 R_rp^2 is non-negative and passes through
at most six roundings before it is summed: its square (1), the two additions of its column (2; s_p^2 is exact), the product with s_p^2
(1), the two additions of the columns (2).  With non-negative terms the computed mf2 is mf2 (1 + t), |t| <= gamma_6 = 6u / (1 - 6u)
(Higham, Accuracy and Stability, Lemma 3.1 and 3.3).  The square root halves that: sqrt(1 + t) lies within 1 +- gamma_3.  The square
root itself may be one ulp off (2u: gamma_2 covers it, also for a square root that is not correctly rounded), and the product with 1.001f
is rounded once (gamma_1).  (1 + gamma_j)(1 + gamma_k) <= 1 + gamma_(j+k), so

    F * 1.001f * (1 - DELTA) <= mfv <= F * 1.001f * (1 + DELTA),   DELTA = gamma_6 + 2^-50 ~ 3.6e-7 ~ 2^-21.4

where 2^-50 covers the model's own float64 square root.  That holds while no product underflows into float32's subnormal range; each of
the nine terms then loses at most 2^-149 per rounding, at most 2^-143 in all, and F at most sqrt(2^-143) < 2^-70: both ends of the
bracket widen by ABS_SLACK = 2^-70, far below the smallest half (2^-24).  F == 0 means every term is an exact zero: mfv = 0, mf = +0.
ceil_half is monotone, so ceil_half of the two ends bracket mf.  A slot with an inf or NaN among its seven halves has no bracket: its
mf must not be < 6e4 (the "never cull" flag of gsr_lane_bounds).
"""
import math
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
DELTA = 6 * U32 / (1 - 6 * U32) + 2.0 ** -50
ABS_SLACK = 2.0 ** -70
C1001 = float(np.float32(1.001))         # the constant 1.001f
FLAG_MF = 6.0e4                          # !(mf < 6e4): never cull
FLAG_POS = np.float32(3.0e38)            # !(|x| < 3e38): never cull
FOLD_START = np.float32(3.0e38)          # GsrClusterIn: lo from +3e38, hi from -3e38, mf from 0
CLUSTER = 64

HALF_MAX = 65504.0


def h2f(bits):
    """uint16 half bits -> float64 (exact)"""
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def f2h(x):
    """float64 -> half bits, round to nearest even (v_cvt_f16_f32 of a value that is already a float32)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).view(np.uint16)


def ceil_half(x: float) -> float:
    """the smallest half >= x (x >= 0, finite), +inf above 65504"""
    x = float(x)
    if x > HALF_MAX:
        return math.inf
    with np.errstate(over="ignore"):
        h = np.float16(x)                  # (float64 -> float16 directly: one rounding)
    if float(h) < x:
        h = np.nextafter(h, np.float16(np.inf))
    return float(h)


def f32_round(q: Fraction) -> float:
    """the float32 nearest to the rational q, ties to even (q is well inside float32's normal range or zero)"""
    if q == 0:
        return 0.0
    a = np.float32(float(q))              # within one float32 step of the answer
    best = None
    for c in (np.nextafter(a, np.float32(-np.inf)), a, np.nextafter(a, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - q)
        if best is None or d < best[0] or (d == best[0] and (int(c.view(np.uint32)) & 1) == 0):
            best = (d, c)
    return float(best[1])


def f32_rotation(qi, qj, qk, qr):
    """the nine float32 entries gsr_extent_half forms from four finite halves (as float64 values), row-major r[row][col]"""
    Q = [Fraction(float(v)) for v in (qi, qj, qk, qr)]
    qi, qj, qk, qr = Q

    def fma(a, b, c):                     # c is an exact product of two halves
        return f32_round(a * b + c)

    def diag(a, b):                       # 1 - 2 fma(a, a, b * b): the doubling is exact, the subtraction rounds once
        return f32_round(1 - 2 * Fraction(fma(a, a, b * b)))

    off = lambda v: 2.0 * v              # (2 * a float32 is exact here: |entries| < 2^34)
    return [[diag(qj, qk), off(fma(qi, qj, -(qr * qk))), off(fma(qi, qk, qr * qj))],
            [off(fma(qi, qj, qr * qk)), diag(qi, qk), off(fma(qj, qk, -(qr * qi)))],
            [off(fma(qi, qk, -(qr * qj))), off(fma(qj, qk, qr * qi)), diag(qi, qj)]]


def extent_F(shape_bits):
    """F = sqrt(sum_p s_p^2 sum_r R_rp^2) for seven finite halves (sx, sy, sz, qi, qj, qk, qr), or None if one is not finite"""
    v = h2f(np.asarray(shape_bits, np.uint16))
    if not np.isfinite(v).all():
        return None
    R = f32_rotation(*v[3:])
    f2 = sum(Fraction(float(v[p])) ** 2 * sum(Fraction(R[r][p]) ** 2 for r in range(3)) for p in range(3))
    return math.sqrt(f2)


def extent_bracket(shape_bits):
    """(lo, hi): the values the stored extent half may take, or None where only !(mf < 6e4) is promised"""
    F = extent_F(shape_bits)
    if F is None:
        return None
    if F == 0.0:
        return 0.0, 0.0
    a = F * C1001
    return ceil_half(max(a * (1 - DELTA) - ABS_SLACK, 0.0)), ceil_half(a * (1 + DELTA) + ABS_SLACK)


def mfv_f32(sx, sy, sz):
    """mfv for the identity quaternion, in numpy float32 in the kernel's op order (R = I exactly: every column sum is 1)"""
    f = np.float32
    one = f(1.0)
    mf2 = (f(sx) * f(sx)) * one + (f(sy) * f(sy)) * one
    mf2 = mf2 + (f(sz) * f(sz)) * one
    return np.sqrt(mf2) * f(C1001)


def cluster_planes(P, mf, n):
    """clusA, clusB (float32 [nclus, 4]) of a storage-ordered cloud: P float32 [>= n, 3] and mf (the extent halves as float) [>= n]
    by storage slot; slots >= n do not count"""
    P = np.asarray(P, np.float32)[:n]
    mf = np.asarray(mf, np.float32)[:n]
    nclus = (n + CLUSTER - 1) // CLUSTER
    A = np.empty((nclus, 4), np.float32)
    B = np.empty((nclus, 4), np.float32)
    for c in range(nclus):
        p, m = P[c * CLUSTER:(c + 1) * CLUSTER], mf[c * CLUSTER:(c + 1) * CLUSTER]
        with np.errstate(invalid="ignore"):
            A[c, :3] = np.fmin.reduce(np.vstack([np.full((1, 3), FOLD_START), p]), axis=0)     # (fmin drops a NaN operand)
            B[c, :3] = np.fmax.reduce(np.vstack([np.full((1, 3), -FOLD_START), p]), axis=0)
            A[c, 3] = np.fmax.reduce(np.concatenate([[np.float32(0.0)], m]))
            bad = (~(np.abs(p) < FLAG_POS)).any() or (~(m < np.float32(FLAG_MF))).any()
        B[c, 3] = 1.0 if bad else 0.0
    return A, B


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
N_BOUNDS = 5 * CLUSTER + 17
SCALE_EDGES = {"0": 0x0000, "-0": 0x8000, "2^-24": 0x0001, "2^-14": 0x0400, "65504": 0x7bff, "-65504": 0xfbff, "+inf": 0x7c00,
               "nan": 0x7e00}


def _quats():
    """(name, (i, j, k, r) float64): every quaternion edge the extent half must survive"""
    c, s = math.cos(math.pi / 8), math.sin(math.pi / 8)
    return [("zero", (0, 0, 0, 0)), ("identity", (0, 0, 0, 1)), ("45 x", (s, 0, 0, c)), ("45 y", (0, s, 0, c)), ("45 z", (0, 0, s, c)),
            ("0.7071 i", (0.7071, 0, 0, 0)), ("0.7071 j", (0, 0.7071, 0, 0)), ("0.7071 k", (0, 0, 0.7071, 0)),
            ("0.7071 i r", (0.7071, 0, 0, 0.0002)), ("all 65504", (65504.0,) * 4), ("all 1e-3", (1e-3,) * 4)]


QUATS = _quats()
_HALVES = None


def _finite_halves():
    global _HALVES
    if _HALVES is None:
        b = np.arange(0x0000, 0x7c00, dtype=np.uint16)
        _HALVES = (b, b.view(np.float16).astype(np.float32))
    return _HALVES


def solve_probe(target):
    """halves (sx, sy, sz) with the identity quaternion for which mfv_f32 == target (a float32), found by search: sx from the halves
    just below target / 1.001, sy over every finite half below sx, then sz likewise"""
    bits, vals = _finite_halves()
    t = np.float32(target)
    base = float(t) / C1001
    i0 = int(np.searchsorted(vals, np.float32(base)))
    for ix in range(max(i0 - 1, 0), max(i0 - 40, 0), -1):
        sx = vals[ix]
        sy = vals[vals <= sx]
        with np.errstate(over="ignore"):
            got = mfv_f32(sx, sy, np.float32(0.0))
        hit = np.nonzero(got == t)[0]
        if hit.size:
            return int(bits[ix]), int(bits[hit[-1]]), 0
        # (a third axis for the targets the first two cannot reach)
        for iy in np.nonzero(np.abs(got.astype(np.float64) - float(t)) <= 64 * abs(float(np.spacing(t))))[0][-8:]:
            with np.errstate(over="ignore"):
                got3 = mfv_f32(sx, vals[iy], vals[vals <= vals[iy]])
            hit = np.nonzero(got3 == t)[0]
            if hit.size:
                return int(bits[ix]), int(bits[iy]), int(bits[hit[-1]])
    raise AssertionError(f"no halves land mfv on {float(t)!r}")


# (half value H, float32 steps from it): the probes that land mfv one float32 step and sixteen (beyond DELTA) below and above a half;
# 59968 / 60000 are the halves on either side of the 6e4 flag, 65504 the last finite one
PROBE_HALVES = (1.0, 0.0999755859375, 59968.0, 60000.0, 65504.0)
PROBE_STEPS = (-16, -1, 1, 16)


def probe_targets():
    out = []
    for H in PROBE_HALVES:
        for k in PROBE_STEPS:
            t = np.float32(H)
            for _ in range(abs(k)):
                t = np.nextafter(t, np.float32(np.inf if k > 0 else -np.inf))
            out.append((H, k, t))
    return out


_PROBES = None


def probes():
    """[(H, k, target, (sx, sy, sz) bits)], solved once"""
    global _PROBES
    if _PROBES is None:
        _PROBES = [(H, k, t, solve_probe(t)) for H, k, t in probe_targets()]
    return _PROBES


def bounds_cloud(seed, scenes):
    """N_BOUNDS splats (a scenes.Splats) whose halves and positions reach every edge of the extent half and of the cluster fold; a
    second seed puts the edges on other splats, and so into other clusters"""
    rng = np.random.default_rng(seed)
    n = N_BOUNDS
    s = scenes.make_scene(n, seed=seed, sh=False, log_scale_range=(-4.0, -1.0))
    order = rng.permutation(n)            # rows the edges go to
    at = iter(order.tolist())
    q = f2h(np.array([v for _, v in QUATS]))
    # every scale edge on every axis, each with a quaternion of the list
    for name, hb in SCALE_EDGES.items():
        for ax in range(3):
            i = next(at)
            s.scale[i, ax] = hb
            s.orient[i] = q[(ax + len(name)) % len(QUATS)]
    # every quaternion, with a random scale and with the largest finite one
    for k in range(len(QUATS)):
        for big in (False, True):
            i = next(at)
            s.orient[i] = q[k]
            if big:
                s.scale[i] = 0x7bff
    # the rounding probes (identity quaternion)
    ident = f2h(np.array([0.0, 0.0, 0.0, 1.0]))
    for _, _, _, sb in probes():
        i = next(at)
        s.scale[i] = np.array(sb, np.uint16)[rng.permutation(3)]
        s.orient[i] = ident
    # inf / NaN in a quaternion
    for hb in (0x7c00, 0xfe00):
        i = next(at)
        s.orient[i, rng.integers(4)] = hb
    # the positions: a NaN coordinate, an inf, one beyond 3e38, a -0
    for ax, v in enumerate((np.nan, np.inf, 3.1e38)):
        s.P[next(at), ax] = np.float32(v)
    s.P[next(at), 1] = np.float32(-0.0)
    return s
