"""A background on the CPU: gsr_composite_over -- the rule the blend kernel's epilogue composites with, on the host -- against a
numpy restatement bit for bit; the verb's argument checks; the struct's layout; the over-kernels' budgets.  The GPU path is held
to gsr_composite_over in test_background_gpu.py.

The rule (include/gsplat_hip.h, "background"):  k = 1.0f - B_a;  out_c = fmaf(k, S_c, B_c);  then the target format's store."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
f32 = np.float32


def fma32(a, b, c):
    """a correctly rounded float32 fma(a, b, c) of float32 arrays, through float64 and ROUND TO ODD.
    The product of two float32 values has 48 significant bits: exact in float64.  The sum p + c is not (the addend may lie far
    below the product), and rounding it to float64 and then to float32 rounds twice.  So the float64 sum is made a round-to-odd one:
    TwoSum gives the exact residual err of s = fl(p + c); if err != 0 the exact sum lies strictly between s and its neighbour on
    err's side, and of those two the one with an odd last bit is taken.  A round-to-odd result with at least two bits more than the
    target format (float64 has 29 more than float32) rounds to the target exactly as the exact sum does (Boldo & Melquiond 2008).
    np.longdouble would not do: its 64 bits hold the product but not every sum, and it is float64 on some platforms."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    need = (err != 0) & even & np.isfinite(s)
    s = np.where(need, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def decode(img):
    if img.dtype == np.uint8:
        return img.astype(np.float32) / f32(255.0)           # (float32 / float32: one IEEE division)
    return img.astype(np.float32)                             # (binary16 -> float32 is exact)


def store(px, fmt):
    if fmt == 0:
        return px
    if fmt == 1:
        with np.errstate(over="ignore"):
            return px.astype(np.float16)                      # (round to nearest even, overflow to infinity)
    c = np.where(px > 0, px, f32(0))                          # (NaN -> 0)
    c = np.where(c < 1, c, f32(1))
    # fmaf(c, 255, 0.5): a 24-bit times an 8-bit value plus 0.5 is exact in float64, so ONE rounding to float32; then truncation
    return (c.astype(np.float64) * 255.0 + 0.5).astype(np.float32).astype(np.uint8)


def rule(S, B, fmt):
    """S, B: float32 [..., 4] (B broadcasts)"""
    B = np.broadcast_to(B, S.shape)
    k = (f32(1.0) - B[..., 3:4]).astype(np.float32)           # one float32 subtraction
    return store(fma32(np.broadcast_to(k, S.shape), S, B), fmt)


def _ulp_neighbours(x, dtype):
    x = np.asarray(x, dtype)
    return np.stack([np.nextafter(x, dtype(-np.inf)), x, np.nextafter(x, dtype(np.inf))], -1).reshape(-1)


def _frame(n=6000, seed=4):
    """premultiplied random pixels, a fifth of them S = 0, and -- so that results fall on both sides of the stores' rounding
    boundaries -- channels at the float32 neighbours of byte boundaries (n + 0.5) / 255 and of binary16 midpoints"""
    rng = np.random.default_rng(seed)
    a = rng.random(n).astype(np.float32)
    S = (rng.random((n, 4)).astype(np.float32) * a[:, None]).astype(np.float32)
    S[:, 3] = a
    S[rng.random(n) < 0.2] = 0
    bytes_ = _ulp_neighbours((np.arange(0, 255, 7, dtype=np.float64) + 0.5) / 255.0, np.float32)
    h = np.linspace(0.01, 0.99, 40).astype(np.float16)
    mids = _ulp_neighbours((h.astype(np.float64) + np.nextafter(h, np.float16(np.inf)).astype(np.float64)) / 2, np.float32)
    edge = np.concatenate([bytes_, mids]).astype(np.float32)
    E = np.repeat(edge[:, None], 4, 1)
    return np.concatenate([S, E]).astype(np.float32), len(S)


def _backgrounds(n, n_rand, seed=9):
    """{name: colour tuple or image [n, 4]}: alpha in {0, 0.4, 1} (the float32 nearest 0.4 survives all three formats' decode only in
    f32; the f16 / u8 images hold their own nearest values), premultiplied random colour; the edge pixels of the frame sit over
    alpha 0 and colour 0 (out = S there: the stores' boundaries are hit), and some S = 0 pixels over boundary-valued B"""
    rng = np.random.default_rng(seed)
    alpha = rng.choice(np.array([0.0, 0.4, 1.0], np.float32), n)
    col = (rng.random((n, 3)).astype(np.float32) * alpha[:, None]).astype(np.float32)
    img = np.concatenate([col, alpha[:, None]], 1).astype(np.float32)
    img[n_rand:] = 0
    with np.errstate(over="ignore"):
        return {"colour": (0.1, 0.2, 0.3, 0.5), "f32": img, "f16": img.astype(np.float16),
                "u8": np.clip(np.rint(img.astype(np.float64) * 255), 0, 255).astype(np.uint8)}


def test_fma_restatement_is_correctly_rounded():
    """the round-to-odd fma against exact rational arithmetic: the result is at least as close to the exact value as both of its
    float32 neighbours (ties: the even one)"""
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.random(300), [1.0, 0.6, 2.0 ** -20, 1.0 - 2.0 ** -24]]).astype(np.float32)
    b = np.concatenate([rng.random(300), [0.3, 0.33333334, 1.0, 1.0 - 2.0 ** -24]]).astype(np.float32)
    c = np.concatenate([rng.random(300) * rng.choice([1.0, 2.0 ** -12, 2.0 ** -30], 300), [0.1, 2.0 ** -40, 0.5, 2.0 ** -25]]).astype(np.float32)
    r = fma32(a, b, c)
    for x, y, z, got in zip(a, b, c, r):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        d = abs(Fraction(float(got)) - exact)
        for nb in (np.nextafter(got, f32(np.inf)), np.nextafter(got, f32(-np.inf))):
            dn = abs(Fraction(float(nb)) - exact)
            assert d < dn or (d == dn and (int(np.float32(got).view(np.uint32)) & 1) == 0), (x, y, z, got)
    # ... and it is not what two roundings give everywhere (the test would hold a contracted or split multiply-add to nothing otherwise)
    two = (a * b + c).astype(np.float32)
    assert (two != r).any()


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("bg", ["colour", "f32", "f16", "u8"])
def test_composite_over_is_the_rule(pkg, fmt, bg):
    E = pkg.engine
    S, n_rand = _frame()
    B = _backgrounds(len(S), n_rand)[bg]
    got = E.composite_over(S, B, fmt)
    Bf = np.asarray(B, np.float32) if bg == "colour" else decode(B)
    want = rule(S, Bf, fmt)
    assert got.dtype == want.dtype == E.target_dtype(fmt) and got.shape == S.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), int((got.view(np.uint8) != want.view(np.uint8)).sum())
    # the consequences the header states: S = 0 gives B, B_a = 1 gives B, B = 0 gives the converted frame
    as_b = E.convert_pixels(np.broadcast_to(Bf, S.shape), fmt)
    zero = (S == 0).all(-1)
    assert zero.sum() > 500 and np.array_equal(got[zero].view(np.uint8), as_b[zero].view(np.uint8))
    if bg != "colour":
        opaque, empty = Bf[:, 3] == 1, (Bf == 0).all(-1)
        assert opaque.sum() > 500 and empty.sum() > 500
        assert np.array_equal(got[opaque].view(np.uint8), as_b[opaque].view(np.uint8))
        assert np.array_equal(got[empty].view(np.uint8), E.convert_pixels(S, fmt)[empty].view(np.uint8))
        assert np.any(np.isclose(Bf[:, 3], 0.4, atol=2e-3))
        # the edge pixels straddle the stores' boundaries: neighbours one float32 ulp apart land in different bytes / halves
        if fmt:
            e = got[n_rand:, 0].astype(np.float64)
            assert (np.diff(e) != 0).sum() > 30
    # the numpy store is the library's (test_target_format.py holds that one to known answers)
    assert np.array_equal(store(S, fmt).view(np.uint8), E.convert_pixels(S, fmt).view(np.uint8))


def test_fma_restatement_is_nan_exactly_where_ieee_fma_is():
    """IEEE 754 fma(a, b, c) is NaN iff an operand is NaN, the product is inf * 0, or the product is infinite and c the opposite
    infinity; an overflowing finite sum is an infinity, not NaN.  Known answers first, then the predicate over every combination of
    the special values (the round-to-odd step of fma32 must not touch a sum that is not finite)"""
    inf, nan, big = f32(np.inf), f32(np.nan), f32(3.0e38)
    table = [(inf, 0, 1, nan), (0, -inf, 1, nan), (inf, 1, -inf, nan), (-inf, 1, inf, nan), (inf, -1, inf, nan), (1, 1, nan, nan),
             (nan, 0, 0, nan), (0, nan, 0, nan), (inf, 1, inf, inf), (inf, -2, -inf, -inf), (inf, 1, 5, inf), (2, 3, -inf, -inf),
             (big, big, -inf, -inf), (big, big, 0, inf), (big, -2, -big, -inf), (big, 2, -big, big), (1, 0, -0.0, 0.0), (1, -0.0, -0.0, -0.0)]
    a, b, c, want = (np.array([row[k] for row in table], np.float32) for k in range(4))
    with np.errstate(all="ignore"):
        got = fma32(a, b, c)
    assert np.array_equal(np.isnan(got), np.isnan(want)), got
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (got, want)
    v = np.array([0.0, -0.0, 1.0, -1.0, 0.4, 3.0e38, -3.0e38, 1.0e-45, np.inf, -np.inf, np.nan], np.float32)
    a, b, c = (g.ravel() for g in np.meshgrid(v, v, v, indexing="ij"))
    with np.errstate(all="ignore"):
        got = fma32(a, b, c)
        p_inf = (np.isinf(a) | np.isinf(b)) & ~np.isnan(a) & ~np.isnan(b)
        invalid = (np.isinf(a) & (b == 0)) | ((a == 0) & np.isinf(b))
        p_sign = np.signbit(a) != np.signbit(b)
        want_nan = np.isnan(a) | np.isnan(b) | np.isnan(c) | invalid | (p_inf & ~invalid & np.isinf(c) & (p_sign != np.signbit(c)))
    assert np.array_equal(np.isnan(got), want_nan)
    assert want_nan.sum() > 300 and (~want_nan).sum() > 300 and np.isinf(got).sum() > 100


EDGE_ALPHAS = (0.0, 0.4, 1.0, 1.5, -0.5, np.inf, np.nan)


def _edge_frame():
    """S and B [n, 4] float32, both drawn from the stores' own edge inputs (test_target_format._inputs: every byte threshold +- 1 ulp,
    binary16 ties and denormals, 65504 / 65519.996 / 65520, infinities, -0) plus NaNs of both signs; B_a cycles through EDGE_ALPHAS,
    so k = 1 - B_a is 1, 0.6, 0, negative, above 1, -inf and NaN.  S is the input set (its alpha whatever falls there: the rule does
    not know what a channel means); B_c is a shuffle of it, so that every edge value meets every k and operands of every other kind"""
    from helpers import NAN_PATTERNS
    from test_target_format import _inputs
    x = _inputs().ravel()
    x = np.concatenate([x, np.tile(NAN_PATTERNS, 7)])
    assert x.size % 4 == 0
    S = x.reshape(-1, 4).copy()
    B = np.random.default_rng(77).permutation(x).reshape(-1, 4).copy()
    B[:, 3] = np.resize(np.array(EDGE_ALPHAS, np.float32), len(B))
    # ... and the pixels where the frame's edge value goes through alone: S over an empty background, an edge-valued B under S = 0
    keep = np.arange(len(S)) % 5
    B[keep == 0] = 0
    S[keep == 1] = 0
    return S, B


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("bg", ["f32", "f16"])
def test_composite_over_is_the_rule_at_the_edges(pkg, fmt, bg):
    """gsr_composite_over against the numpy rule on non-finite, out-of-range and boundary operands, under the NaN rule
    (helpers.assert_same_pixels): the reference the GPU is held to in test_store_edges_gpu.py, validated at the edges first"""
    from helpers import assert_same_pixels, store_edge_classes
    E = pkg.engine
    S, B = _edge_frame()
    with np.errstate(all="ignore"):
        Bi = B if bg == "f32" else B.astype(np.float16)
        Bf = decode(Bi)
        for a in decode(np.array(EDGE_ALPHAS, Bi.dtype)):
            assert (np.isnan(Bf[:, 3]) if np.isnan(a) else Bf[:, 3] == a).sum() > 5000, a
        want = rule(S, Bf, fmt)
        out32 = rule(S, Bf, 0)
        want_store = store(out32, fmt)
    got = E.composite_over(S, Bi, fmt)
    assert got.dtype == want.dtype == E.target_dtype(fmt)
    assert_same_pixels(got, want, f"format {fmt} over an {bg} image")
    # teeth: what reaches the store holds every class of edge, and NaN exactly where IEEE says (inf * 0 under B_a = -inf ... )
    cls = store_edge_classes(out32)
    print(f"composite_over edges, format {fmt}, {bg} image: {cls}")
    assert min(v for k, v in cls.items() if k != "neg_zero") > 0, cls      # (a sum is -0 only if both of its terms are)
    assert cls["nan"] > np.isnan(S).sum() + np.isnan(Bf).sum() and cls["byte_edges"] > 300 and cls["negatives"] > 10000
    if fmt == 2:
        assert (got[np.isnan(out32)] == 0).all() and got.min() == 0 and got.max() == 255
    # the numpy store is the library's on this set too
    assert_same_pixels(E.convert_pixels(out32, fmt), want_store, f"convert_pixels, format {fmt}")


def test_composite_over_rejects_bad_arguments(pkg):
    E = pkg.engine
    L = pkg.load_library()
    S = np.zeros((4, 4), np.float32)
    out = np.zeros((4, 4), np.float32)
    img = np.zeros((4, 4), np.float32)

    def call(bg, n=4, src=S, fmt=0, dst=out):
        return L.gsr_composite_over(None if src is None else src.ctypes.data, n, None if bg is None else C.byref(bg), fmt, None if dst is None else dst.ctypes.data)

    good, _ = E.background_struct((0.1, 0.2, 0.3, 0.5))
    assert call(good) == 0
    assert call(None) == GSR_E_INVALID and b"gsr_composite_over" in L.gsr_last_error()
    assert call(good, n=-1) == GSR_E_INVALID
    assert call(good, src=None) == GSR_E_INVALID and call(good, dst=None) == GSR_E_INVALID
    assert call(good, fmt=3) == GSR_E_INVALID
    assert call(good, n=0, src=None, dst=None) == 0
    b = E.gsr_background()                     # kind 0: nothing to composite over
    assert call(b) == GSR_E_INVALID
    b.kind = 3
    assert call(b) == GSR_E_INVALID
    b.kind, b.format, b.image = E.BG_IMAGE, 5, img.ctypes.data
    assert call(b) == GSR_E_INVALID            # unknown image format
    b.format, b.image = 0, None
    assert call(b) == GSR_E_INVALID            # NULL image
    b.image, b.image_is_device = img.ctypes.data, 1
    assert call(b) == GSR_E_INVALID            # the host verb reads host memory
    b.image_is_device = 0
    assert call(b) == 0
    # the render verb refuses without a context before it touches a GPU
    assert L.gsr_render_over(None, None, None, 0, C.byref(good), None, 0) == GSR_E_INVALID
    # the Python face
    with pytest.raises(pkg.GsrError):
        E.composite_over(S, np.zeros((3, 4), np.float32))
    with pytest.raises(pkg.GsrError):
        E.composite_over(S, np.zeros((4, 4), np.float64))
    with pytest.raises(pkg.GsrError):
        E.composite_over(S, (0.0, 0.0, 0.0))


def test_background_struct_matches_the_header(pkg):
    e = pkg.engine
    B = e.gsr_background
    assert C.sizeof(B) == 40
    assert [(n, getattr(B, n).offset) for n, _ in B._fields_] == [("kind", 0), ("format", 4), ("rgba", 8), ("image", 24), ("image_is_device", 32), ("reserved_", 36)]
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    body = text[text.index("typedef struct gsr_background {") + len("typedef struct gsr_background {"):text.index("} gsr_background;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")) for d in (x.strip() for x in body.split(";")) if d]
    assert names == [n for n, _ in B._fields_]
    assert "#define GSR_BG_COLOUR 1" in text and "#define GSR_BG_IMAGE  2" in text and (e.BG_COLOUR, e.BG_IMAGE) == (1, 2)
    for name in ("gsr_render_over", "gsr_composite_over", "gsplat_renderer_set_background"):
        assert hasattr(pkg.load_library(), name) and name in e.C_ABI_SYMBOLS


def test_dry_shim_remembers_the_background(pkg):
    E = pkg.engine
    R = pkg.GSplatRenderer(-1)
    col, _ = E.background_struct((0.1, 0.2, 0.3, 0.5))
    img, keep = E.background_struct(np.zeros((4, 4, 4), np.uint8))
    plane = np.zeros((4, 4, 2), np.float32)
    assert R.setBackground(col) == 0 and R.setBackground(img) == 0
    assert R.setAovTarget(E.AOV_DEPTH, plane.ctypes.data) == GSR_E_INVALID      # (there is no AOV + background verb)
    assert R.setBackground(None) == 0
    bad = E.gsr_background()
    bad.kind = 7
    assert R.setBackground(bad) == GSR_E_INVALID
    bad.kind, bad.format = E.BG_IMAGE, 9
    bad.image = keep.ctypes.data
    assert R.setBackground(bad) == GSR_E_INVALID
    bad.format, bad.image = 0, None
    assert R.setBackground(bad) == GSR_E_INVALID
    assert R.setAovTarget(E.AOV_DEPTH, plane.ctypes.data) == 0
    assert R.setBackground(col) == GSR_E_INVALID
    assert R.setAovTarget(0, None) == 0 and R.setBackground(col) == 0 and R.setBackground(E.gsr_background()) == 0


def test_over_kernels_keep_their_budgets():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): both k_blend_over instantiations use no
    scratch, at most 80 registers -- six waves per SIMD -- and at most 22 KB of LDS: the limits the depth-tested colour kernel is
    held to"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for prefix in ("_Z12k_blend_overILb0E", "_Z12k_blend_overILb1E"):
        hit = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, sorted(rows))
        vg, sg, lds, scratch = hit[0]
        print(f"{prefix}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0 and vg <= 80 and lds <= 22 * 1024, (prefix, hit[0])
