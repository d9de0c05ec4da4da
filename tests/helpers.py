"""shared helpers for the test-suite (loading golden fixtures)"""
import glob
import os
import types

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_names():
    """beauty-path fixtures holding their own inputs (the wireframe fixture w1_wire and the full-size band c4_band_* are
    handled by their own tests)"""
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
                  if not n.startswith("w") and not n.startswith("c4_band"))


def oracle_render_golden(oracle, d, s, c, threads=0):
    """the oracle's frame for a fixture: depth-tested when the fixture carries an opaque pass's depth buffer (N4)"""
    if "depth" in d.files:
        return oracle.render_depth(s, c, d["depth"], d["origin"])
    return oracle.render(s, c, d["origin"], threads=threads) if threads else oracle.render(s, c, d["origin"])


def engine_render_golden(engine, d, c):
    return engine.render_depth(c, d["depth"]) if "depth" in d.files else engine.render(c)


def load_golden(name):
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    s = types.SimpleNamespace(P=d["P"], Cd=d["Cd"], alpha=d["alpha"], scale=d["scale"], orient=d["orient"],
                              shx=d["shx"] if "shx" in d else None, shy=d["shy"] if "shy" in d else None,
                              shz=d["shz"] if "shz" in d else None)
    s.n = s.P.shape[0]
    w, h, order = [int(x) for x in d["cam_whs"]]
    c = types.SimpleNamespace(obj_view=d["cam_obj_view"], object=d["cam_object"], inv_object=d["cam_inv_object"],
                              view=d["cam_view"], proj=d["cam_proj"], cam_pos=d["cam_pos"], width=w, height=h,
                              sh_order=order)
    return d, s, c


# Acceptance of an image against the reference-GLSL golden (SwiftShader, rasterised at `supersample` times the nominal resolution
# so that its vertex snapping -- 1/16 of ITS pixel -- shrinks to `grid` = 1/(16 * supersample) of a nominal pixel: ~8-bit sub-pixel
# hardware).  Where may such an image differ from the analytic frame by more than the north-star tolerance of 1e-3 per channel?
# Round 4 answers that per pixel instead of with a blanket "0.2 % of the pixels":
#   * inside the oracle's EDGE MASK (gso_edge_mask): the pixel centre lies within 1.5 grid steps of an edge of some visible quad --
#     there the rasteriser's fixed-point coverage rule decides -- or a covering fragment sits at the 1/255 discard threshold to
#     within what a grid step of quad shift does to its alpha, or (depth-tested frames) at the depth test's threshold.  A flipped
#     fragment moves a channel by at most opacity * exp(-4) * T (edge) or 1/255 (discard): bounded by GOLDEN_MAX_OUTLIER;
#   * everywhere else the fragments are the same on both sides, and the only difference is that GL interpolates the quad-local
#     coordinate from SNAPPED vertices: |err| <= 1e-3 + GOLDEN_SNAP_GAIN * grid * sens[p], sens = gso_snap_sensitivity (sum of
#     T * alpha * |d|kq|^2 / d shift| over the pixel's fragments; half-pixel-wide splats make that term exceed 1e-3 by itself).
# Measured on the twelve fixtures: no pixel outside the mask needs a gain above 0.22 (the bound is ~2 ln2 * shift / grid ~ 1);
# the mask covers 1-13 % of a frame.  The old global figures stay as sanity bounds.
GOLDEN_TOL = 1e-3
GOLDEN_MIN_FRAC = 0.997      # >= 99.7 % of pixels within 1e-3 on every channel (sanity; the per-pixel rule below is the test)
GOLDEN_MAX_OUTLIER = 0.02    # edge-flip bound: exp(-4) * opacity * T
GOLDEN_MEAN = 1e-4
GOLDEN_EDGE_STEPS = 1.5      # half-width of the edge band, in sub-pixel grid steps
GOLDEN_SNAP_GAIN = 1.0       # channel change per (grid step x sensitivity) outside the mask


def golden_uncertainty(oracle, d, s, c):
    """(edge mask bool [H, W], allowed |err| outside the mask float [H, W]) for a fixture: see the rule above"""
    grid = 1.0 / (16.0 * int(d["supersample"]))
    depth = d["depth"] if "depth" in d.files else None
    mask = oracle.edge_mask(s, c, d["origin"], delta_px=GOLDEN_EDGE_STEPS * grid, eps_log2=1e-5, depth=depth, eps_depth=1e-6)
    sens = oracle.snap_sensitivity(s, c, d["origin"]).astype(np.float64)
    return mask, GOLDEN_TOL + GOLDEN_SNAP_GAIN * grid * sens


def check_against_golden(img, golden_img, max_bias=2e-5, uncertainty=None, extra_tol=0.0):
    """uncertainty = golden_uncertainty(...): the per-pixel rule; extra_tol: what the image under test may add by construction
    (the blend kernel's per-pixel early-out: 2^-14)"""
    err = np.abs(img.astype(np.float64) - golden_img.astype(np.float64))
    frac = float((err.max(axis=2) <= GOLDEN_TOL).mean())
    assert frac >= GOLDEN_MIN_FRAC, f"only {frac:.5f} of pixels within {GOLDEN_TOL}"
    assert err.max() <= GOLDEN_MAX_OUTLIER, f"outlier {err.max()} exceeds the edge-flip bound"
    assert err.mean() <= GOLDEN_MEAN, f"mean abs error {err.mean()}"
    signed = float((img.astype(np.float64) - golden_img).mean())
    assert abs(signed) <= max_bias, f"biased by {signed}"
    if uncertainty is not None:
        mask, allowed = uncertainty
        e = err.max(axis=2)
        bad = (~mask) & (e > allowed + extra_tol)
        assert not bad.any(), (f"{int(bad.sum())} pixels differ by more than the 1e-3 budget away from every quad edge and discard threshold: "
                               f"first at (x, y) = {np.argwhere(bad)[0][::-1].tolist()}, |err| = {e[bad].max():.5f}")
        assert mask.mean() <= 0.25, f"the edge mask covers {mask.mean():.3f} of the frame: not a sharp rule any more"
    return frac, float(err.max()), float(err.mean())


def dilate1(m):
    out = m.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= np.roll(np.roll(m, dy, 0), dx, 1)
    return out


def check_wire_against_golden(img, golden_wire):
    """GL rasterises lines with the diamond-exit rule, the contract with a centre-sampling rule: the two
    agree to within one pixel everywhere and pixel-for-pixel on the vast majority"""
    g, o = golden_wire[..., 3] > 0, img[..., 3] > 0
    assert g.sum() > 1000
    assert (g & dilate1(o)).sum() == g.sum() and (o & dilate1(g)).sum() == o.sum()
    same = g & o
    assert same.sum() >= 0.97 * g.sum()
    # where both drew the same splat's line the colour (Cd, fp16-exact) is identical
    eq = np.all(img[same] == golden_wire[same].astype(np.float32), axis=1)
    assert eq.mean() >= 0.97


class HipBuffers:
    """raw device buffers for tests that hand DEVICE pointers to the C ABI (hipMalloc / hipMemcpy through ctypes)"""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.hip = C.CDLL("libamdhip64.so")
        self.ptrs = []

    def alloc(self, nbytes: int) -> int:
        p = self.C.c_void_p()
        assert self.hip.hipMalloc(self.C.byref(p), self.C.c_size_t(nbytes)) == 0
        self.ptrs.append(p)
        return p.value

    def upload(self, arr: np.ndarray) -> int:
        a = np.ascontiguousarray(arr)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(self.C.c_void_p(p), self.C.c_void_p(a.ctypes.data), self.C.c_size_t(a.nbytes), 1) == 0
        return p

    def download(self, ptr: int, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(self.C.c_void_p(out.ctypes.data), self.C.c_void_p(ptr), self.C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


# The blend contract ("early-out"): a GPU frame differs from the oracle's only by the per-pixel early-out (the
# oracle restates it: out_eo) and by the last bits of 2^x (out_bound, per pixel and channel).  Every GPU-vs-oracle comparison
# goes through check_contract; the north-star 1e-3 against the plain frame stays as well.
CONTRACT_TOL = 1e-3


def check_contract(img, oracle, splats, cam, origin=(0, 0, 0), depth=None, rows=None, threads=0, label="", ret_plain=False):
    """assert |img - plain| <= 1e-3, |img - eo| <= bound on every pixel and channel, img finite; returns the worst err / bound
    (printed as a CONTRACT line), and the oracle's plain frame too if ret_plain.  rows = (lo, hi): img holds rows [lo, hi) only."""
    eo, plain, bound, _ = oracle.render_contract(splats, cam, origin=origin, depth=depth, rows=rows, threads=threads)
    assert img.shape == plain.shape, (img.shape, plain.shape)
    assert np.isfinite(img).all()
    e_plain = np.abs(img - plain)
    err = np.abs(img.astype(np.float64) - eo.astype(np.float64))
    fin = np.isfinite(bound)
    ratio = np.zeros(err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio[fin] = np.where(bound[fin] > 0, err[fin] / bound[fin], np.where(err[fin] > 0, np.inf, 0.0))
    worst = float(ratio.max(initial=0.0))
    print(f"CONTRACT {label or 'frame'} {img.shape[1]}x{img.shape[0]}: worst err/bound = {worst:.4f}, "
          f"max|err| = {float(err[fin].max(initial=0.0)):.3e}, median bound = {float(np.median(bound[fin])) if fin.any() else 0.0:.3e}, "
          f"max|img - plain| = {float(e_plain.max(initial=0.0)):.3e}")
    assert e_plain.max(initial=0.0) <= CONTRACT_TOL, \
        f"max err {e_plain.max()} at {np.unravel_index(e_plain.argmax(), e_plain.shape)}"
    if not (worst <= 1.0):
        over = fin & (err > bound)
        y, x, ch = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{int(over.any(axis=2).sum())} pixels outside the contract bound; worst at (x, y, channel) = "
                             f"({x}, {y}, {ch}): |img - eo| = {err[y, x, ch]:.4e}, bound = {bound[y, x, ch]:.4e}, "
                             f"ratio = {worst:.3f}, img = {img[y, x].tolist()}, eo = {eo[y, x].tolist()}")
    return (worst, plain) if ret_plain else worst


def camera_axes(cam):
    """(position, rows = camera x / y / z axes in world space) of a camera, float64"""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    R = V[:3, :3]
    return -R.T @ V[:3, 3], R


def _object_matrix():
    a, b = np.deg2rad(25.0), np.deg2rad(-40.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx @ np.diag([1.3, 0.8, 1.1])
    m[:3, 3] = (0.1, -0.05, 0.2)
    return m


# an object transform with a rotation about two axes, a non-uniform scale and a translation (test_frame_constants_gpu.py, cull_edge_cases.py)
OBJECT_MATRIX = _object_matrix()


def unproject(cam, X, Y, D):
    """float64 world points at GL window coordinates (X, Y) (y up, pixel centres at +0.5) and view distance D, for a
    perspective camera whose projection has no off-centre terms"""
    X, Y, D = (np.asarray(a, np.float64) for a in np.broadcast_arrays(X, Y, D))
    Pm = np.asarray(cam.proj, np.float64).reshape(4, 4).T
    pos, R = camera_axes(cam)
    xc = (2.0 * X / cam.width - 1.0) * D / Pm[0, 0]
    yc = (2.0 * Y / cam.height - 1.0) * D / Pm[1, 1]
    return pos + xc[..., None] * R[0] + yc[..., None] * R[1] - D[..., None] * R[2]


def world_sigma(cam, s_px, D):
    """isotropic world scale whose projected axis s1 = sqrt(2 lambda) is about s_px pixels at view distance D"""
    focal = cam.width * float(np.asarray(cam.proj, np.float64).reshape(4, 4).T[0, 0]) * 0.5
    return np.asarray(s_px, np.float64) * np.asarray(D, np.float64) / (np.sqrt(2.0) * focal)


def make_splats(pkg, P, sigma, opacity, Cd, orient=None, sh=None):
    """a Splats from float64 arrays: P [n, 3], sigma [n] or [n, 3], opacity [n], Cd [n, 3]; orient (x, y, z, w) [n, 4]
    (identity when None); sh = (shx, shy, shz) float [n, 15] each or None"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    n = P.shape[0]
    sig = np.asarray(sigma, np.float64)
    sig = np.broadcast_to(sig[:, None] if sig.ndim == 1 else sig, (n, 3))
    if orient is None:
        orient = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1))
    f16 = pkg.scenes.f16bits
    shs = [None, None, None]
    if sh is not None:
        for k in range(3):
            shs[k] = np.zeros((n, 16), np.uint16)
            shs[k][:, :15] = f16(np.asarray(sh[k], np.float64).reshape(n, 15))
    return pkg.scenes.Splats(np.ascontiguousarray(P, np.float32), f16(np.broadcast_to(np.asarray(Cd, np.float64), (n, 3))),
                             np.ascontiguousarray(np.broadcast_to(np.asarray(opacity, np.float64), (n,)), np.float32),
                             f16(sig), f16(np.asarray(orient, np.float64)), *shs)


def veil_scene(pkg, cam, n=3000, seed=0, colours=(0.0, 1.0)):
    """a veil: n splats of opacity 0.005-0.05 and 10-40 px, in a ball 0.3 across at the camera's pivot; stacks hundreds deep,
    most pixels unsaturated"""
    rng = np.random.default_rng(seed)
    pos, R = camera_axes(cam)
    D = float(np.linalg.norm(pos))
    P = rng.normal(0.0, 0.15, (n, 3))
    return make_splats(pkg, P, world_sigma(cam, rng.uniform(15.0, 50.0, n), D), rng.uniform(0.005, 0.05, n),
                       rng.uniform(colours[0], colours[1], (n, 3)))


def stop_scene(pkg, cam, n=500, seed=0):
    """a deep stack of wide, faint splats along the view axis (distinct depths, lateral jitter): each pixel's T falls through
    2^-14 after a few hundred fragments, and on many pixels it lands within the bound's error of 2^-14 -- the early-out's
    decision is ambiguous there"""
    rng = np.random.default_rng(seed)
    D = np.linspace(2.0, 3.5, n) + rng.uniform(0.0, 1e-3, n)
    X = cam.width * (0.5 + rng.uniform(-0.05, 0.05, n))
    Y = cam.height * (0.5 + rng.uniform(-0.05, 0.05, n))
    P = unproject(cam, X, Y, D)
    return make_splats(pkg, P, world_sigma(cam, rng.uniform(0.4, 0.8, n) * max(cam.width, cam.height), D),
                       rng.uniform(0.02, 0.04, n), rng.uniform(0.0, 1.0, (n, 3)))


# The NaN rule (include/gsplat_hip.h, "target format" and "background"): in an RGBA32F or RGBA16F target a channel that is NaN on
# one side is NaN on the other, with sign and payload unspecified -- x86 and gfx950 quiet and propagate NaNs differently; every other
# channel, infinities and signed zeros included, is bit-exact.  RGBA8 holds no NaN (the store maps it to 0): bit-exact throughout.
# quiet and signalling NaNs of both signs with several payloads: what the edge tests feed wherever a NaN may arrive
NAN_PATTERNS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fc12345, 0xff923456], np.uint32).view(np.float32)


def _as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def pixels_differ(got, want):
    """the boolean array of channels on which two images of one target format differ under the NaN rule"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    diff = _as_bits(got) != _as_bits(want)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        diff = np.where(gn | wn, gn != wn, diff)
    return diff


def assert_same_pixels(got, want, label=""):
    """got == want under the NaN rule; the message names the first channel that differs"""
    diff = pixels_differ(got, want)
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{label}: {int(diff.sum())} of {diff.size} channels differ; first at {at}: got {got[at]!r} "
                             f"(bits {int(_as_bits(got)[at]):#x}), want {want[at]!r} (bits {int(_as_bits(want)[at]):#x})")


def store_edge_classes(x):
    """how many float32 values of x sit in each class the packed stores can get wrong:
    ties            exactly halfway between two neighbouring binary16 values (round to nearest EVEN decides), below the overflow threshold
    half_denormals  non-zero, below 2^-14 in magnitude: binary16 has no normal number for them (denormal, or rounds to zero)
    overflow        finite, at least 65520 in magnitude: binary16 infinity
    in_1_65504      in (1, 65504): beyond the 8-bit store's clamp, inside binary16's range
    byte_edges      within one float32 step of a threshold (k + 0.5) / 255 between two bytes
    and nan, inf, negatives (below zero, -inf included), neg_zero"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    fin = np.isfinite(x)
    a = np.abs(x[fin]).astype(np.float64)
    a = a[a < 65520.0]
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
    lo = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    h = h.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ties = (a != h) & ((a == (h + lo) / 2) | (a == (h + hi) / 2))
    t = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    near = np.concatenate([np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))])
    return {"ties": int(ties.sum()), "half_denormals": int(((a > 0) & (a < 2.0 ** -14)).sum()),
            "overflow": int((fin & (np.abs(x) >= np.float32(65520.0))).sum()),
            "in_1_65504": int(((x > 1) & (x < 65504)).sum()), "byte_edges": int(np.isin(x, near).sum()),
            "nan": int(np.isnan(x).sum()), "inf": int(np.isinf(x).sum()), "negatives": int((x < 0).sum()),
            "neg_zero": int(((x == 0) & np.signbit(x)).sum())}
