"""The case table of the measuring tests (gsr_measure; include/gsplat_hip.h, "measuring a selection"), shared by test_measure.py (no
GPU) and test_measure_gpu.py.  Everything expected comes from gsr_measure_eval -- the rule on the host -- and the numpy restatement
below (restate), never from the GPU path.  The restatement is written from the header's text, not from the library: the tree sum is
a literal level-by-level pairwise sum in np.float64 over the padded leaves, the bounds go through the ordered key of the float's bits,
the bin rule runs in np.float32 steps.

A case = a cloud, the requests REQUESTS and the masks of masks():
  clouds   n in SIZES: one lane; 63, 64, 65 (the wave's edge); 255, 256, 257 (the workgroup's edge); 16385 (65 workgroup partials:
           more than a wave's worth) and 65537 (257: more than a workgroup's worth, so the partials need a further level), each with
           SH and without.  Positions are OFFSET plus a spread of +-1 with full 24-bit mantissas, and a third of them lie within 2^-10
           of REF instead: products fill 48 bits at exponents 40 apart, so the sums round at nearly every add, and a left-to-right
           float64 sum and a float32 sum differ from the tree's (test_measure.py asserts it on the table: it is a condition of the
           table, not a measurement);
  seeded   splats at upload indices spread over the cloud (n >= 63): +0 and -0 x positions (the smallest x of the cloud: the lower
           bound is -0 whichever comes first), NaN, +inf and -inf position components; NaN, inf, negative and denormal scale halves;
           alpha exactly at the histogram's lo, one float under its hi (where (x - lo) * inv_w rounds UP to bins: the clamp), NaN, and
           above 1; a NaN Cd half;
  masks    all set, none set, one bit, alternating words of 0 and ~0 (half of every wave loads nothing), alternating PAIRS of words
           (a wave reads two: whole waves skip), random; the all-set and random ones carry garbage in the bits at and behind n of the
           last word.
EXTENT_K is 3: two significant bits, so the restatement's fmaf -- the product and the sum in float64, rounded once to float32 -- is
exact before its one rounding for every half (11 bits) and every position here, denormal halves included."""
import ctypes as C

import numpy as np

SIZES = (1, 63, 64, 65, 255, 256, 257, 16385, 65537)
OFFSET = np.array([1000.0, -2000.0, 500.0], np.float32)
REF = (1.5, -0.25, 3.0)
EXTENT_K = 3.0
A_LO, A_HI, A_BINS = np.float32(0.125), np.float32(0.875), 70         # (1 ulp under hi lands on bin 70 of 70: the clamp)
WHATS = tuple(range(8))
_CACHE = {}

# (channel name, lo, hi, bins, log2): two sets of four cover the nine channels
HISTS_A = (("ALPHA", 0.125, 0.875, A_BINS, False), ("SCALE_MAX", -8.0, -1.0, 56, True), ("X", 998.5, 1001.5, 256, False), ("CD_G", 0.0, 1.0, 17, False))
HISTS_B = (("Y", -2001.5, -1999.5, 3, False), ("Z", 498.5, 501.5, 255, False), ("SCALE_MIN", -9.0, -2.0, 1, True), ("CD_R", 0.25, 0.75, 100, False))
HISTS_C = (("CD_B", 0.0, 1.0, 256, False), ("ALPHA", -12.0, 0.5, 200, True), ("SCALE_MAX", 0.0, 0.25, 64, False))


def request(pkg, what=7, hists=(), skip_hidden=False):
    E = pkg.engine
    specs = [E.hist_spec(getattr(E, "HIST_" + ch), lo, hi, bins, log2) for ch, lo, hi, bins, log2 in hists]
    return E.measure_request(bounds=bool(what & 1), extent=EXTENT_K if what & 2 else None, moments=bool(what & 4), ref=REF, hists=specs,
                             skip_hidden=skip_hidden)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------------
def tree_sum(leaves):
    """the perfect binary tree over the leaves, padded with +0.0 to the smallest 2^k >= max(n, 64): every level is left + right"""
    a = np.asarray(leaves, np.float64)
    size = 64
    while size < a.shape[0]:
        size *= 2
    level = np.zeros((size,) + a.shape[1:], np.float64)
    level[:a.shape[0]] = a
    with np.errstate(over="ignore", invalid="ignore"):
        while level.shape[0] > 1:
            level = level[0::2] + level[1::2]
    return level[0]


def ordered_key(x):
    """float32 -> int32 whose order is the total order of the floats' bits (-0 < +0)"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def key_to_float(k):
    k = np.asarray(k, np.int32)
    return (k ^ ((k >> 31) & np.int32(0x7fffffff))).view(np.float32)


def bounds(x):
    """(min, max) of the rows of float32 x (m, 3) in key order; +inf / -inf for none"""
    if x.shape[0] == 0:
        return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    k = ordered_key(x).reshape(-1, 3)
    return key_to_float(k.min(axis=0)), key_to_float(k.max(axis=0))


def log2_linear(x):
    """GSR_HIST_LOG2's replacement of finite x > 0, in integer and conversion arithmetic"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (bits - np.uint32(0x3f800000)).view(np.int32).astype(np.float32) * np.float32(2.0 ** -23)


def histogram(x, lo, hi, bins, log2):
    """bins + 3 counts of float32 x: the bins, under, over, nan; every step in float32"""
    f32 = np.float32
    x = np.ascontiguousarray(x, np.float32)
    lo, hi = f32(lo), f32(hi)
    inv_w = f32(np.float64(bins) / (np.float64(hi) - np.float64(lo)))
    out = np.zeros(bins + 3, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(x)
        under, over = np.zeros(x.shape, bool), np.zeros(x.shape, bool)
        if log2:
            under |= ~nan & ~(x > 0)
            over |= ~nan & np.isposinf(x)
            ok = ~(nan | under | over)
            v = np.where(ok, log2_linear(np.where(ok, x, f32(1))), f32(0))
        else:
            ok, v = ~nan, x
        u2 = ok & ~(v >= lo)
        o2 = ok & ~u2 & ~(v < hi)
        inside = ok & ~u2 & ~o2
        t = ((v[inside] - lo).astype(f32) * inv_w).astype(f32)
        idx = np.where(t >= f32(bins), bins - 1, np.trunc(np.where(np.isfinite(t), t, 0)).astype(np.int64))
    out[:bins] = np.bincount(idx, minlength=bins).astype(np.uint32)
    out[bins], out[bins + 1], out[bins + 2] = (under | u2).sum(), (over | o2).sum(), nan.sum()
    return out


def channel(name, P, alpha, scale, Cd):
    h2f = lambda a: np.ascontiguousarray(a, np.uint16).view(np.float16).astype(np.float32)
    if name in "XYZ":
        return P[:, "XYZ".index(name)]
    if name == "ALPHA":
        return alpha
    if name.startswith("CD_"):
        return h2f(Cd)[:, "RGB".index(name[3])]
    s = np.abs(h2f(scale))
    bad = np.isnan(s).any(axis=1)
    v = np.where(bad, np.float32(0), (s.max(axis=1) if name == "SCALE_MAX" else s.min(axis=1)))
    return np.where(bad, np.float32(np.nan), v).astype(np.float32)


def restate(P, alpha, scale, Cd, sel, hists=()):
    """everything gsr_measure reports of the selected splats sel (bool (n,)), with every bit of `what` set -> dict"""
    f32 = np.float32
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = P.shape[0]
    measured = sel & np.isfinite(P).all(axis=1)
    halves = np.ascontiguousarray(scale, np.uint16).reshape(-1, 3)
    extent = measured & ((halves & 0x7c00) != 0x7c00).all(axis=1)
    out = {"n_selected": int(sel.sum()), "n_measured": int(measured.sum()), "n_extent": int(extent.sum())}
    out["lo"], out["hi"] = bounds(P[measured])
    smax = np.abs(halves[extent].view(np.float16).astype(np.float32)).max(axis=1) if extent.any() else np.zeros(0, f32)
    pe = P[extent].astype(np.float64)
    reach = np.float64(f32(EXTENT_K)) * smax.astype(np.float64)[:, None]
    out["lo_e"], _ = bounds((pe - reach).astype(f32))
    _, out["hi_e"] = bounds((pe + reach).astype(f32))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (P - np.asarray(REF, f32)[None, :]).astype(f32).astype(np.float64)
    d = np.where(measured[:, None], d, 0.0)
    terms = np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                      d[:, 2] * d[:, 2]], axis=1)
    terms[~measured] = 0.0                                # (+0.0: a product of -0.0 must not leave a -0.0 leaf behind)
    out["terms"] = terms
    out["sum"] = tree_sum(terms) if n else np.zeros(9)
    out["hist"] = [histogram(channel(ch, P, alpha, scale, Cd)[sel], lo, hi, bins, log2) for ch, lo, hi, bins, log2 in hists]
    return out


def assert_result(res, want, what, label, n_hist=None):
    """a gsr_measure_result against restate()'s dict, for the bits of `what` that were asked for: field for field and bit for bit; what
    was not asked for holds the empty result's value"""
    u32 = lambda a: np.asarray(list(a), np.float32).view(np.uint32)
    inf = np.float32(np.inf)
    assert res.n_selected == want["n_selected"], (label, "n_selected", res.n_selected, want["n_selected"])
    assert res.n_measured == (want["n_measured"] if what else 0), (label, "n_measured", res.n_measured)
    assert res.n_extent == (want["n_extent"] if what & 2 else 0), (label, "n_extent", res.n_extent)
    for name, bit, empty in (("lo", 1, inf), ("hi", 1, -inf), ("lo_e", 2, inf), ("hi_e", 2, -inf)):
        exp = want[name] if what & bit else np.full(3, empty, np.float32)
        assert np.array_equal(u32(getattr(res, name)), u32(exp)), (label, name, list(getattr(res, name)), list(exp))
    exp = want["sum"] if what & 4 else np.zeros(9)
    got = np.asarray(list(res.sum), np.float64)
    assert np.array_equal(got.view(np.uint64), np.asarray(exp, np.float64).view(np.uint64)), (label, "sum", got.tolist(), np.asarray(exp).tolist())
    if n_hist is not None:
        assert len(res.hist) == n_hist == len(want["hist"]), label
        for k in range(n_hist):
            assert res.hist[k].dtype == np.uint32 and np.array_equal(res.hist[k], want["hist"][k]), (label, "hist", k, res.hist[k].tolist(), want["hist"][k].tolist())


def same_result(a, b):
    """two gsr_measure_result (with .hist): equal in every byte and every histogram word"""
    return bytes(a) == bytes(b) and len(a.hist) == len(b.hist) and all(np.array_equal(x, y) for x, y in zip(a.hist, b.hist))


# ---- the table -------------------------------------------------------------------------------------------------------------------------
SEEDS = ("pos_pzero", "pos_nzero", "pos_nan", "pos_pinf", "pos_ninf", "scale_nan", "scale_inf", "scale_negative", "scale_denormal",
         "alpha_at_lo", "alpha_under_hi", "alpha_nan", "alpha_above_1", "cd_nan")


def _seed(s, i, label):
    f32, u16 = np.float32, np.uint16
    h = lambda v: np.asarray(v, np.float32).astype(np.float16).view(np.uint16)
    if label == "pos_pzero":
        s.P[i, 0] = f32(0.0)
    elif label == "pos_nzero":
        s.P[i, 0] = f32(-0.0)
    elif label == "pos_nan":
        s.P[i, 1] = f32(np.nan)
    elif label == "pos_pinf":
        s.P[i, 0] = f32(np.inf)
    elif label == "pos_ninf":
        s.P[i, 2] = f32(-np.inf)
    elif label == "scale_nan":
        s.scale[i, 1] = u16(0x7e00)
    elif label == "scale_inf":
        s.scale[i, 0] = u16(0xfc00)
    elif label == "scale_negative":
        s.scale[i] = h([-0.06, -0.005, -0.03])
    elif label == "scale_denormal":
        s.scale[i] = (u16(0x0001), u16(0x8002), u16(0x0000))
    elif label == "alpha_at_lo":
        s.alpha[i] = A_LO
    elif label == "alpha_under_hi":
        s.alpha[i] = np.nextafter(A_HI, f32(-np.inf))
    elif label == "alpha_nan":
        s.alpha[i] = f32(np.nan)
    elif label == "alpha_above_1":
        s.alpha[i] = f32(1.5)
    elif label == "cd_nan":
        s.Cd[i, 2] = u16(0x7e00)


class Case:
    def __init__(self, name, splats, specials):
        self.name, self.splats, self.specials, self.n = name, splats, specials, splats.n
        self.sh = splats.shx is not None
        self._restated = {}

    def masks(self, pkg):
        """name -> (bool (n,) the splats selected, packed words as the verbs take them)"""
        if not hasattr(self, "_masks"):
            n, E = self.n, pkg.engine
            rng = np.random.default_rng(900 + n)
            words = (n + 31) // 32
            garbage = np.uint32((0xffffffff << (n % 32)) & 0xffffffff) if n % 32 else np.uint32(0)
            one = np.zeros(n, bool)
            one[(n * 2) // 3] = True
            alt = np.repeat(np.arange(words) % 2 == 1, 32)[:n]           # words 0, ~0, 0, ~0, ...: half of every wave loads nothing
            alt2 = np.repeat(np.arange(words) % 4 >= 2, 32)[:n]          # words 0, 0, ~0, ~0, ...: a wave reads two words, so whole waves skip
            rnd = rng.random(n) < 0.4
            out = {}
            for name, m, dirty in (("all", np.ones(n, bool), True), ("none", np.zeros(n, bool), False), ("one", one, False), ("alt", alt, False),
                                   ("alt2", alt2, False), ("random", rnd, True)):
                w = E.pack_mask(m)
                if dirty and w.size:
                    w[-1] |= garbage
                out[name] = (m, w)
            self._masks = out
        return self._masks

    def restate(self, pkg, mask_name, hists=(), cloud=None, hidden=None):
        s = self.splats if cloud is None else cloud
        sel = self.masks(pkg)[mask_name][0] if isinstance(mask_name, str) else mask_name
        if hidden is not None:
            sel = sel & ~hidden
        return restate(s.P, s.alpha, s.scale, s.Cd, sel, hists)

    def __repr__(self):
        return self.name


def _make(pkg, name, n, sh, seed):
    s = pkg.scenes.make_scene(n, seed=seed, sh=sh, log_scale_range=(-4.0, -2.0))
    rng = np.random.default_rng(700 + seed)
    s.P[:] = (OFFSET[None, :] + rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).astype(np.float32)
    near = rng.random(n) < 0.3                              # ... and a third lies within 2^-10 of REF: terms 2^-40 of the others' size
    s.P[near] = (np.asarray(REF, np.float32)[None, :] + rng.uniform(-2.0 ** -10, 2.0 ** -10, (int(near.sum()), 3)).astype(np.float32)).astype(np.float32)
    s.alpha[:] = rng.random(n).astype(np.float32)
    specials = {}
    if n >= 63:
        for k, label in enumerate(SEEDS):
            i = (19 * k + 2) % n
            _seed(s, i, label)
            specials[label] = i
    return Case(name, s, specials)


def case_names():
    out = []
    for n in SIZES:
        out += [f"n{n}_sh", f"n{n}_nosh"]
    return out


def case(pkg, name):
    """the case of that name, built on first use and kept (the large ones are built only by the tests that run them)"""
    if name not in _CACHE:
        n, sh = int(name[1:name.index("_")]), name.endswith("_sh")
        _CACHE[name] = _make(pkg, name, n, sh, 30 + 2 * SIZES.index(n) + (0 if sh else 1))
    return _CACHE[name]
