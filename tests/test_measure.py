"""Measuring a selection without a GPU (include/gsplat_hip.h, "measuring a selection"): gsr_measure_eval -- the rule the kernels
evaluate, on the host -- against the numpy restatement of measure_cases.py for every case, mask and `what` combination, the case
table's own conditions, the empty selection and the empty cloud, SKIP_HIDDEN by volumes and by a mask, every refusal of
gsr_hist_prepare and of the request, the header's constants and structs, the LOG2 replacement, and the resources the compiler gives
k_measure.  No tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import measure_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
NAMES = MC.case_names()
NAN, INF = float("nan"), float("inf")
HIST_SETS = (MC.HISTS_A, MC.HISTS_B, MC.HISTS_C, ())


def _ev(pkg, c, req, mask_words, cloud=None, vis=None):
    s = c.splats if cloud is None else cloud
    return pkg.engine.measure_eval(req, s.P, s.alpha, s.scale, s.Cd, mask=mask_words, vis=vis)


# ---- (a) the eval against the numpy restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_eval_equals_the_restatement(pkg, name):
    c = MC.case(pkg, name)
    every = MC.HISTS_A + MC.HISTS_B + MC.HISTS_C
    for mask_name, (sel, words) in c.masks(pkg).items():
        full = c.restate(pkg, mask_name, every)
        for what in MC.WHATS:
            pick = 0 if what == 7 else what % 4               # (every set meets several combinations; everything at once: set A)
            hists, at = HIST_SETS[pick], (0, 4, 8, 0)[pick]
            want = dict(full, hist=full["hist"][at:at + len(hists)])
            got = _ev(pkg, c, MC.request(pkg, what, hists), words)
            MC.assert_result(got, want, what, f"{name} mask {mask_name} what {what}", n_hist=len(hists))
        # a NULL mask is every splat; a boolean mask is its packed words
        if mask_name == "all":
            MC.assert_result(_ev(pkg, c, MC.request(pkg, 7, MC.HISTS_B), None), dict(full, hist=full["hist"][4:8]), 7, f"{name} NULL mask", n_hist=4)
        assert MC.same_result(_ev(pkg, c, MC.request(pkg, 7, MC.HISTS_C), sel), _ev(pkg, c, MC.request(pkg, 7, MC.HISTS_C), words)), mask_name


# ---- (b) the case table is not vacuous -----------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_its_header_says(pkg):
    assert pkg.engine.SELECT_BLOCK == 256 and {1, 63, 64, 65, 255, 256, 257}.issubset(MC.SIZES)
    assert (16385 + 255) // 256 == 65 and (65537 + 255) // 256 == 257 and {16385, 65537}.issubset(MC.SIZES)
    assert NAMES == [f"n{n}_{s}" for n in MC.SIZES for s in ("sh", "nosh")]
    used = {ch for hs in HIST_SETS for ch, *_ in hs}
    assert used == {"X", "Y", "Z", "ALPHA", "SCALE_MAX", "SCALE_MIN", "CD_R", "CD_G", "CD_B"}
    # one float under the alpha histogram's hi, (x - lo) * inv_w rounds UP to bins in float32: only the clamp keeps it in the last bin
    f32 = np.float32
    x = np.nextafter(MC.A_HI, f32(-np.inf))
    inv_w = f32(np.float64(MC.A_BINS) / (np.float64(MC.A_HI) - np.float64(MC.A_LO)))
    assert f32(f32(x - MC.A_LO) * inv_w) == f32(MC.A_BINS) and x < MC.A_HI
    assert pkg.engine.hist_spec(pkg.engine.HIST_ALPHA, MC.A_LO, MC.A_HI, MC.A_BINS).inv_w == inv_w


@pytest.mark.parametrize("name", [n for n in NAMES if int(n[1:n.index("_")]) >= 63])
def test_cases_are_not_vacuous(pkg, name):
    c = MC.case(pkg, name)
    s, at = c.splats, c.specials
    assert sorted(at) == sorted(MC.SEEDS) and len(set(at.values())) == len(MC.SEEDS)
    for mask_name in ("all", "random"):
        sel = c.masks(pkg)[mask_name][0]
        r = c.restate(pkg, mask_name, MC.HISTS_A)
        terms = r["terms"]
        # a left-to-right float64 sum and a float32 sum are NOT the tree's sum: an order-blind or narrower reduction cannot pass
        naive = np.cumsum(terms, axis=0, dtype=np.float64)[-1]
        narrow = np.cumsum(terms.astype(np.float32), axis=0, dtype=np.float32)[-1].astype(np.float64)
        assert (naive != r["sum"]).any(), (name, mask_name, "the sequential float64 sum equals the tree sum")
        assert (narrow != r["sum"]).sum() >= 6, (name, mask_name, "the float32 sum equals the tree sum")
        assert 0 < r["n_extent"] < r["n_measured"] < r["n_selected"] or mask_name == "random"
        assert 0 < r["n_selected"] <= c.n
    r = c.restate(pkg, "all", MC.HISTS_A)
    assert r["n_selected"] == c.n and r["n_measured"] == c.n - 3 and r["n_extent"] == c.n - 5
    # -0 and +0 are both the smallest x: the lower bound is -0 whichever is met first
    assert at["pos_pzero"] != at["pos_nzero"] and r["lo"].view(np.uint32)[0] == 0x80000000
    alpha_h, smax_h, x_h, cd_h = r["hist"]
    assert alpha_h[0] >= 1 and alpha_h[MC.A_BINS - 1] >= 1 and alpha_h[MC.A_BINS + 1] >= 1 and alpha_h[MC.A_BINS + 2] == 1      # at lo, the clamp, above 1, NaN
    assert smax_h[56 + 1] == 1 and smax_h[56 + 2] == 1 and smax_h[56] >= 1                   # an infinite half, a NaN half, the denormal halves
    assert x_h[256] >= 2 and x_h[256 + 1] == 1 and x_h[256 + 2] == 0                         # +-0 (and what lies near REF) under, +inf over
    assert int(alpha_h.sum()) == int(smax_h.sum()) == int(x_h.sum()) == int(cd_h.sum()) == c.n, "a histogram's domain is the selected splats"
    # the whole-wave skip: some wave's 64 bits are clear in alt2 and not all are
    if c.n >= 256:
        alt2 = c.masks(pkg)["alt2"][0]
        waves = np.add.reduceat(alt2.astype(np.int64), np.arange(0, c.n, 64))
        assert (waves == 0).any() and (waves == 64).any()


# ---- (c) the empty selection and the empty cloud ----------------------------------------------------------------------------------------
def _assert_empty(res, n_hist_words):
    u32 = lambda a: np.asarray(list(a), np.float32).view(np.uint32)
    assert (res.n_selected, res.n_measured, res.n_extent) == (0, 0, 0)
    for lo, hi in ((res.lo, res.hi), (res.lo_e, res.hi_e)):
        assert (u32(lo) == 0x7f800000).all() and (u32(hi) == 0xff800000).all()
    assert (np.asarray(list(res.sum)).view(np.uint64) == 0).all()
    assert sum(h.size for h in res.hist) == n_hist_words and all((h == 0).all() for h in res.hist)


def test_the_empty_selection_and_the_empty_cloud(pkg):
    E = pkg.engine
    c = MC.case(pkg, "n257_sh")
    words = sum(b + 3 for _, _, _, b, _ in MC.HISTS_A)
    _assert_empty(_ev(pkg, c, MC.request(pkg, 7, MC.HISTS_A), c.masks(pkg)["none"][1]), words)
    _assert_empty(E.measure_eval(MC.request(pkg, 7, MC.HISTS_A), n=0), words)
    _assert_empty(E.measure_eval(MC.request(pkg, 7), np.zeros((0, 3), np.float32)), 0)
    res = E.measure_eval(MC.request(pkg, 7), n=0)
    assert np.isnan(res.centroid()).all() and np.isnan(res.covariance()).all()


def test_centroid_and_covariance(pkg):
    c = MC.case(pkg, "n257_nosh")
    sel = c.masks(pkg)["random"][0]
    res = _ev(pkg, c, MC.request(pkg, 4), sel)
    P = c.splats.P[sel & np.isfinite(c.splats.P).all(axis=1)].astype(np.float64)
    assert res.centroid().dtype == np.float64 and res.covariance().dtype == np.float64 and res.covariance().shape == (3, 3)
    # (derived values: the sums are exact to the bit above; the centre and the spread are what numpy gives to rounding.  d = p - ref is
    # rounded to float32 first: half an ulp of 2048, 6.1e-5, per splat.)
    assert np.allclose(res.centroid(), P.mean(axis=0), rtol=0, atol=1e-4)
    assert np.allclose(res.covariance(), np.cov(P.T, bias=True), rtol=0, atol=1e-3)


# ---- (d) SKIP_HIDDEN with volumes and with a mask -----------------------------------------------------------------------------------------
def test_skip_hidden(pkg):
    E = pkg.engine
    c = MC.case(pkg, "n257_nosh")
    s = c.splats
    hide = np.arange(c.n) % 5 == 1
    vols = [E.crop_box(tuple(float(v) for v in MC.OFFSET + np.float32([0.3, 0.0, 0.0])), 0.8)]
    vis, keep = E.visibility_struct(vols, hide)
    visible = E.visibility_eval(vis, s.P)
    assert (~visible).sum() > 20 and visible.sum() > 20
    sel, words = c.masks(pkg)["random"]
    for what, hists in ((7, MC.HISTS_A), (0, MC.HISTS_B), (4, ())):
        plain = _ev(pkg, c, MC.request(pkg, what, hists), words)
        # without the flag a visibility changes nothing; with it the hidden splats are not selected; with no visibility nothing is hidden
        assert MC.same_result(_ev(pkg, c, MC.request(pkg, what, hists), words, vis=vis), plain)
        assert MC.same_result(_ev(pkg, c, MC.request(pkg, what, hists, skip_hidden=True), words), plain)
        got = _ev(pkg, c, MC.request(pkg, what, hists, skip_hidden=True), words, vis=vis)
        MC.assert_result(got, c.restate(pkg, "random", hists, hidden=~visible), what, f"skip hidden {what}", n_hist=len(hists))
        assert got.n_selected == int((sel & visible).sum()) < plain.n_selected
    # a mask alone needs no positions
    vm, keep2 = E.visibility_struct((), hide)
    req = MC.request(pkg, 0, (MC.HISTS_A[0],), skip_hidden=True)
    got = E.measure_eval(req, alpha=s.alpha, vis=vm)
    assert got.n_selected == int((~hide).sum()) and np.array_equal(got.hist[0], MC.histogram(s.alpha[~hide], *MC.HISTS_A[0][1:]))


# ---- (e) refusals --------------------------------------------------------------------------------------------------------------------------
def test_hist_prepare_refusals(pkg):
    L, E = pkg.load_library(), pkg.engine
    out = E.gsr_hist_spec()
    out.bins = -5
    bad = [(9, 0, 0.0, 1.0, 8), (-1, 0, 0.0, 1.0, 8), (0, 2, 0.0, 1.0, 8), (0, -1, 0.0, 1.0, 8), (0, 0, 0.0, 1.0, 0), (0, 0, 0.0, 1.0, 257),
           (0, 0, 0.0, 1.0, -1), (0, 0, 1.0, 1.0, 8), (0, 0, 2.0, 1.0, 8), (0, 0, NAN, 1.0, 8), (0, 0, 0.0, NAN, 8), (0, 0, -INF, 1.0, 8),
           (0, 0, 0.0, INF, 8), (0, 0, 0.0, 1e39, 8), (0, 0, 1.0, 1.0 + 1e-12, 8),      # (equal as float32)
           (0, 0, 0.0, 1e-44, 256)]                                                      # (inv_w overflows float32)
    for args in bad:
        assert L.gsr_hist_prepare(*args, C.byref(out)) == GSR_E_INVALID and b"gsr_hist_prepare" in L.gsr_last_error(), args
    assert L.gsr_hist_prepare(0, 0, 0.0, 1.0, 8, None) == GSR_E_INVALID
    assert out.bins == -5, "a refusal wrote the spec"
    for ch in range(9):
        for flags in (0, 1):
            assert L.gsr_hist_prepare(ch, flags, -1.0, 3.0, 256, C.byref(out)) == 0
            assert (out.channel, out.flags, out.bins, out.lo, out.hi, out.inv_w) == (ch, flags, 256, -1.0, 3.0, 64.0)
    with pytest.raises(E.GsrError):
        E.hist_spec(E.HIST_X, 1.0, 0.0, 4)


def _bad_requests(pkg):
    """every field value the library refuses: (label, request)"""
    out = []

    def bad(label, spec=None, **fields):
        r = MC.request(pkg, 7, MC.HISTS_A)
        for k, v in fields.items():
            if k == "ref":
                r.ref[v[0]] = v[1]
            else:
                setattr(r, k, v)
        for k, v in (spec or {}).items():
            setattr(r.hist[2], k, v)
        out.append((label, r))

    bad("what bit 8", what=8 | 1)
    bad("what bit 1 << 30", what=1 << 30)
    bad("flags 2", flags=2)
    bad("reserved_ 1", reserved_=1)
    bad("ref NaN", ref=(1, NAN))
    bad("ref inf", ref=(2, INF))
    bad("extent_k NaN", extent_k=NAN)
    bad("extent_k -inf", extent_k=-INF)
    bad("n_hist 5", n_hist=5)
    bad("n_hist -1", n_hist=-1)
    bad("spec channel 9", spec={"channel": 9})
    bad("spec channel -1", spec={"channel": -1})
    bad("spec flags 2", spec={"flags": 2})
    bad("spec bins 0", spec={"bins": 0})
    bad("spec bins 257", spec={"bins": 257})
    bad("spec hi == lo", spec={"hi": 998.5})
    bad("spec lo NaN", spec={"lo": NAN})
    bad("spec hi inf", spec={"hi": INF})
    bad("spec inv_w 0", spec={"inv_w": 0.0})
    bad("spec inv_w NaN", spec={"inv_w": NAN})
    bad("spec inv_w inf", spec={"inv_w": INF})
    bad("spec inv_w negative", spec={"inv_w": -1.0})
    return out


def test_eval_refusals_write_nothing(pkg):
    L, E = pkg.load_library(), pkg.engine
    c = MC.case(pkg, "n63_sh")
    s = c.splats
    res = E.gsr_measure_result()
    res.n_selected = -9
    hist = np.full(1200, 9, np.uint32)
    arrs = [s.P.ctypes.data, s.alpha.ctypes.data, s.scale.ctypes.data, s.Cd.ctypes.data]
    ok = MC.request(pkg, 7, MC.HISTS_A)

    def call(r=ok, vis=None, n=c.n, mask=None, a=arrs, out=res, h=hist.ctypes.data):
        return L.gsr_measure_eval(C.byref(r) if r is not None else None, C.byref(vis) if vis is not None else None, n, mask, *a,
                                  C.byref(out) if out is not None else None, h)

    for label, r in _bad_requests(pkg):
        assert call(r) == GSR_E_INVALID and b"gsr_measure_eval" in L.gsr_last_error(), label
    assert call(None) == GSR_E_INVALID and call(out=None) == GSR_E_INVALID
    assert call(n=-1) == GSR_E_INVALID and call(n=1 << 31) == GSR_E_INVALID
    assert call(h=None) == GSR_E_INVALID                                       # n_hist > 0 without hist_out
    assert call(MC.request(pkg, 7)) == GSR_E_INVALID                           # ... and hist_out with n_hist == 0
    for k, (name, what, hists) in enumerate((("P", 1, ()), ("alpha", 0, (MC.HISTS_A[0],)), ("scale", 2, ()), ("Cd", 0, (MC.HISTS_A[3],)))):
        a = list(arrs)
        a[k] = None
        h = hist.ctypes.data if hists else None
        assert call(MC.request(pkg, what, hists), a=a, h=h) == GSR_E_INVALID, name
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)], np.zeros(c.n - 1, bool))
    skip = MC.request(pkg, 7, MC.HISTS_A, skip_hidden=True)
    assert call(skip, vis=vis) == GSR_E_INVALID                                # the visibility's mask does not cover the splats
    vis.n_volumes = 7
    assert call(skip, vis=vis) == GSR_E_INVALID                                # a visibility gsr_set_visibility would refuse
    vis, keep = E.visibility_struct([E.crop_box((0, 0, 0), 1.0)])
    a = list(arrs)
    a[0] = None
    assert call(MC.request(pkg, 0, (MC.HISTS_A[0],), skip_hidden=True), vis=vis, a=a) == GSR_E_INVALID     # SKIP_HIDDEN by volumes needs P
    assert res.n_selected == -9 and (hist == 9).all(), "a refusal wrote something"
    # what the request does not look at may be NULL
    assert call(MC.request(pkg, 0, (MC.HISTS_A[0],)), a=[None, arrs[1], None, None]) == 0 and res.n_selected == c.n
    assert call(MC.request(pkg, 0), a=[None] * 4, h=None) == 0 and res.n_selected == c.n and res.n_measured == 0


def test_context_refusals_without_a_gpu(pkg):
    L = pkg.load_library()
    r = MC.request(pkg, 7)
    res = pkg.engine.gsr_measure_result()
    res.n_selected = -9
    w = np.full(2, 0xdeadbeef, np.uint32)
    assert L.gsr_measure(None, w.ctypes.data, 0, C.byref(r), C.byref(res), None) == GSR_E_INVALID
    assert L.gsr_multi_measure(None, w.ctypes.data, C.byref(r), C.byref(res), None) == GSR_E_INVALID
    assert L.gsr_get_measure(None, None, None, None) == GSR_E_INVALID
    assert res.n_selected == -9 and (w == 0xdeadbeef).all()


# ---- (f) the header and the Python door --------------------------------------------------------------------------------------------------
def test_header_constants_structs_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("MEASURE_BOUNDS", 1), ("MEASURE_EXTENT", 2), ("MEASURE_MOMENTS", 4), ("MEASURE_SKIP_HIDDEN", 1), ("HIST_X", 0), ("HIST_Y", 1),
                        ("HIST_Z", 2), ("HIST_ALPHA", 3), ("HIST_SCALE_MAX", 4), ("HIST_SCALE_MIN", 5), ("HIST_CD_R", 6), ("HIST_CD_G", 7), ("HIST_CD_B", 8),
                        ("HIST_LOG2", 1), ("HIST_MAX_BINS", 256), ("MEASURE_MAX_HIST", 4)):
        assert int(re.search(r"#define GSR_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(E, name), name
    for struct in ("gsr_hist_spec", "gsr_measure_request", "gsr_measure_result"):
        body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        body = body[body.index("{") + 1:]
        names = []
        for decl in body.split(";"):
            m = re.match(r"\s*(?:int64_t|int32_t|float|double|gsr_hist_spec)\s+(.*)", decl.strip(), flags=re.S)
            if m:
                names += [re.sub(r"\[.*", "", x.strip()) for x in m.group(1).split(",")]
        assert names == [n for n, _ in getattr(E, struct)._fields_], (struct, names)
    assert C.sizeof(E.gsr_hist_spec) == 24 and E.gsr_hist_spec.inv_w.offset == 20
    R = E.gsr_measure_request
    assert C.sizeof(R) == 128 and (R.ref.offset, R.extent_k.offset, R.n_hist.offset, R.hist.offset, R.reserved_.offset) == (8, 20, 24, 28, 124)
    S = E.gsr_measure_result
    assert C.sizeof(S) == 144 and (S.n_extent.offset, S.lo.offset, S.hi.offset, S.lo_e.offset, S.hi_e.offset, S.sum.offset) == (16, 24, 36, 48, 60, 72)
    for sym in ("gsr_measure", "gsr_measure_eval", "gsr_hist_prepare", "gsr_get_measure", "gsr_multi_measure"):
        assert hasattr(L, sym) and sym in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % sym, hdr), sym
    for name in ("measure_request", "hist_spec", "measure_eval"):
        assert callable(getattr(E, name)), name
    for name in ("measure", "measure_device", "get_measure"):
        assert callable(getattr(pkg.Engine, name)), name
    assert callable(pkg.MultiEngine.measure)


def test_request_builder(pkg):
    E = pkg.engine
    r = E.measure_request()
    assert (r.what, r.flags, list(r.ref), r.extent_k, r.n_hist, r.reserved_) == (0, 0, [0.0] * 3, 0.0, 0, 0)
    h = E.hist_spec(E.HIST_SCALE_MIN, -6, 2, 16, log2=True)
    assert (h.channel, h.flags, h.bins, h.lo, h.hi, h.inv_w) == (5, 1, 16, -6.0, 2.0, 2.0)
    r = E.measure_request(bounds=True, extent=2.5, moments=True, ref=(1, 2, 3), hists=[h, h], skip_hidden=True)
    assert (r.what, r.flags, list(r.ref), r.extent_k, r.n_hist) == (7, 1, [1.0, 2.0, 3.0], 2.5, 2)
    assert bytes(r.hist[1]) == bytes(h)
    assert E.measure_request(extent=0.0).what == E.MEASURE_EXTENT
    with pytest.raises(E.GsrError):
        E.measure_eval(E.measure_request(bounds=True), P=np.zeros((2, 3), np.float32), alpha=np.zeros(3, np.float32))


# ---- (g) the LOG2 replacement ----------------------------------------------------------------------------------------------------------------
def test_log2_replacement(pkg):
    """the replacement is exact at powers of two, piecewise-linear between them and monotone, denormals included; the library bins what
    the integer restatement bins, for every bin edge an exact power of two can sit on"""
    E = pkg.engine
    f32 = np.float32
    pow2 = (2.0 ** np.arange(-149, 128)).astype(f32)
    assert np.array_equal(MC.log2_linear(pow2[23:]), np.arange(-126, 128).astype(f32))     # the normal powers of two: their exponent
    assert MC.log2_linear(np.array([1.5, 0.75, 3.0], f32)).tolist() == [0.5, -0.5, 1.5]     # linear in the mantissa
    rng = np.random.default_rng(3)
    x = np.concatenate([pow2, np.nextafter(pow2, f32(0)), np.nextafter(pow2, f32(np.inf)), np.exp(rng.uniform(-100, 88, 4000)).astype(f32),
                        rng.integers(1, 1 << 23, 200).astype(np.uint32).view(f32),              # denormals
                        np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, np.finfo(f32).max], f32)])
    v = MC.log2_linear(np.sort(x[np.isfinite(x) & (x > 0)]))
    assert (np.diff(v) >= 0).all()
    for lo, hi, bins in ((-150.0, 128.0, 256), (-127.0, -126.0, 7), (-8.0, 8.0, 16), (0.0, 1.0, 255), (-149.5, 127.5, 111)):
        spec = E.hist_spec(E.HIST_ALPHA, lo, hi, bins, log2=True)
        got = E.measure_eval(E.measure_request(hists=[spec]), alpha=x)
        assert np.array_equal(got.hist[0], MC.histogram(x, lo, hi, bins, True)), (lo, hi, bins)
        assert got.hist[0][bins + 2] == 1 and got.hist[0][bins] >= 4 and got.hist[0][bins + 1] >= 1      # NaN; 0, -0, -1, -inf; +inf


# ---- (h) from the code object ----------------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): k_measure and k_measure_fold are there,
    once each, use no scratch, and k_measure stays within 64 VGPRs (eight waves per SIMD) and the LDS of four histograms
    (4 x 259 words), the tree's two buffers of 4 x 9 doubles and the final 4 x 16 words"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    main = {k: v for k, v in rows.items() if re.match(r"_Z9k_measure", k)}
    fold = {k: v for k, v in rows.items() if re.match(r"_Z14k_measure_fold", k)}
    assert len(main) == 1 and len(fold) == 1, (sorted(main), sorted(fold))
    for name, (vg, sg, lds, scratch) in list(main.items()) + list(fold.items()):
        print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}")
        assert scratch == 0 and vg <= 64, (name, vg, sg, lds, scratch)
    (vg, sg, lds, scratch), = main.values()
    assert lds <= 4 * 259 * 4 + 2 * 4 * 9 * 8 + 4 * 16 * 4, lds
