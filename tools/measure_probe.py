"""gsr_measure beside k_select and beside the only way there was before it, in one session:
    python tools/measure_probe.py [C4] [--reps 20] [--n N]
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), from the verbs' own clocks (gsr_get_measure: k_measure,
the launches that finish the sums, copies, wall; gsr_get_select: kernel, copies, wall), every call from a DEVICE mask:
 (1)   bounds + moments of a 1 % selection (one contiguous run of upload indices: most waves skip)
 (10)  ... of a 10 % selection (random splats: every wave has lanes to load)
 (100) ... of the whole cloud                                                    -- one 16-byte geoA gather per splat, as k_select's
 (e)   bounds + extent + moments of the whole cloud                              -- + one 16-byte geoB gather
 (h)   four 256-bin histograms of the whole cloud: alpha, log2 scale_max, x, Cd green -- geoA, geoB and colour chunk 0, no tree
 (*)   everything at once
 (k)   k_select with a whole-frame rect, on the config's first orbit camera      -- the yardstick: the same mask pass and geoA gather
 (0)   the only way before: Engine.read of P, the centroid, bounds and second moments in numpy
Each result is compared with gsr_measure_eval over the whole cloud (the rule on the host), bit for bit."""
import ctypes as C
import sys
import time

sys.path.insert(0, '.')
import numpy as np
import __graft_entry__ as ge

pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
reps = int(opt("--reps", "20"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n, W, H = splats.n, cfg["width"], cfg["height"]
words = (n + 31) // 32
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")

rng = np.random.default_rng(1)
one = np.zeros(n, bool)
one[n // 3: n // 3 + n // 100] = True
masks = {"1 %": one, "10 %": rng.random(n) < 0.1, "100 %": np.ones(n, bool)}
ref = tuple(float(v) for v in splats.P[np.isfinite(splats.P).all(axis=1)][:1000].mean(axis=0))
hists = [E.hist_spec(E.HIST_ALPHA, 0.0, 1.0, 256), E.hist_spec(E.HIST_SCALE_MAX, -12.0, 2.0, 256, log2=True),
         E.hist_spec(E.HIST_X, float(np.nanmin(splats.P[:, 0])), float(np.nanmax(splats.P[:, 0])) + 1e-3, 256), E.hist_spec(E.HIST_CD_G, 0.0, 1.0, 256)]
bm = E.measure_request(bounds=True, moments=True, ref=ref)
runs = [("(1)   bounds + moments, 1 %", bm, "1 %"), ("(10)  bounds + moments, 10 %", bm, "10 %"), ("(100) bounds + moments, 100 %", bm, "100 %"),
        ("(e)   bounds + extent + moments, 100 %", E.measure_request(bounds=True, extent=3.0, moments=True, ref=ref), "100 %"),
        ("(h)   four 256-bin histograms, 100 %", E.measure_request(hists=hists), "100 %"),
        ("(*)   everything at once, 100 %", E.measure_request(bounds=True, extent=3.0, moments=True, ref=ref, hists=hists), "100 %")]


def device_words(w):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(w.nbytes, 4))) == 0
    assert hip.hipMemcpy(p, C.c_void_p(w.ctypes.data), C.c_size_t(w.nbytes), 1) == 0
    return p


def clocks(get, call):
    out = []
    for r in range(reps + 1):
        call()
        if r:
            out.append(get()["ms"])
    return np.asarray(out)


def same(a, b):
    return bytes(a) == bytes(b) and all(np.array_equal(x, y) for x, y in zip(a.hist, b.hist))


print("%s: %d splats, SH %s, %dx%d; median [min .. max] of %d calls, ms" % (name, n, splats.shx is not None, W, H, reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    dmasks = {k: device_words(E.pack_mask(m)) for k, m in masks.items()}
    kern = {}
    for label, req, which in runs:
        got = [None]

        def call():
            got[0] = eng.measure_device(req, dmasks[which].value)
        ms = clocks(eng.get_measure, call)
        want = E.measure_eval(req, splats.P, splats.alpha, splats.scale, splats.Cd, mask=masks[which])
        assert same(got[0], want), label + ": the result is not the host rule's"
        kern[label] = ms[:, 0]
        print("%-40s k_measure %s   fold %s   copies %s   wall %s   measured %d" % (label, cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 2]), cell(ms[:, 3]),
                                                                                     got[0].n_measured), flush=True)
    cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
    cs = E.camera_struct(cam)
    ms = clocks(eng.get_select, lambda: eng.select_device(cs, E.select_region(None), dmasks["1 %"].value))
    k = ms[:, 0]
    print("%-40s kernel %s   wall %s" % ("(k)   k_select, whole-frame rect", cell(ms[:, 0]), cell(ms[:, 3])), flush=True)
    for label, v in kern.items():
        print("%-40s %.2f x k_select (median %.4f vs %.4f ms)" % (label, np.median(v) / np.median(k), np.median(v), np.median(k)), flush=True)

    # ---- the only way before: P over the link, the same figures in numpy
    read_ms, host_ms = [], []
    for r in range(max(3, reps // 4) + 1):
        t0 = time.perf_counter()
        R = eng.read(names=("P",))
        t1 = time.perf_counter()
        P = R.P[masks["100 %"] & np.isfinite(R.P).all(axis=1)].astype(np.float64)
        centre, lo, hi = P.mean(axis=0), P.min(axis=0), P.max(axis=0)
        cov = np.cov(P.T, bias=True)
        t2 = time.perf_counter()
        if r:
            read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3)
    print("(0) before: Engine.read of P %s   centroid, bounds, covariance in numpy %s   (%.0f MB over the link)" % (cell(read_ms), cell(host_ms), n * 12 / 1e6),
          flush=True)
    for p in dmasks.values():
        hip.hipFree(p)
