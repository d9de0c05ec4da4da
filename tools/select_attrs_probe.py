"""gsr_select_attrs beside k_select and beside the only way there was before it, in one session:
    python tools/select_attrs_probe.py [C4] [--reps 20] [--n N]
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), from the verbs' own clocks (gsr_get_select_attrs /
gsr_get_select: kernel, copies, wall), every call into a DEVICE mask (REPLACE):
 (a)  the alpha clause alone (a trainer's opacity prune)                          -- one 16-byte geoA gather per splat, as k_select's
 (b)  alpha + scale_max + scale_min + anisotropy (size and needle prune)           -- + one 16-byte geoB gather
 (c)  every clause, with one box                                                   -- + one 16-byte gather of colour chunk 0
 (k)  k_select with a whole-frame rect, on the config's first orbit camera         -- the yardstick of (a)
 (0)  the only way before: Engine.read of P, alpha, scale and Cd, the predicate of (c) in numpy, the mask packed and copied back to
      the device
Each device mask is compared with gsr_select_attrs_eval over the whole cloud (the rule on the host).  Bandwidth: the bytes a splat's
lane moves (the 4-byte inverse of the storage order, its 16-byte gathers, 1/8 byte of mask) over the kernel time, beside the HBM peak
tools/ubench_hbm measures in the same session (built by __graft_entry__.build())."""
import ctypes as C
import json
import os
import subprocess
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

# the rules: thresholds about the cloud's own medians, so that each clause keeps part of it
sc = np.abs(splats.scale.view(np.float16).astype(np.float32))
smax, smin = sc.max(axis=1), sc.min(axis=1)
a_lo = float(np.quantile(splats.alpha, 0.3))
rules = {
    "(a) alpha": dict(alpha=(a_lo, np.inf)),
    "(b) alpha + scales + anisotropy": dict(alpha=(a_lo, np.inf), scale_max=(0.0, float(np.quantile(smax, 0.9))),
                                            scale_min=(float(np.quantile(smin, 0.05)), np.inf), anisotropy=2.0),
    "(c) every clause, one box": dict(alpha=(a_lo, np.inf), scale_max=(0.0, float(np.quantile(smax, 0.9))),
                                      scale_min=(float(np.quantile(smin, 0.05)), np.inf), anisotropy=2.0, colour=(0.05, 0.95),
                                      volumes=[E.crop_box((0.0, 0.0, 0.0), 0.8)]),
}
lane_bytes = {"(a) alpha": 16, "(b) alpha + scales + anisotropy": 32, "(c) every clause, one box": 48}


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


def clocks(get, call):
    out = []
    for r in range(reps + 1):
        call()
        if r:
            out.append(get()["ms"])
    return np.asarray(out)


def hbm_peak():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ubench_hbm")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe, "--json"], capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
    return json.loads(out[-1]) if out else None


print("%s: %d splats, SH %s, %dx%d; median [min .. max] of %d calls, ms" % (name, n, splats.shx is not None, W, H, reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    dmask = device_room(words * 4)

    def check(label, rule):
        got = np.empty(words, np.uint32)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dmask, C.c_size_t(got.nbytes), 2) == 0
        want = E.select_attrs_eval(rule, splats.P, splats.alpha, splats.scale, splats.Cd)
        assert np.array_equal(got, E.pack_mask(want)), label + ": the device mask is not the host rule's"
        return int(want.sum())

    kern = {}
    for label, kw in rules.items():
        rule = E.attr_rule(**kw)
        ms = clocks(eng.get_select_attrs, lambda: eng.select_attrs_device(rule, dmask.value))
        hits = check(label, rule)
        kern[label] = ms[:, 0]
        print("%-34s kernel %s   wall %s   hits %d (%.3f of the cloud)" % (label, cell(ms[:, 0]), cell(ms[:, 3]), hits, hits / n), flush=True)
    cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
    cs = E.camera_struct(cam)
    ms = clocks(eng.get_select, lambda: eng.select_device(cs, E.select_region(None), dmask.value))
    kern["(k)"] = ms[:, 0]
    print("%-34s kernel %s   wall %s" % ("(k) k_select, whole-frame rect", cell(ms[:, 0]), cell(ms[:, 3])), flush=True)
    a, k = kern["(a) alpha"], kern["(k)"]
    print("(a) against (k): median %.4f vs %.4f ms; (a)'s median %s k_select's spread [%.4f .. %.4f]"
          % (np.median(a), np.median(k), "lies within" if np.min(k) <= np.median(a) <= np.max(k) else "lies OUTSIDE", np.min(k), np.max(k)), flush=True)

    peak = hbm_peak()
    for label, b in lane_bytes.items():
        per = b + 4 + 1.0 / 8.0                 # (the default storage order: every gather goes through the 4-byte inverse)
        gbs = n * per / (np.median(kern[label]) * 1e-3) / 1e9
        print("%-34s %.1f bytes per splat -> %.0f GB/s%s" % (label, per, gbs, "" if not peak else " = %.2f of the measured peak %.0f GB/s (read-only %.0f)"
                                                            % (gbs / peak["peak_GBps"], peak["peak_GBps"], peak.get("read_GBps", 0.0))), flush=True)

    # ---- the only way before: the four arrays over the link, the predicate of (c) in numpy, the mask back
    kw = rules["(c) every clause, one box"]
    box = E.visibility_struct(kw["volumes"])[0]
    read_ms, host_ms, back_ms, before_hits = [], [], [], 0
    for r in range(max(3, reps // 4) + 1):
        t0 = time.perf_counter()
        R = eng.read(names=("P", "alpha", "scale", "Cd"))
        t1 = time.perf_counter()
        s = np.abs(R.scale.view(np.float16).astype(np.float32))
        c = R.Cd.view(np.float16).astype(np.float32)
        hi_, lo_ = s.max(axis=1), s.min(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            sel = (R.alpha >= np.float32(kw["alpha"][0])) & (hi_ <= np.float32(kw["scale_max"][1])) & (lo_ >= np.float32(kw["scale_min"][0])) & \
                  (hi_ > 0) & (hi_ >= np.float32(2.0) * lo_) & ((c >= np.float32(0.05)) & (c <= np.float32(0.95))).all(axis=1) & \
                  E.visibility_eval(box, R.P)
        host_words = E.pack_mask(sel)
        t2 = time.perf_counter()
        assert hip.hipMemcpy(dmask, C.c_void_p(host_words.ctypes.data), C.c_size_t(host_words.nbytes), 1) == 0
        t3 = time.perf_counter()
        if r:
            read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3); back_ms.append((t3 - t2) * 1e3)
        before_hits = int(sel.sum())
    print("(0) before: Engine.read of P, alpha, scale, Cd %s   numpy predicate + packing %s   mask to the device %s   (%.0f MB over the link; "
          "%d hits)" % (cell(read_ms), cell(host_ms), cell(back_ms), n * (12 + 4 + 6 + 6) / 1e6, before_hits), flush=True)
    hip.hipFree(dmask)
