"""gsr_grade beside the only way there was before it, in one session:
    python tools/grade_probe.py [C4] [--reps 20] [--n N]
    rocprofv3 --kernel-trace --stats -- python tools/grade_probe.py [C4] --kernels     # a run of its own: k_grade beside k_update<true> and k_transform<true>
Medians [min .. max] of `reps` calls from the verb's own stage clock (gsr_get_grade: mask copy and count, the kernel between HIP events,
the visibility rule, wall).  Every call changes the cloud, so every call gets a FRESH context (create, upload, one unmeasured frame).
 (1)  the whole cloud (NULL mask)
 (2)  the ~10 % a gsr_select box hits, from the DEVICE mask the select wrote
 (3)  1 % of the cloud (a contiguous range in the middle) from a HOST mask
 (4)  beside them, over the same splats in the same session: gsr_update of Cd, SH and alpha of the whole cloud (k_update<true> between
      its HIP events, gsr_stats.upload_ms[5]) and gsr_transform of the whole cloud (gsr_get_transform: kernel .. sort)
 (5)  the only way before, its three parts timed separately: gsr_read of Cd, SH and alpha; engine.grade_eval on the host; gsr_update
      with them -- for the whole cloud
--kernels: no clocks; `reps` rounds of [update_attrs of Cd, SH and alpha of the whole cloud (k_update<true>), a whole-cloud transform
(k_transform<true>), a whole-cloud grade (k_grade<true>)] for a kernel trace: the three kernels work over the same splats in one
work shape, and that comparison is k_grade's yardstick."""
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
kernels_only = "--kernels" in sys.argv
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n, W, H = splats.n, cfg["width"], cfg["height"]
words = (n + 31) // 32
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")
cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
cs = E.camera_struct(cam)
rule = E.grade_prepare(E.grade_params(exposure=0.4, gain=(1.1, 0.95, 0.8), saturation=1.3, contrast=1.2, pivot=0.45, offset=(0.03, -0.02, 0.01),
                                      alpha_gain=0.8, alpha_offset=0.05))
colour_only = dict(rule, ag=1.0, ab=0.0, flags=E.GRADE_COLOUR)
x = E.xform(axis_angle=((1.0, 2.0, 3.0), 37.0), scale=1.1, translate=(0.05, -0.02, 0.03))
attrs = ("Cd", "alpha", "shx", "shy", "shz") if splats.has_sh else ("Cd", "alpha")
rows = {k: getattr(splats, k) for k in attrs}


def fresh():
    eng = pkg.Engine(0)
    eng.upload(splats)
    eng.render(cam)
    return eng


if kernels_only:
    with fresh() as eng:
        for r in range(reps):
            eng.update_attrs(0, **rows)
            eng.transform(x, None)
            eng.grade(rule, None)
    print("rounds:", reps)
    sys.exit(0)

print("%s: %d splats, SH %s, %dx%d; median [min .. max] of %d calls, ms" % (name, n, "yes" if splats.has_sh else "no", W, H, reps), flush=True)
s = np.sqrt(0.1)
rect = (W * (0.5 - s / 2), H * (0.5 - s / 2), W * (0.5 + s / 2), H * (0.5 + s / 2))
part = np.zeros(n, bool)
part[n // 2:n // 2 + max(n // 100, 1)] = True
part_words = E.pack_mask(part)
dmask = C.c_void_p()
assert hip.hipMalloc(C.byref(dmask), C.c_size_t(words * 4)) == 0


def case(label, call, what=rule):
    ms, wall, graded = [], [], 0
    for r in range(reps):
        with fresh() as eng:
            call(eng, what, True)
            eng.synchronize()
            t0 = time.perf_counter()
            graded = call(eng, what, False)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.get_grade()["ms"])
    ms = np.asarray(ms)
    print("%-44s mask copy + count %s   k_grade %s   wall %s   graded %d (%.3f of the cloud)"
          % (label, cell(ms[:, 0]), cell(ms[:, 1]), cell(wall), graded, graded / n), flush=True)


def whole(eng, what, prepare):
    return None if prepare else eng.grade(what, None)


def boxed(eng, what, prepare):
    if prepare:
        return eng.select_device(cs, E.select_region(rect), dmask.value)
    return eng.grade_device(what, dmask.value)


def one_percent(eng, what, prepare):
    return None if prepare else eng.grade(what, part_words)


case("(1) whole cloud, NULL mask", whole)
case("(1c) whole cloud, colour only", whole, colour_only)
case("(2) a select box, device mask", boxed)
case("(3) 1 %%, host mask (%.2f MB)" % (words * 4 / 1e6), one_percent)

# ---- beside them: k_update<true> and the transform's kernel .. sort over the same splats
upd_ms, xf_ms = [], []
for r in range(reps):
    with fresh() as eng:
        eng.update_attrs(0, **rows)
        upd_ms.append(eng.stats()["upload_ms"][5])
        eng.transform(x, None)
        xf_ms.append(eng.get_transform()["ms"][1])
print("(4) gsr_update of Cd, SH, alpha: k_update between its events %s   gsr_transform: kernel .. sort %s" % (cell(upd_ms), cell(xf_ms)), flush=True)

# ---- the only way before: the colour arrays and alpha over the link, the host rule, an update with them
names = attrs
read_ms, host_ms, back_ms = [], [], []
for r in range(max(3, reps // 4)):
    with fresh() as eng:
        eng.synchronize()
        t0 = time.perf_counter()
        back = eng.read(names=names)
        t1 = time.perf_counter()
        full = pkg.scenes.Splats(splats.P, back.Cd, back.alpha, splats.scale, splats.orient, back.shx, back.shy, back.shz)
        out = E.grade_eval(rule, full, None)
        t2 = time.perf_counter()
        eng.update_attrs(0, **{k: getattr(out, k) for k in names})
        t3 = time.perf_counter()
        read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3); back_ms.append((t3 - t2) * 1e3)
row = 6 + 4 + (96 if splats.has_sh else 0)
print("(before) gsr_read %s   grade_eval on the host %s   gsr_update %s   (%.0f MB each way)"
      % (cell(read_ms), cell(host_ms), cell(back_ms), n * row / 1e6), flush=True)
hip.hipFree(dmask)
