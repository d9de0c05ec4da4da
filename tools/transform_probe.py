"""gsr_transform beside the only way there was before it, in one session:
    python tools/transform_probe.py [C4] [--reps 20] [--n N]
    rocprofv3 --kernel-trace --stats -- python tools/transform_probe.py [C4] --kernels     # a run of its own: k_transform beside k_update<true> and k_repack<true>
Medians [min .. max] of `reps` calls from the verb's own stage clock (gsr_get_transform: mask over the link, kernel .. sort, repack, wall).
Every call changes the cloud, so every call gets a FRESH context (create, upload, one unmeasured frame), whose first transform also
allocates the spare planes: that is in the wall time and in none of the stage times.
 (1)  the whole cloud (NULL mask)
 (2)  the ~10 % a gsr_select box hits, from the DEVICE mask the select wrote
 (3)  1 % of the cloud (a contiguous range in the middle) from a HOST mask
 (4)  the only way before, its three parts timed separately: gsr_read of P, scale, orient and SH; engine.transform_eval on the host;
      gsr_move with the attributes -- for the whole cloud
Then a check that is recorded, not asserted (--check: only this): the whole cloud is rotated by a generic rotation about the origin and
the frame is compared with the untransformed frame, max and mean |delta| per channel, (a) with the camera's object matrix set to the
inverse and (b) from the camera turned along with the cloud.  (b) is the pixel cost of re-quantising orient, scale and SH to halves.
(a) also holds what the vertex stage does under ANY object matrix that rotates: it forms the SH direction as
inv_object3 (P_object - camera_world), object-space position minus world-space camera, so a rotation in the object matrix does not turn
the view direction the way it turns the cloud.
--kernels: no clocks; `reps` rounds of [update_attrs of every attribute of the whole cloud (k_update<true>), a whole-cloud move
(k_repack<true>), a whole-cloud transform (k_transform<true>, and its own k_repack)] for a kernel trace: the three kernels move comparable
bytes over the same splats, and that comparison is k_transform's yardstick."""
import ctypes as C
import dataclasses
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
centre = 0.5 * (splats.P.min(axis=0) + splats.P.max(axis=0))
x = E.xform(axis_angle=((1.0, 2.0, 3.0), 37.0), scale=1.1, translate=(0.05, -0.02, 0.03), pivot=tuple(float(v) for v in centre))
attrs = ("Cd", "alpha", "scale", "orient", "shx", "shy", "shz") if splats.has_sh else ("Cd", "alpha", "scale", "orient")


def fresh():
    eng = pkg.Engine(0)
    eng.upload(splats)
    eng.render(cam)
    return eng


if kernels_only:
    with fresh() as eng:
        rows = {k: getattr(splats, k) for k in attrs}
        for r in range(reps):
            eng.update_attrs(0, **rows)
            eng.move(0, splats.P)
            eng.transform(x, None)
    print("rounds:", reps)
    sys.exit(0)

# ---- recorded, not asserted: rotate the cloud, counter-rotate what looks at it, compare with the untransformed frame
def check():
    rot = E.xform(axis_angle=((1.0, 2.0, 3.0), 37.0))
    R = np.eye(4)
    R[:3, :3] = E.xform_prepare(rot)["A"].astype(np.float64)         # (the pivot is the origin: p' = R p)
    view = np.asarray(cam.view, np.float64).reshape(4, 4).T
    obj = np.asarray(cam.object, np.float64).reshape(4, 4).T
    gl = pkg.camera._gl
    # (a) the camera's OBJECT MATRIX set to the inverse: object' = object R^-1 (column vectors; R^-1 = R^T)
    obj2 = obj @ R.T
    by_object = dataclasses.replace(cam, obj_view=gl(view @ obj2), object=gl(obj2), inv_object=gl(np.linalg.inv(obj2)))
    # (b) the CAMERA carried along with the cloud: view' = view R^-1, so its position turns too
    view2 = view @ R.T
    by_camera = dataclasses.replace(cam, obj_view=gl(view2 @ obj), view=gl(view2), cam_pos=np.linalg.inv(view2)[:3, 3].astype(np.float32))
    with fresh() as eng:
        before = eng.render(cam).copy()
        eng.transform(rot, None)
        for label, c in (("(check a) under the inverse OBJECT matrix", by_object), ("(check b) from the camera turned along with the cloud", by_camera)):
            d = np.abs(eng.render(c).astype(np.float64) - before.astype(np.float64))
            print("%s against the untransformed frame: max |delta| per channel %s, mean %s"
                  % (label, np.array2string(d.max(axis=(0, 1)), precision=5), np.array2string(d.mean(axis=(0, 1)), precision=7)), flush=True)


if "--check" in sys.argv:
    check()
    sys.exit(0)

print("%s: %d splats, SH %s, %dx%d; median [min .. max] of %d calls, ms" % (name, n, "yes" if splats.has_sh else "no", W, H, reps), flush=True)
s = np.sqrt(0.1)
rect = (W * (0.5 - s / 2), H * (0.5 - s / 2), W * (0.5 + s / 2), H * (0.5 + s / 2))
part = np.zeros(n, bool)
part[n // 2:n // 2 + max(n // 100, 1)] = True
part_words = E.pack_mask(part)
dmask = C.c_void_p()
assert hip.hipMalloc(C.byref(dmask), C.c_size_t(words * 4)) == 0


def case(label, call):
    ms, wall, moved = [], [], 0
    for r in range(reps):
        with fresh() as eng:
            prep = call(eng, True)
            eng.synchronize()
            t0 = time.perf_counter()
            moved = call(eng, False, prep)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.get_transform()["ms"])
    ms = np.asarray(ms)
    print("%-34s mask copy %s   kernel .. sort %s   repack %s   wall %s   moved %d (%.3f of the cloud)"
          % (label, cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 2]), cell(wall), moved, moved / n), flush=True)


def whole(eng, prepare, prep=None):
    return None if prepare else eng.transform(x, None)


def boxed(eng, prepare, prep=None):
    if prepare:
        return eng.select_device(cs, E.select_region(rect), dmask.value)
    return eng.transform_device(x, dmask.value)


def one_percent(eng, prepare, prep=None):
    return None if prepare else eng.transform(x, part_words)


case("(1) whole cloud, NULL mask", whole)
case("(2) a select box, device mask", boxed)
case("(3) 1 %%, host mask (%.2f MB)" % (words * 4 / 1e6), one_percent)

# ---- the only way before: four arrays over the link, the host rule, a move with the attributes
names = ("P", "scale", "orient", "shx", "shy", "shz") if splats.has_sh else ("P", "scale", "orient")
read_ms, host_ms, move_ms = [], [], []
for r in range(max(3, reps // 4)):
    with fresh() as eng:
        eng.synchronize()
        t0 = time.perf_counter()
        back = eng.read(names=names)
        t1 = time.perf_counter()
        full = pkg.scenes.Splats(back.P, splats.Cd, splats.alpha, back.scale, back.orient, back.shx, back.shy, back.shz)
        out = E.transform_eval(x, full, None)
        t2 = time.perf_counter()
        eng.move(0, out.P, **{k: getattr(out, k) for k in names if k != "P"})
        t3 = time.perf_counter()
        read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3); move_ms.append((t3 - t2) * 1e3)
row = 12 + 6 + 8 + (96 if splats.has_sh else 0)
print("(before) gsr_read %s   transform_eval on the host %s   gsr_move with the attributes %s   (%.0f MB each way)"
      % (cell(read_ms), cell(host_ms), cell(move_ms), n * row / 1e6), flush=True)

check()
hip.hipFree(dmask)
