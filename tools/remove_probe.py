"""gsr_remove against the only way there was before it, in one session:
    python tools/remove_probe.py [C4] [--reps 20] [--n N] [--frames 60] [--windows 3]
The box keeps about 40 % of the cloud (the cube of tools/visibility_probe.py: 0.595 x the box of the positions, centred).  A removal is
not idempotent, so every repetition starts from the whole cloud: in a FRESH context (the first removal of a context also allocates
the spare planes: that is inside the call) and, second table, in ONE context that is uploaded the whole cloud again before every call
(the spare planes are there from the first, unmeasured round).  Medians [min .. max] of `reps` calls: the wall clock around the
synchronous verb, and beside it the verb's own stage clock (gsr_get_removal: mask copy, mark .. sort, repack).
 (1)  the 60 % the box hides: from a host mask, from a device mask, and with GSR_REMOVE_HIDDEN under gsr_set_visibility of the box
 (2)  a random 1 %
 (3)  beside each, the only way before: gsr_upload of the survivors' arrays into a context that holds the cloud (this same tree: that
      path is unchanged), with its stage clock (gsr_stats.upload_ms)
 (4)  frames per second of the orbit (device target): the full cloud; the 60 % hidden by gsr_set_visibility; after removing them; a
      fresh upload of the survivors -- the last two are the same bits, and must agree within the spread of the repeated windows"""
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
frames = int(opt("--frames", "60"))
windows = int(opt("--windows", "3"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
P = np.ascontiguousarray(splats.P, np.float32)
lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
centre, half = (lo + hi) / 2, (hi - lo) / 2 * 0.595
box = [E.crop_box(centre, half)]
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")


def device_copy(a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def timed(fn, eng):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


gone_box = ~E.visibility_eval(E.visibility_struct(box)[0], P)
gone_1 = np.random.default_rng(1).random(n) < 0.01
words_box, words_1 = E.pack_mask(gone_box), E.pack_mask(gone_1)
dev_box = device_copy(words_box)
print("%s: %d splats, SH %s; the box keeps %.3f; median [min .. max] of %d calls, ms" % (name, n, "yes" if splats.has_sh else "no", 1.0 - gone_box.mean(), reps), flush=True)


def verb(e, ptr, is_device, flags):
    """the C verb alone (Engine.remove also asks the context for its splat count, to check the mask's length)"""
    left = C.c_int64(0)
    E._check(e.L.gsr_remove(e.h, C.c_void_p(ptr), is_device, flags, C.byref(left)))
    return left.value


CASES = (("60 %, host mask", lambda e: verb(e, words_box.ctypes.data, 0, 0), False, gone_box),
         ("60 %, device mask", lambda e: verb(e, dev_box.value, 1, 0), False, gone_box),
         ("60 %, GSR_REMOVE_HIDDEN", lambda e: verb(e, None, 0, E.REMOVE_HIDDEN), True, gone_box),
         ("random 1 %, host mask", lambda e: verb(e, words_1.ctypes.data, 0, 0), False, gone_1))
shared = pkg.Engine(0)
for fresh in (True, False):
    print("---- %s" % ("a fresh context per call (the call allocates the spare planes)" if fresh else
                       "one context, uploaded the whole cloud again before every call"), flush=True)
    for label, call, vis, gone in CASES:
        wall, stage = [], []
        for r in range(reps + (0 if fresh else 1)):
            eng = pkg.Engine(0) if fresh else shared
            eng.set_visibility()
            eng.upload(splats)
            if vis:
                eng.set_visibility(volumes=box)
            t, left = timed(lambda: call(eng), eng)
            assert left == int((~gone).sum()), (label, left)
            if fresh or r:
                wall.append(t); stage.append(eng.get_removal()["ms"])
            if fresh:
                eng.close()
        st = np.asarray(stage)
        print("%-26s wall %s   mask copy %s   mark..sort %s   repack %s   (%d left, %.2f MB of mask)"
              % (label, cell(wall), cell(st[:, 0]), cell(st[:, 1]), cell(st[:, 2]), int((~gone).sum()), words_box.nbytes / 1e6), flush=True)
shared.set_visibility()

# ---- (3) the only way before: the survivors' arrays uploaded again
for label, gone in (("60 %", gone_box), ("random 1 %", gone_1)):
    left = splats.subset(~gone)
    wall, stage = [], []
    for r in range(reps + 1):
        shared.upload(splats)
        t, _ = timed(lambda: shared.upload(left), shared)
        if r:
            wall.append(t); stage.append(shared.stats()["upload_ms"][:4])
    st = np.asarray(stage)
    print("gsr_upload of the survivors of %-10s wall %s   link %s   order %s   pack %s   (%d splats, %.0f MB over the link)"
          % (label + ":", cell(wall), cell(st[:, 0]), cell(st[:, 1]), cell(st[:, 2]), left.n, left.n * (132 if splats.has_sh else 36) / 1e6), flush=True)

# ---- (4) frames per second
target = C.c_void_p()
assert hip.hipMalloc(C.byref(target), C.c_size_t(cfg["width"] * cfg["height"] * 16)) == 0
cams = [E.camera_struct(pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], f)) for f in range(frames + 10)]


def fps(who):
    out = []
    for w in range(windows):
        for c in cams[:10]:
            who.render_struct_to_device(c, target.value)
        who.synchronize()
        t0 = time.perf_counter()
        for c in cams[10:]:
            who.render_struct_to_device(c, target.value)
        who.synchronize()
        out.append(frames / (time.perf_counter() - t0))
    return out


shared.upload(splats)
rates = {"the full cloud": fps(shared)}
shared.set_visibility(volumes=box)
rates["60 % hidden (gsr_set_visibility)"] = fps(shared)
shared.set_visibility()
assert shared.remove(words_box) == int((~gone_box).sum())
rates["60 % removed (gsr_remove)"] = fps(shared)
other = pkg.Engine(0)
other.upload(splats.subset(~gone_box))
rates["the survivors uploaded"] = fps(other)
for label, v in rates.items():
    print("(4) %-34s %s frames per second over %d windows of %d orbit frames" % (label, cell(v), windows, frames), flush=True)
a, b = rates["60 % removed (gsr_remove)"], rates["the survivors uploaded"]
spread = max(max(a) - min(a), max(b) - min(b))
print("(4) removed vs uploaded: medians differ by %.1f fps; the larger run-to-run spread of the two is %.1f fps: %s"
      % (abs(np.median(a) - np.median(b)), spread, "agree" if abs(np.median(a) - np.median(b)) <= spread else "DO NOT AGREE"), flush=True)
hip.hipFree(target); hip.hipFree(dev_box)
other.close()
shared.close()
