"""gsr_add against the only way there was before it, in one session:
    python tools/add_probe.py [C4] [--reps 20] [--n N] [--frames 60] [--windows 3] [--fractions 0.01,0.05,1.0]
The new rows are the first m splats of the cloud itself, mirrored through the centre of its box (so the box stays, and they fall among
the resident ones).  An add is not idempotent, so every repetition starts from the cloud alone:
 (1)  WITH growth: a FRESH context per call, uploaded the cloud (capacity n), then the add -- the call allocates the planes, the frame
      slots' arrays and everything else at the new capacity, and frees the old ones
 (2)  WITHOUT growth: ONE context that holds the larger capacity from a first, unmeasured round and is uploaded the cloud again before
      every call (gsr_upload keeps the capacity)
each for the host form (gsr_add) and the device form (gsr_add_device from float32 arrays in device memory).  Medians [min .. max] of
`reps` calls: the wall clock around the synchronous verb, and beside it the verb's own stage clock (gsr_get_add: link, positions ..
sort, pack).
 (3)  beside them, the only way before: gsr_upload of the concatenated arrays into a context that holds the cloud, with its stage clock
 (4)  frames per second of the orbit (device target): the cloud; after an add of the middle fraction; a fresh upload of the same
      concatenation -- the last two are the same bits, and must agree within the spread of the repeated windows"""
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
fractions = [float(x) for x in opt("--fractions", "0.01,0.05,1.0").split(",")]
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
sh = splats.has_sh
P = np.ascontiguousarray(splats.P, np.float32)
mirror = (P.min(axis=0) + P.max(axis=0)).astype(np.float32)
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")
row_bytes = 132 if sh else 36


def device_copy(a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 4))) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def timed(fn, eng):
    eng.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def new_rows(m):
    """the first m splats, mirrored through the centre of the box"""
    B = splats.subset(slice(0, m))
    B.P = np.ascontiguousarray(mirror - B.P, np.float32)
    return B


def floats(B):
    """the rows as a trainer holds them: float32 arrays (the halves widened: the timing does not depend on the values)"""
    w = lambda h: np.ascontiguousarray(h.view(np.float16).astype(np.float32))
    f = {"P": B.P, "Cd": w(B.Cd), "alpha": np.ascontiguousarray(B.alpha, np.float32), "scale": w(B.scale), "orient": w(B.orient)}
    if sh:
        f["sh"] = np.ascontiguousarray(np.stack([w(B.shx)[:, :15], w(B.shy)[:, :15], w(B.shz)[:, :15]], axis=2))       # (m, 15, 3)
    return f


def host_verb(e, arr):
    total = C.c_int64(0)
    E._check(e.L.gsr_add(e.h, arr.n, *arr.ptrs(), C.byref(total)))
    return total.value


def device_verb(e, a, m):
    total = C.c_int64(0)
    E._check(e.L.gsr_add_device(e.h, m, C.byref(a), C.byref(total)))
    return total.value


print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, "yes" if sh else "no", reps), flush=True)
shared = pkg.Engine(0)
for frac in fractions:
    m = max(1, int(round(n * frac)))
    B = new_rows(m)
    arr = E.add_arrays(B)
    dev = {k: device_copy(v) for k, v in floats(B).items()}
    dstruct, _, _ = E.device_attrs_struct(m, 15 if sh else None, **{k: v.value for k, v in dev.items()})
    forms = (("host form", lambda e: host_verb(e, arr)), ("device form", lambda e: device_verb(e, dstruct, m)))
    print("---- %.0f %%: %d new rows, %.1f MB over the link in the host form" % (frac * 100, m, m * row_bytes / 1e6), flush=True)
    for grow in (True, False):
        for label, call in forms:
            wall, stage = [], []
            for r in range(reps + (0 if grow else 1)):
                eng = pkg.Engine(0) if grow else shared
                eng.upload(splats)
                t, total = timed(lambda: call(eng), eng)
                assert total == n + m, (label, total)
                ad = eng.get_add()
                if grow or r:
                    assert ad["grows"] == (1 if grow else shared_grows), (label, ad)
                    wall.append(t); stage.append(ad["ms"])
                else:
                    shared_grows = ad["grows"]
                if grow:
                    eng.close()
            st = np.asarray(stage)
            print("%-12s %-15s wall %s   link %s   positions..sort %s   pack %s"
                  % (label, "with growth" if grow else "without growth", cell(wall), cell(st[:, 0]), cell(st[:, 1]), cell(st[:, 2])), flush=True)
    # ---- (3) the only way before: the concatenated arrays uploaded again
    S = splats.concat(B)
    wall, stage = [], []
    for r in range(reps + 1):
        shared.upload(splats)
        t, _ = timed(lambda: shared.upload(S), shared)
        if r:
            wall.append(t); stage.append(shared.stats()["upload_ms"][:4])
    st = np.asarray(stage)
    print("gsr_upload of the concatenation:  wall %s   link %s   order %s   pack %s   (%d splats, %.0f MB over the link)"
          % (cell(wall), cell(st[:, 0]), cell(st[:, 1]), cell(st[:, 2]), S.n, S.n * row_bytes / 1e6), flush=True)
    for p in dev.values():
        hip.hipFree(p)
    del S

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


frac = fractions[len(fractions) // 2]
B = new_rows(max(1, int(round(n * frac))))
shared.upload(splats)
rates = {"the cloud": fps(shared)}
assert shared.add(B) == n + B.n
rates["after gsr_add of %.0f %%" % (frac * 100)] = fps(shared)
other = pkg.Engine(0)
other.upload(splats.concat(B))
rates["the concatenation uploaded"] = fps(other)
for label, v in rates.items():
    print("(4) %-34s %s frames per second over %d windows of %d orbit frames" % (label, cell(v), windows, frames), flush=True)
a, b = rates["after gsr_add of %.0f %%" % (frac * 100)], rates["the concatenation uploaded"]
spread = max(max(a) - min(a), max(b) - min(b))
print("(4) added vs uploaded: medians differ by %.1f fps; the larger run-to-run spread of the two is %.1f fps: %s"
      % (abs(np.median(a) - np.median(b)), spread, "agree" if abs(np.median(a) - np.median(b)) <= spread else "DO NOT AGREE"), flush=True)
hip.hipFree(target)
other.close()
shared.close()
