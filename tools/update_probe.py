"""gsr_update against a full re-upload, in one session: python tools/update_probe.py [C4] [--reps 5] [--n N]
For each attribute subset, the whole cloud is edited in place `reps` times; then the same (edited) arrays are uploaded afresh `reps` times.
Then one splat's scale is edited.  Prints, per case: bytes moved host -> device, the median wall time of the call, and gsr_stats.upload_ms[4] / [5] (host -> device wall
clock / kernels by HIP events) -- for the upload, upload_ms[0] / [1] + [2] (copies / ordering + packing)."""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
reps = int(opt("--reps", "5"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
BYTES = {"Cd": 6, "alpha": 4, "scale": 6, "orient": 8, "shx": 32, "shy": 32, "shz": 32}
CASES = (("alpha", ("alpha",)), ("Cd", ("Cd",)), ("Cd+alpha", ("Cd", "alpha")), ("scale+orient", ("scale", "orient")),
         ("everything", tuple(BYTES)))
rng = np.random.default_rng(5)
# the edited arrays: a permutation of the cloud's own rows (same distributions; P stays)
shuffle = rng.permutation(n)
new = {k: np.ascontiguousarray(getattr(splats, k)[shuffle]) for k in BYTES if getattr(splats, k, None) is not None}
med = lambda v: float(np.median(v))
eng = pkg.Engine(0)
eng.upload(splats)
cam = pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], 0)
eng.render(cam)
print("%s: %d splats, SH %s; medians of %d calls" % (name, n, "yes" if splats.has_sh else "no", reps), flush=True)
print("%-14s %10s %10s %10s %10s" % ("case", "MB h->d", "wall ms", "h->d ms", "kernel ms"), flush=True)
for label, names in CASES:
    names = tuple(k for k in names if k in new)
    wall, h2d, kern = [], [], []
    for r in range(reps + 1):
        arrays = {k: (new[k] if r % 2 == 0 else np.ascontiguousarray(getattr(splats, k))) for k in names}
        eng.synchronize(); t0 = time.perf_counter()
        eng.update_attrs(0, **arrays)
        dt = (time.perf_counter() - t0) * 1e3
        um = eng.stats()["upload_ms"]
        if r:                                           # (the first call of a case grows the arena / builds the inverse permutation)
            wall.append(dt); h2d.append(um[4]); kern.append(um[5])
    print("%-14s %10.1f %10.3f %10.3f %10.3f" % (label, n * sum(BYTES[k] for k in names) / 1e6, med(wall), med(h2d), med(kern)), flush=True)
    eng.render(cam)
# ... and the smallest edit: one splat's scale (k_cluster_extents still runs over every cluster: 32 bytes read per resident splat)
wall, h2d, kern = [], [], []
for r in range(reps + 1):
    row = np.ascontiguousarray((new["scale"] if r % 2 == 0 else splats.scale)[n // 2:n // 2 + 1])
    eng.synchronize(); t0 = time.perf_counter()
    eng.update_attrs(n // 2, scale=row)
    dt = (time.perf_counter() - t0) * 1e3
    um = eng.stats()["upload_ms"]
    if r:
        wall.append(dt); h2d.append(um[4]); kern.append(um[5])
print("%-14s %10.6f %10.3f %10.3f %10.3f" % ("scale, 1 splat", 6 / 1e6, med(wall), med(h2d), med(kern)), flush=True)
wall, h2d, kern = [], [], []
for r in range(reps + 1):
    eng.synchronize(); t0 = time.perf_counter()
    eng.upload(splats)
    dt = (time.perf_counter() - t0) * 1e3
    um = eng.stats()["upload_ms"]
    if r:
        wall.append(dt); h2d.append(um[0]); kern.append(um[1] + um[2])
print("%-14s %10.1f %10.3f %10.3f %10.3f" % ("full upload", n * (12 + sum(BYTES[k] for k in new)) / 1e6, med(wall), med(h2d), med(kern)), flush=True)
eng.close()
