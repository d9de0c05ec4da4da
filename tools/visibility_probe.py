"""gsr_set_visibility against the only way there was before it, in one session:
    python tools/visibility_probe.py [C4] [--reps 20] [--n N] [--frames 60]
    (cd _tree && python ../tools/visibility_probe.py [C4] --parent)      # the tree of tools/build_tree.sh: case (c) alone
The box keeps about 40 % of the cloud (a cube of 0.595 x the box of the positions, centred).  Medians [min .. max] of `reps` calls, wall
clock around the synchronous verb, after one unmeasured round (which allocates):
 (a)  whole-cloud crop: nothing hidden -> the box (the true alphas are put aside, the rule runs, 60 % of the opacities are rewritten);
      (a') the box -> the box half its size further along x, both ways in turn (no capture: the rule and the stores of what changes);
      and clearing (everything visible again).
 (b)  a dragged handle: every step moves the box centre by 1 % of its size; few bits change.
 (c)  the only way before: a numpy float32 evaluation of the same box on the host, then gsr_update(alpha) of the whole cloud; the host
      pass and the verb are reported separately (with the verb's link and kernel times from gsr_stats.upload_ms[4], [5]).
 (e)  for information: frames per second on the orbit with 60 % of the cloud hidden, against none hidden (device target), and of a
      second context that was UPLOADED the effective alphas: the same frames by contract, so the same rate.
A library without the verb (--parent) runs (c) alone."""
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
n_over = opt("--n", None)
parent = "--parent" in sys.argv or not hasattr(E, "visibility_struct")
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
P = np.ascontiguousarray(splats.P, np.float32)
lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
centre, half = (lo + hi) / 2, (hi - lo) / 2 * 0.595
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))


def timed(fn, eng):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_box(c):
    """the box on the host as a caller would write it: float32 numpy over every position"""
    q = (P - c.astype(np.float32)) * (1.0 / half).astype(np.float32)
    return (np.abs(q) <= 1.0).all(axis=1)


eng = pkg.Engine(0)
eng.upload(splats)
cam0 = pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], 0)
eng.render(cam0)
print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, "yes" if splats.has_sh else "no", reps), flush=True)

# ---- (c) the only way before
host_ms, verb_ms, link_ms, kern_ms = [], [], [], []
for r in range(reps + 1):
    c = centre + np.array([(r % 2) * half[0], 0.0, 0.0])
    t0 = time.perf_counter()
    inside = host_box(c)
    eff = np.where(inside, splats.alpha, np.float32(0.0)).astype(np.float32)
    th = (time.perf_counter() - t0) * 1e3
    tv = timed(lambda: eng.update_attrs(0, alpha=eff), eng)
    st = eng.stats()
    if r:
        host_ms.append(th); verb_ms.append(tv); link_ms.append(st["upload_ms"][4]); kern_ms.append(st["upload_ms"][5])
print("(c) host evaluation + gsr_update(alpha), %s tree: host pass %s   verb %s   (its link %s, its kernels %s); %.1f MB over the link"
      % ("PARENT" if parent else "this", cell(host_ms), cell(verb_ms), cell(link_ms), cell(kern_ms), n * 4 / 1e6), flush=True)
eng.update_attrs(0, alpha=splats.alpha)
if parent:
    eng.close()
    sys.exit(0)

# ---- (a) whole-cloud crop
box = lambda c: [E.crop_box(c, half)]
kept = E.visibility_eval(E.visibility_struct(box(centre))[0], P).mean()
set_ms, swap_ms, clear_ms = [], [], []
for r in range(reps + 1):
    ts = timed(lambda: eng.set_visibility(volumes=box(centre)), eng)
    hidden = eng.get_visibility()[1]
    tw = timed(lambda: eng.set_visibility(volumes=box(centre + np.array([half[0], 0.0, 0.0]))), eng)
    tw2 = timed(lambda: eng.set_visibility(volumes=box(centre)), eng)
    tc = timed(lambda: eng.set_visibility(), eng)
    if r:
        set_ms.append(ts); swap_ms += [tw, tw2]; clear_ms.append(tc)
print("(a) nothing hidden -> box (keeps %.3f, hides %d): %s   (a') box <-> box half a size along x: %s   clear: %s"
      % (kept, hidden, cell(set_ms), cell(swap_ms), cell(clear_ms)), flush=True)
print("    floor of the rule's pass, not measured: 16 + 4 + 4 bytes read per splat = %.0f MB" % (n * 24 / 1e6), flush=True)

# ---- (b) a dragged handle
eng.set_visibility(volumes=box(centre))
drag_ms, drag_changed = [], []
prev = E.visibility_eval(E.visibility_struct(box(centre))[0], P)
for r in range(1, reps + 2):
    c = centre + np.array([0.02 * half[0] * r, 0.0, 0.0])
    td = timed(lambda: eng.set_visibility(volumes=box(c)), eng)
    now = E.visibility_eval(E.visibility_struct(box(c))[0], P)           # (not timed)
    if r > 1:
        drag_ms.append(td); drag_changed.append(int((now != prev).sum()))
    prev = now
print("(b) dragged handle, 1 %% of the box size per step: %s   splats that change sides per step: %d .. %d"
      % (cell(drag_ms), min(drag_changed), max(drag_changed)), flush=True)

# ---- (e) frames per second, for information
hip = C.CDLL("libamdhip64.so")
target = C.c_void_p()
assert hip.hipMalloc(C.byref(target), C.c_size_t(cfg["width"] * cfg["height"] * 16)) == 0
cams = [E.camera_struct(pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], f)) for f in range(frames + 10)]
fresh = pkg.Engine(0)
eff = np.where(E.visibility_eval(E.visibility_struct(box(centre))[0], P), splats.alpha, np.float32(0.0)).astype(np.float32)
fresh.upload(pkg.scenes.Splats(splats.P, splats.Cd, eff, splats.scale, splats.orient, splats.shx, splats.shy, splats.shz))
for label, who, vols in (("none hidden", eng, None), ("60 % hidden", eng, box(centre)), ("uploaded that way", fresh, None), ("none hidden again", eng, None)):
    if who is eng:
        eng.set_visibility(volumes=vols) if vols else eng.set_visibility()
    for c in cams[:10]:
        who.render_struct_to_device(c, target.value)
    who.synchronize()
    t0 = time.perf_counter()
    for c in cams[10:]:
        who.render_struct_to_device(c, target.value)
    who.synchronize()
    print("(e) %-18s %.1f frames per second over %d orbit frames" % (label, frames / (time.perf_counter() - t0), frames), flush=True)
hip.hipFree(target)
fresh.close()
eng.close()
