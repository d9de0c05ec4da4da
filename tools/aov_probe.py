"""Device-target frames with and without the depth AOV, in one process: python tools/aov_probe.py C4 [--size WxH] [--rounds N] [--depth]
Alternates legs of 60 moving-camera frames (the plain frame, the AOV frame, the AOV frame + gsr_resolve_depth_device) and prints, per leg,
the frame time and the blend kernel's duration (HIP events around it: k_blend without the AOV, k_blend_aov with it).  --depth: every
frame is depth-tested against a cleared depth buffer, the frame the viewport hook issues."""
import sys, time
sys.path.insert(0, '.')
import ctypes as C
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1]
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
rounds = int(opt("--rounds", "3"))
splats, cfg = pkg.scenes.make_config(name)
W, H, order = cfg["width"], cfg["height"], cfg["sh_order"]
if "--size" in sys.argv: W, H = (int(x) for x in opt("--size", "").split("x"))
eng = pkg.Engine(0); eng.upload(splats)
eng.set_option(E.OPT_STAGE_TIMING, 1)
hip = C.CDLL("libamdhip64.so")
def dev(nbytes):
    p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    return p.value
img, plane, zbuf, depth = dev(W * H * 16), dev(W * H * 8), dev(W * H * 4), 0
if "--depth" in sys.argv:
    ones = np.ones(W * H, np.float32)
    depth = dev(W * H * 4)
    assert hip.hipMemcpy(C.c_void_p(depth), C.c_void_p(ones.ctypes.data), C.c_size_t(ones.nbytes), 1) == 0
cs = [E.camera_struct(pkg.scenes.config_camera(name, pkg.camera, W, H, order, i)) for i in range(70)]
def frame(c, leg):
    eng.render_aov_struct_to_device(c, img, plane if leg else 0, depth)
    if leg == 2: eng.resolve_depth_device(plane, W * H, 0.5, zbuf)
LEGS = ("plain", "aov", "aov + resolve")
acc = {k: [] for k in range(3)}
for r in range(rounds):
    for leg in range(3):
        for c in cs[:10]: frame(c, leg)
        eng.synchronize(); eng.stats_reset(); t0 = time.perf_counter()
        for c in cs[10:]: frame(c, leg)
        eng.synchronize(); dt = (time.perf_counter() - t0) / 60
        st = eng.stats()
        acc[leg].append((dt * 1e3, st["blend_ms_total"] / max(st["blend_launches"], 1)))
        print("round %d %-14s %.4f ms per frame = %5.0f fps, blend kernel %.4f ms" % (r, LEGS[leg], dt * 1e3, 1 / dt, acc[leg][-1][1]), flush=True)
med = lambda v: float(np.median(v))
base = med([a[0] for a in acc[0]])
for leg in range(3):
    f, b = med([a[0] for a in acc[leg]]), med([a[1] for a in acc[leg]])
    print("%s %dx%d%s %-14s median %.4f ms per frame (%.3f x plain), blend kernel %.4f ms" % (name, W, H, " depth-tested" if depth else "", LEGS[leg], f, f / base, b), flush=True)
eng.close()
for p in (img, plane, zbuf, depth):
    if p: hip.hipFree(C.c_void_p(p))
