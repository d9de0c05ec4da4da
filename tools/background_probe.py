"""Device-target frames with and without a background, in one process: python tools/background_probe.py C4 [--size WxH] [--rounds N] [--depth]
Per target format (RGBA32F, RGBA16F, RGBA8) alternates legs of 60 moving-camera frames -- no background, a colour, a DEVICE image in
each of the three image formats -- and prints, per leg, the frame time and the blend kernel's duration (HIP events around it: k_blend
without a background, k_blend_over with one), each beside the no-background frame of the same run.  --depth: every frame is
depth-tested against a cleared depth buffer, the frame the viewport hook issues."""
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
held = []
def dev(nbytes, src=None):
    p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    if src is not None: assert hip.hipMemcpy(p, C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes), 1) == 0
    held.append(p.value)
    return p.value
img = dev(W * H * 16)
depth = dev(W * H * 4, np.ones(W * H, np.float32)) if "--depth" in sys.argv else 0
rng = np.random.default_rng(3)
alpha = rng.choice(np.array([0.0, 0.4, 1.0], np.float32), (H, W, 1))
f32 = np.concatenate([rng.random((H, W, 3)).astype(np.float32) * alpha, alpha], -1).astype(np.float32)
def image_bg(a):
    b, _ = E.background_struct(a)
    b.image, b.image_is_device = dev(a.nbytes, a), 1
    return b
LEGS = [("none", None), ("colour", E.background_struct((0.1, 0.2, 0.3, 0.5))[0]), ("image f32", image_bg(f32)),
        ("image f16", image_bg(f32.astype(np.float16))), ("image u8", image_bg(np.rint(f32 * 255).astype(np.uint8)))]
cs = [E.camera_struct(pkg.scenes.config_camera(name, pkg.camera, W, H, order, i)) for i in range(70)]
med = lambda v: float(np.median(v))
for fmt, fname in ((E.TARGET_RGBA32F, "RGBA32F"), (E.TARGET_RGBA16F, "RGBA16F"), (E.TARGET_RGBA8, "RGBA8")):
    eng.set_target_format(fmt)
    acc = {k: [] for k in range(len(LEGS))}
    for r in range(rounds):
        for leg, (lname, bg) in enumerate(LEGS):
            for c in cs[:10]: eng.render_over_struct_to_device(c, bg, img, depth)
            eng.synchronize(); eng.stats_reset(); t0 = time.perf_counter()
            for c in cs[10:]: eng.render_over_struct_to_device(c, bg, img, depth)
            eng.synchronize(); dt = (time.perf_counter() - t0) / 60
            st = eng.stats()
            acc[leg].append((dt * 1e3, st["blend_ms_total"] / max(st["blend_launches"], 1)))
            print("%s round %d %-10s %.4f ms per frame = %5.0f fps, blend kernel %.4f ms" % (fname, r, lname, dt * 1e3, 1 / dt, acc[leg][-1][1]), flush=True)
    base_f, base_b = med([a[0] for a in acc[0]]), med([a[1] for a in acc[0]])
    for leg, (lname, bg) in enumerate(LEGS):
        f, b = med([a[0] for a in acc[leg]]), med([a[1] for a in acc[leg]])
        print("%s %dx%d%s %s %-10s median %.4f ms per frame = %5.0f fps (%.3f x none), blend kernel %.4f ms (%+.1f us)"
              % (name, W, H, " depth-tested" if depth else "", fname, lname, f, 1e3 / f, f / base_f, b, (b - base_b) * 1e3), flush=True)
eng.close()
for p in held: hip.hipFree(C.c_void_p(p))
