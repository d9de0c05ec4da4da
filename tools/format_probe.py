"""Device-target frames in one target format: python tools/format_probe.py C4 --format 0|1|2 [--size WxH]
Prints the frame rate; run under `rocprofv3 --kernel-trace --stats -- python tools/format_probe.py ...` (a run of its own) for k_blend's duration per format."""
import sys, time
sys.path.insert(0, '.')
import ctypes as C
import __graft_entry__ as ge
pkg = ge.load_package()
name = sys.argv[1]
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
fmt = int(opt("--format", "0"))
splats, cfg = pkg.scenes.make_config(name)
W, H, order = cfg["width"], cfg["height"], cfg["sh_order"]
if "--size" in sys.argv: W, H = (int(x) for x in opt("--size", "").split("x"))
eng = pkg.Engine(0); eng.upload(splats)
eng.set_target_format(fmt)
bpp = 16 >> fmt
hip = C.CDLL("libamdhip64.so")
p = C.c_void_p(); assert hip.hipMalloc(C.byref(p), C.c_size_t(W * H * bpp)) == 0
cs = [pkg.engine.camera_struct(pkg.scenes.config_camera(name, pkg.camera, W, H, order, i)) for i in range(70)]
for c in cs[:10]: eng.render_struct_to_device(c, p.value)
eng.synchronize(); t0 = time.perf_counter()
for c in cs[10:]: eng.render_struct_to_device(c, p.value)
eng.synchronize(); dt = (time.perf_counter() - t0) / 60
print("%s %dx%d device target, %d B/px: %.4f ms per frame = %4.0f fps" % (name, W, H, bpp, dt * 1e3, 1 / dt), flush=True)
eng.close(); hip.hipFree(p)
