"""gsr_multi's three shard layouts on the GPUs of this node: python tools/multi_layout_probe.py [T1] [--gpus 4] [--layouts 1,0,2] [--steps 200] [--warmup 40]
One line per layout: frames per second over `steps` device-target frames along the config's orbit (no synchronisation in between: the
gather of a frame overlaps the next one), whether the last frame is the 1-GPU frame bit for bit, and for the band layouts the boundaries
and how often layout 2 moved them.  With fewer GPUs than asked for the ranks share GPU 0 over the COPY transport (the figure is then the
sum of the bands, not a multi-GPU frame rate).  tools/first_multi_gpu_node.sh runs it; tools/band_balance_probe.py is the one-GPU view."""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "T1"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
gpus, steps, warmup = int(opt("--gpus", "4")), int(opt("--steps", "200")), int(opt("--warmup", "40"))
layouts = [int(x) for x in opt("--layouts", "1,0,2").split(",")]
splats, cfg = pkg.scenes.make_config(name)
W, H, order = cfg["width"], cfg["height"], cfg["sh_order"]
cams = [pkg.scenes.config_camera(name, pkg.camera, W, H, order, i) for i in range(warmup + steps)]
structs = [E.camera_struct(c) for c in cams]
real = torch.cuda.device_count() >= gpus
devices = list(range(gpus)) if real else [0] * gpus
target = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
with pkg.Engine(0) as ref:
    ref.upload(splats)
    want = ref.render(cams[-1])
print(f"{name}: {splats.n} splats {W}x{H}, {gpus} ranks on {'distinct GPUs' if real else 'GPU 0 (COPY transport: bands in turn)'}", flush=True)
for layout in layouts:
    with pkg.MultiEngine(devices, E.TRANSPORT_AUTO if real else E.TRANSPORT_COPY) as M:
        M.set_option(E.OPT_SHARD_LAYOUT, layout)
        M.set_option(E.OPT_STAGE_TIMING, 0)
        M.upload(splats)
        for c in structs[:warmup]:
            M.render_struct_to_device(c, target.data_ptr())
        M.synchronize()
        t0 = time.perf_counter()
        for c in structs[warmup:]:
            M.render_struct_to_device(c, target.data_ptr())
        M.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        same = np.array_equal(target.cpu().numpy(), want)
        bands = "" if layout == 0 else "  boundaries %s  rebalances %d" % (M.get_bands()[0].tolist(), M.get_bands()[1])
        print(f"layout {layout}: {1e3 / ms:8.1f} fps  {ms:.4f} ms per frame  transport {M.transport}  bit-identical {same}{bands}", flush=True)
