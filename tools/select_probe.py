"""gsr_select beside the only way there was before it, in one session:
    python tools/select_probe.py [C4] [--reps 20] [--n N]
    rocprofv3 --kernel-trace --stats -- python tools/select_probe.py [C4] --kernels      # a run of its own: k_select beside k_alpha_capture
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), from the verb's own clock (gsr_get_select: kernel,
copies, wall), on the config's first orbit camera, of
 (1)  a rect over about a tenth of the frame into a DEVICE mask (REPLACE), and the same as TOGGLE (the read-modify-write of an op)
 (2)  the same rect with a depth test against the resolved depth AOV (gsr_render_aov + gsr_resolve_depth_device, bias 1e-4): device mask
 (2') the same rect with a painted image (a disc inscribed in the rect) and the depth test: device mask
 (3)  (1) and (2) into a HOST mask
 (4)  the only way before: gsr_read of P and alpha, plus the projection of every point in numpy float32
The device mask of (1), (2) and (2') is compared with gsr_select_eval over the whole cloud (the rule on the host).
--kernels: no clocks; `reps` rounds of [a visibility set from nothing, cleared again, one select of each kind], so that a kernel trace holds
k_alpha_capture over the whole cloud -- the same gather of geoA through the inverse of the storage order: this kernel's yardstick --
next to k_select."""
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


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


def clocks(eng, call):
    out = []
    for r in range(reps + 1):
        call()
        if r:
            out.append(eng.get_select()["ms"])
    return np.asarray(out)


cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
cs = E.camera_struct(cam)
s = np.sqrt(0.1)
rect = (W * (0.5 - s / 2), H * (0.5 - s / 2), W * (0.5 + s / 2), H * (0.5 + s / 2))
yy, xx = np.mgrid[0:H, 0:W]
disc = ((xx + 0.5 - W / 2) / (W * s / 2)) ** 2 + ((yy + 0.5 - H / 2) / (H * s / 2)) ** 2 <= 1.0
print("%s: %d splats, %dx%d; rect %.1f x %.1f px (%.3f of the frame); median [min .. max] of %d calls, ms"
      % (name, n, W, H, rect[2] - rect[0], rect[3] - rect[1], (rect[2] - rect[0]) * (rect[3] - rect[1]) / (W * H), reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    target, plane, depth, dmask, dimage = (device_room(b) for b in (W * H * 16, W * H * 8, W * H * 4, words * 4, (W * H + 31) // 32 * 4))
    img_words = E.pack_image(disc)
    assert hip.hipMemcpy(dimage, C.c_void_p(img_words.ctypes.data), C.c_size_t(img_words.nbytes), 1) == 0
    eng.render_aov_struct_to_device(cs, target.value, plane.value)
    eng.resolve_depth_device(plane.value, W * H, 0.5, depth.value)
    eng.synchronize()
    host_depth = np.empty((H, W), np.float32)
    assert hip.hipMemcpy(C.c_void_p(host_depth.ctypes.data), depth, C.c_size_t(host_depth.nbytes), 2) == 0
    bias = 1.0e-4
    kinds = {"rect": {}, "rect + depth": {"depth_device": depth.value, "depth_bias": bias},
             "rect + image + depth": {"image_device": dimage.value, "depth_device": depth.value, "depth_bias": bias}}
    host_kinds = {"rect": {}, "rect + depth": {"depth": host_depth, "depth_bias": bias}, "rect + image + depth": {"image": disc, "depth": host_depth, "depth_bias": bias}}

    if kernels_only:
        for r in range(reps):
            eng.set_visibility(mask=np.zeros(n, bool))     # from nothing: k_alpha_capture over the whole cloud
            eng.set_visibility()
            for kw in kinds.values():
                eng.select_device(cs, E.select_region(rect, **kw), dmask.value)
        print("rounds:", reps)
        sys.exit(0)

    def check(label, kw):
        got = np.empty(words, np.uint32)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dmask, C.c_size_t(got.nbytes), 2) == 0
        want = E.select_eval(cs, (0, 0, 0), E.select_region(rect, **kw), splats.P, splats.alpha)
        assert np.array_equal(got, E.pack_mask(want)), label + ": the device mask is not the host rule's"
        return int(want.sum())

    for label, kw in kinds.items():
        ms = clocks(eng, lambda: eng.select_device(cs, E.select_region(rect, **kw), dmask.value))
        hits = check(label, host_kinds[label])
        print("(device mask) %-22s kernel %s   copies %s   wall %s   hits %d (%.3f of the cloud)"
              % (label, cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 3]), hits, hits / n), flush=True)
    ms = clocks(eng, lambda: eng.select_device(cs, E.select_region(rect, op=E.SELECT_TOGGLE), dmask.value))
    print("(device mask) %-22s kernel %s   copies %s   wall %s" % ("rect, TOGGLE", cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 3])), flush=True)
    host_words = np.zeros(words, np.uint32)
    hit, nset = C.c_int64(0), C.c_int64(0)
    for label in ("rect", "rect + depth"):
        r, keep = E.select_region(rect, **kinds[label])
        ms = clocks(eng, lambda: E._check(eng.L.gsr_select(eng.h, C.byref(cs), C.byref(r), host_words.ctypes.data, 0, C.byref(hit), C.byref(nset))))
        print("(host mask)   %-22s kernel %s   copies %s   wall %s   (%.2f MB over the link)"
              % (label, cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 3]), words * 4 / 1e6), flush=True)

    # ---- the only way before: P and alpha over the link, the vertex stage restated in numpy
    ov = np.asarray(cam.obj_view, np.float32).reshape(4, 4).T
    pr = np.asarray(cam.proj, np.float32).reshape(4, 4).T
    read_ms, host_ms, before_hits = [], [], 0
    for r in range(max(3, reps // 4) + 1):
        t0 = time.perf_counter()
        back = eng.read(names=("P", "alpha"))
        t1 = time.perf_counter()
        tv = back.P @ ov[:3, :3].T + ov[:3, 3]
        tv[:, 1] = -tv[:, 1]
        cl = tv @ pr[:, :3].T + pr[:, 3]
        w = cl[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            cx = ((cl[:, 0] / w) * np.float32(0.5) + np.float32(0.5)) * np.float32(W)
            cy = ((-cl[:, 1] / w) * np.float32(0.5) + np.float32(0.5)) * np.float32(H)
            sel = (w > 0) & (cl[:, 2] >= -w) & (cl[:, 2] <= w) & (back.alpha >= np.float32(1.0 / 255.0)) & \
                  (cx >= np.float32(rect[0])) & (cx < np.float32(rect[2])) & (cy >= np.float32(rect[1])) & (cy < np.float32(rect[3]))
        mask = E.pack_mask(sel)
        t2 = time.perf_counter()
        if r:
            read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3)
        before_hits = int(sel.sum())
    print("(before)      gsr_read of P and alpha %s   numpy projection + rect + packing %s   (%.0f MB over the link; %d hits: numpy does not fuse, so "
          "a centre on an edge may fall on the other side)" % (cell(read_ms), cell(host_ms), n * 16 / 1e6, before_hits), flush=True)
    for p in (target, plane, depth, dmask, dimage):
        hip.hipFree(p)
