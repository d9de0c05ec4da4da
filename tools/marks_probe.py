"""gsr_render_marks beside its yardsticks, in one session:
    python tools/marks_probe.py [C4] [--reps 20] [--n N]
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), on the config's first orbit camera, a device mask and
a device target throughout, from the verb's own clock (gsr_get_marks: clear + k_mark, k_mark_resolve, copies, wall):
 (1)  dots (radius 1, a fixed colour) of a random 1 %, 10 % and 100 % of the cloud
 (2)  outlines (Cd) of the same three selections -- the sparse ones are where one thread per upload index loses: a wave keeps all its
      lanes while a few of them walk long edges
and, for comparison,
 (3)  gsr_select with the whole frame as its rect: the same pass over the mask's span and the same gather of geoA, k_mark<DOT>'s floor
 (4)  gsr_render_wire_over of the whole cloud (wall clock): what a 100 % outline is measured against
 (5)  the read-back path the verb replaces: gsr_read of P and alpha plus the mask over the link (wall clock), before any drawing
The 100 % images are compared with each other where the contract says they agree: outlines of every splat with ANY_OPACITY are
gsr_render_wire_over's bytes."""
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
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n, W, H = splats.n, cfg["width"], cfg["height"]
words = (n + 31) // 32
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


def to_device(p, a):
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0


cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
cs = E.camera_struct(cam)
rng = np.random.default_rng(7)
draw = rng.random(n)
print("%s: %d splats, %dx%d; median [min .. max] of %d calls, ms" % (name, n, W, H, reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    frame, target, dmask = device_room(W * H * 16), device_room(W * H * 16), device_room(words * 4)
    eng.render_struct_to_device(cs, frame.value)
    eng.synchronize()

    def fresh():
        assert hip.hipMemcpy(target, frame, C.c_size_t(W * H * 16), 3) == 0

    for label, style in (("dots r=1", E.mark_style(E.MARK_DOT, 1, (1.0, 1.0, 0.0, 1.0))), ("outlines", E.mark_style(E.MARK_OUTLINE, 0, "cd"))):
        for frac in (0.01, 0.1, 1.0):
            m = draw < frac
            to_device(dmask, E.pack_mask(m))
            ms, px = [], 0
            for r in range(reps + 1):
                fresh()
                px = eng.render_marks_device(cs, dmask.value, style, target.value)
                if r:
                    ms.append(eng.get_marks()["ms"])
            ms = np.asarray(ms)
            print("%-9s %5.1f %% (%8d splats)  clear + k_mark %s   k_mark_resolve %s   copies %s   wall %s   %d pixels"
                  % (label, frac * 100, int(m.sum()), cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 2]), cell(ms[:, 3]), px), flush=True)

    # (3) k_select over the whole frame: the floor of k_mark<DOT>
    ms = []
    for r in range(reps + 1):
        eng.select_device(cs, E.select_region((0.0, 0.0, float(W), float(H))), dmask.value)
        if r:
            ms.append(eng.get_select()["ms"])
    ms = np.asarray(ms)
    print("gsr_select, whole-frame rect: kernel %s   wall %s" % (cell(ms[:, 0]), cell(ms[:, 3])), flush=True)

    # (4) the wire overlay of the whole cloud, and the 100 % outline with ANY_OPACITY beside it: the same bytes
    wall = []
    for r in range(reps + 1):
        fresh()
        t0 = time.perf_counter()
        eng.render_wire_over_device(cam, target.value)
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    wire = np.empty((H, W, 4), np.float32)
    assert hip.hipMemcpy(C.c_void_p(wire.ctypes.data), target, C.c_size_t(wire.nbytes), 2) == 0
    print("gsr_render_wire_over, whole cloud: wall %s" % cell(wall), flush=True)
    fresh()
    wall = []
    for r in range(reps + 1):
        fresh()
        eng.render_marks_device(cs, None, E.mark_style(E.MARK_OUTLINE, 0, "cd", any_opacity=True), target.value)
        if r:
            wall.append(eng.get_marks()["ms"])
    wall = np.asarray(wall)
    mine = np.empty((H, W, 4), np.float32)
    assert hip.hipMemcpy(C.c_void_p(mine.ctypes.data), target, C.c_size_t(mine.nbytes), 2) == 0
    print("outlines, NULL mask, ANY_OPACITY: clear + k_mark %s   k_mark_resolve %s   wall %s   same bytes as the wire overlay: %s"
          % (cell(wall[:, 0]), cell(wall[:, 1]), cell(wall[:, 3]), np.array_equal(mine.view(np.uint32), wire.view(np.uint32))), flush=True)

    # (5) the read-back path: P and alpha of the cloud and the mask over the link, before the caller has drawn a single point
    wall = []
    back_mask = np.empty(words, np.uint32)
    for r in range(max(3, reps // 4) + 1):
        t0 = time.perf_counter()
        back = eng.read(names=("P", "alpha"))
        assert hip.hipMemcpy(C.c_void_p(back_mask.ctypes.data), dmask, C.c_size_t(back_mask.nbytes), 2) == 0
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    print("(before) gsr_read of P and alpha + the mask: wall %s   (%.0f MB over the link)" % (cell(wall), (n * 16 + words * 4) / 1e6), flush=True)
    for p in (frame, target, dmask):
        hip.hipFree(p)
