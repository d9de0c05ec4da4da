"""gsr_read / gsr_read_device beside the upload that runs the same bytes the other way, in one session:
    python tools/read_probe.py [C4] [--reps 20] [--n N]
Medians [min .. max] of `reps` calls, from the verb's own clock (gsr_get_read: kernel, device -> host copies, wall), of
 (1)  a whole-cloud gsr_read_device with everything, sh_vec3_per_point = 15 (a trainer's features_rest)
 (2)  a P-only whole-cloud gsr_read_device
 (3)  a whole-cloud gsr_read (host arrays)
 (4)  gsr_read and gsr_read_device of 1 % of the cloud (from the middle of the upload order)
and beside them, from the same session, the upload's stage clock: upload_ms[2] is k_pack -- the same bytes the other way -- and
upload_ms[0] the link's rate, the floor of the host form.  The whole-cloud reads are compared with the arrays that were uploaded."""
import ctypes as C
import sys

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
n, sh = splats.n, splats.has_sh
cell = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")
half_row = 36 + (96 if sh else 0)                   # bytes of a splat in gsr_upload_append's layout
f32_row = 64 + (180 if sh else 0)                   # ... in gsr_device_attrs' layout at 15 vec3 per point
res_row = 32 + (128 if sh else 16)                  # what k_unpack loads of a splat when everything is wanted


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


def clocks(eng, call):
    out = []
    for r in range(reps + 1):                       # (the first call allocates: the arena, the inverse of the storage order, the events)
        call()
        if r:
            out.append(eng.get_read()["ms"])
    return np.asarray(out)


print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, "yes" if sh else "no", reps), flush=True)
with pkg.Engine(0) as eng:
    up = []
    for r in range(3):
        eng.upload(splats)
        up.append(eng.stats()["upload_ms"][:4])
    up = np.asarray(up)
    print("gsr_upload:                 link (upload_ms[0]) %s = %.1f GB/s   k_pack (upload_ms[2]) %s   wall %s   (%d MB over the link)"
          % (cell(up[:, 0]), n * half_row / 1e6 / np.median(up[:, 0]), cell(up[:, 2]), cell(up[:, 3]), n * half_row // 1000000), flush=True)
    pack_ms = float(np.median(up[:, 2]))
    width = {"P": 3, "Cd": 3, "alpha": 1, "scale": 3, "orient": 4, **({"sh": 45} if sh else {})}
    room = {k: device_room(n * w * 4) for k, w in width.items()}
    ptrs = {k: v.value for k, v in room.items()}
    vpp = 15 if sh else None
    m, first = max(1, n // 100), n // 2

    ms = clocks(eng, lambda: eng.read_device(ptrs, 0, n, vpp))
    k_all = float(np.median(ms[:, 0]))
    print("(1) gsr_read_device, everything, vpp 15:   kernel %s = %.0f GB/s read + written   wall %s   (%.2f x k_pack%s)"
          % (cell(ms[:, 0]), n * (res_row + f32_row) / 1e6 / k_all, cell(ms[:, 3]), k_all / pack_ms,
             ": MORE THAN TWICE k_pack" if k_all > 2 * pack_ms else ""), flush=True)
    got = np.empty((n, 3), np.float32)
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), room["P"], C.c_size_t(got.nbytes), 2) == 0
    assert np.array_equal(got.view(np.uint32), splats.P.view(np.uint32)), "the P read back is not the P uploaded"
    ms = clocks(eng, lambda: eng.read_device({"P": ptrs["P"]}, 0, n))
    print("(2) gsr_read_device, P only:               kernel %s = %.0f GB/s read + written   wall %s"
          % (cell(ms[:, 0]), n * (16 + 4 + 12) / 1e6 / np.median(ms[:, 0]), cell(ms[:, 3])), flush=True)
    back = [None]

    def whole():
        back[0] = eng.read()
    ms = clocks(eng, whole)
    print("(3) gsr_read, everything:                  kernel %s   device -> host %s = %.1f GB/s   wall %s   (%d MB over the link)"
          % (cell(ms[:, 0]), cell(ms[:, 1]), n * half_row / 1e6 / np.median(ms[:, 1]), cell(ms[:, 3]), n * half_row // 1000000), flush=True)
    for k in ("P", "Cd", "alpha", "scale", "orient") + (("shx", "shy", "shz") if sh else ()):
        assert np.array_equal(getattr(back[0], k).view(np.uint8), np.ascontiguousarray(getattr(splats, k)).view(np.uint8)), k + " read back is not what was uploaded"
    # ... and into the SAME host arrays every time (Engine.read allocates fresh ones per call, whose pages the copy touches first)
    names = tuple(k for k, _, _ in E.READ_ARRAYS if sh or not k.startswith("sh"))
    r, keep = E.read_arrays_struct(n, names)
    ms = clocks(eng, lambda: E._check(eng.L.gsr_read(eng.h, 0, n, C.byref(r))))
    print("(3) gsr_read, the same destinations again: kernel %s   device -> host %s = %.1f GB/s   wall %s"
          % (cell(ms[:, 0]), cell(ms[:, 1]), n * half_row / 1e6 / np.median(ms[:, 1]), cell(ms[:, 3])), flush=True)
    assert all(np.array_equal(keep[k].view(np.uint8), getattr(back[0], k).view(np.uint8)) for k in names)
    del keep, r
    ms = clocks(eng, lambda: eng.read(first, m))
    print("(4) gsr_read of 1 %% (%d rows):          kernel %s   device -> host %s   wall %s" % (m, cell(ms[:, 0]), cell(ms[:, 1]), cell(ms[:, 3])), flush=True)
    ms = clocks(eng, lambda: eng.read_device(ptrs, first, m, vpp))
    print("(4) gsr_read_device of 1 %% (%d rows):   kernel %s   wall %s" % (m, cell(ms[:, 0]), cell(ms[:, 3])), flush=True)
    st = eng.stats()
    assert st["uploads"] == 3 and st["moves"] == 0
    for p in room.values():
        hip.hipFree(p)
