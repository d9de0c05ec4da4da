"""gsr_read_masked_device, gsr_read_masked and gsr_duplicate beside the only way there was before them, in one session:
    python tools/copy_probe.py [C4] [--reps 20] [--n N]
Medians [min .. max] of `reps` calls, ms, for seeded random selections of 1 %, 10 % and 100 % of the cloud, each from a DEVICE mask (the
rows that come back are compared with the arrays that were uploaded, outside the clocks):
 (1)  read_masked_device into float32 device arrays (sh_vec3_per_point 16): the wall clock of the call and the kernels between their HIP
      events (gsr_get_read: compaction + k_unpack); beside it gsr_read_device of the whole cloud, the yardstick of the 100 % case
 (2)  gsr_read_masked into host arrays sized by the selection: wall, kernels, device -> host copies
 (3)  gsr_duplicate: the verb's stage clock (gsr_get_duplicate: mark .. sort, repack, wall).  Every call changes the cloud, so every
      call gets a FRESH context (create, upload, one unmeasured frame)
 (4)  the only way before: gsr_read of the whole cloud plus the numpy index -- and the same followed by gsr_add of the rows"""
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
cam = pkg.scenes.config_camera(name, pkg.camera, W, H, cfg["sh_order"], 0)
sh = splats.has_sh
row_f32 = 4 * (3 + 3 + 1 + 3 + 4 + (48 if sh else 0))
row_half = 12 + 4 + 6 + 6 + 8 + (96 if sh else 0)


def dev_alloc(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p.value


def fresh():
    eng = pkg.Engine(0)
    eng.upload(splats)
    eng.render(cam)
    return eng


print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, "yes" if sh else "no", reps), flush=True)
rng = np.random.default_rng(7)
selections = {}
for label, share in (("1 %", 0.01), ("10 %", 0.1), ("100 %", 1.0)):
    sel = np.ones(n, bool) if share == 1.0 else rng.random(n) < share
    w = E.pack_mask(sel)
    d = dev_alloc(words * 4)
    assert hip.hipMemcpy(C.c_void_p(d), C.c_void_p(w.ctypes.data), C.c_size_t(w.nbytes), 1) == 0
    selections[label] = (sel, w, d, int(sel.sum()))

dst = {k: dev_alloc(n * 4 * wd) for k, wd in (("P", 3), ("Cd", 3), ("alpha", 1), ("scale", 3), ("orient", 4))}
if sh:
    dst["sh"] = dev_alloc(n * 4 * 48)
vpp = 16 if sh else None

with fresh() as eng:
    # ---- (1) the device form, and gsr_read_device of everything beside it
    wall, kern = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        eng.read_device(dst, 0, n, sh_vec3_per_point=vpp)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(eng.get_read()["ms"][0])
    print("(1) gsr_read_device, whole cloud:              wall %s   k_unpack %s   (%.0f MB written)" % (cell(wall[1:]), cell(kern[1:]), n * row_f32 / 1e6), flush=True)
    for label, (sel, w, d, m) in selections.items():
        wall, kern = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            got = eng.read_masked_device(dst, d, n, sh_vec3_per_point=vpp)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(eng.get_read()["ms"][0])
        assert got == m
        check = np.empty((m, 3), np.float32)                   # the content too: P of every row
        assert hip.hipMemcpy(C.c_void_p(check.ctypes.data), C.c_void_p(dst["P"]), C.c_size_t(check.nbytes), 2) == 0
        assert np.array_equal(check.view(np.uint32), splats.P[sel].view(np.uint32)), "read_masked_device: wrong rows"
        print("(1) read_masked_device %5s (%8d rows):    wall %s   compact + k_unpack %s   (%.1f MB written)"
              % (label, m, cell(wall[1:]), cell(kern[1:]), m * row_f32 / 1e6), flush=True)
    # ---- (2) the host form (the count call of the Python wrapper is left out: the arrays are sized here)
    L = pkg.load_library()
    for label, (sel, w, d, m) in selections.items():
        r_, arrays = E.read_arrays_struct(m, tuple(k for k, _, _ in E.READ_ARRAYS if sh or not k.startswith("sh")))
        wall, kern, copy = [], [], []
        cnt = C.c_int64(0)
        for r in range(reps + 1):
            t0 = time.perf_counter()
            E._check(L.gsr_read_masked(eng.h, C.c_void_p(d), 1, m, C.byref(r_), C.byref(cnt)))
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = eng.get_read()["ms"]
            kern.append(ms[0]); copy.append(ms[1])
        assert cnt.value == m
        last = np.flatnonzero(sel)[-1]                          # the content too: P and alpha of every row, every array of the last row
        assert np.array_equal(arrays["P"].view(np.uint32), splats.P[sel].view(np.uint32)), "read_masked: wrong rows"
        assert np.array_equal(arrays["alpha"].view(np.uint32), splats.alpha[sel].view(np.uint32))
        assert all(np.array_equal(arrays[k][-1], getattr(splats, k)[last]) for k in arrays if not k.startswith("sh"))
        print("(2) read_masked        %5s (%8d rows):    wall %s   compact + k_unpack %s   copies %s   (%.1f MB over the link)"
              % (label, m, cell(wall[1:]), cell(kern[1:]), cell(copy[1:]), m * row_half / 1e6), flush=True)
    # ---- (4a) the only way before a masked read: everything over the link, and the numpy index
    for label, (sel, w, d, m) in selections.items():
        rd, ix = [], []
        for r in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            back = eng.read()
            t1 = time.perf_counter()
            rows = back.subset(sel)
            t2 = time.perf_counter()
            rd.append((t1 - t0) * 1e3); ix.append((t2 - t1) * 1e3)
        assert rows.n == m
        print("(4) before, %5s: gsr_read of everything %s (%.0f MB over the link)   numpy index %s" % (label, cell(rd), n * row_half / 1e6, cell(ix)), flush=True)

# ---- (3) duplicate: a fresh context per call
for label, (sel, w, d, m) in selections.items():
    ms, wall = [], []
    for r in range(reps):
        with fresh() as eng:
            eng.synchronize()
            t0 = time.perf_counter()
            got = eng.duplicate_device(d)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.get_duplicate()["ms"])
            assert got == (m, n + m)
            if r == 0:                                          # the content too: the copies' P, and one whole copy
                tail = eng.read(n, m, names=("P", "Cd", "alpha"))
                assert np.array_equal(tail.P.view(np.uint32), splats.P[sel].view(np.uint32)), "duplicate: wrong copies"
                assert np.array_equal(tail.Cd[-1], splats.Cd[np.flatnonzero(sel)[-1]])
    ms = np.asarray(ms)
    print("(3) duplicate          %5s (%8d copies):  wall %s   mark .. sort %s   repack %s" % (label, m, cell(wall), cell(ms[:, 1]), cell(ms[:, 2])), flush=True)

# ---- (4b) the only way before a duplicate: everything over the link, the numpy index, gsr_add of the rows
for label, (sel, w, d, m) in selections.items():
    rd, ix, ad = [], [], []
    for r in range(max(3, reps // 4)):
        with fresh() as eng:
            eng.synchronize()
            t0 = time.perf_counter()
            back = eng.read()
            t1 = time.perf_counter()
            rows = back.subset(sel)
            t2 = time.perf_counter()
            assert eng.add(rows) == n + m
            t3 = time.perf_counter()
            rd.append((t1 - t0) * 1e3); ix.append((t2 - t1) * 1e3); ad.append((t3 - t2) * 1e3)
    print("(4) before, %5s: gsr_read %s   numpy index %s   gsr_add %s   (%.0f MB down, %.1f MB up)"
          % (label, cell(rd), cell(ix), cell(ad), n * row_half / 1e6, m * row_half / 1e6), flush=True)
for p in [v[2] for v in selections.values()] + list(dst.values()):
    hip.hipFree(C.c_void_p(p))
