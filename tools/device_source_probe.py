"""Device sources against the host verbs, in one session: python tools/device_source_probe.py [C4] [--reps 20] [--n N] [--torch] [--host-only]
Six cases are run INTERLEAVED on one Engine, `reps` times each after one unmeasured round (which allocates the spare planes, the sort
scratch and the inverse permutation):
  a whole-cloud Cd + alpha edit      through update_attrs_device (float32 rows in device memory) and through update_attrs (halves on the host)
  a whole-cloud move                 through move_device and through move
  a move of 1 % of the cloud         each way (a contiguous range in the middle)
Two sets of source arrays alternate, so every call really changes what is resident (the tool checks that the storage order changes
with every timed move, outside the timed calls).  The device sources are raw
hipMalloc buffers, or with --torch torch tensors (torch is then imported FIRST, so the library shares its HIP runtime).  --host-only runs
the three host cases alone: from another tree's root (cd _tree && python ../tools/device_source_probe.py --host-only) it times THAT tree's
host verbs on the same box, which is the yardstick a device verb is held to.
Prints, per case: MB over the link, then median [min .. max] of the wall time of the (synchronous) call and of its stage times --
gsr_stats.upload_ms[4], [5] for an update (host -> device / kernels), move_ms[0..3] for a move (host -> device / order / repack / call)."""
import sys, time
sys.path.insert(0, '.')
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
use_torch, host_only = "--torch" in sys.argv, "--host-only" in sys.argv
if use_torch:
    import torch
import ctypes as C
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
reps = int(opt("--reps", "20"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
rng = np.random.default_rng(5)
ext = splats.P.max(axis=0) - splats.P.min(axis=0)
part_first, part_n = n // 2, max(n // 100, 1)
# two sets of sources: float32 as a device caller holds them, and the same values as the host verbs take them (Cd quantised on the host)
P = [np.ascontiguousarray(splats.P, np.float32)]
P.append((P[0] + rng.uniform(-1.0, 1.0, P[0].shape).astype(np.float32) * (0.01 * ext).astype(np.float32)).astype(np.float32))
Cd = [rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32) for _ in range(2)]
al = [rng.uniform(0.05, 1.0, n).astype(np.float32) for _ in range(2)]
Cd_h = [pkg.engine.quantize_half(a) for a in Cd]
Ppart = [np.ascontiguousarray(a[part_first:part_first + part_n]) for a in P]
eng = pkg.Engine(0)
eng.upload(splats)
cam = pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], 0)
eng.render(cam)
dev = {}
if not host_only:
    if use_torch:
        put = lambda a: torch.from_numpy(a).cuda()
        kw = lambda a: {}
    else:
        hip = C.CDLL("libamdhip64.so")
        def put(a):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
            return p.value
        kw = lambda a: {"n": len(a)}
    dev = {"P": [put(a) for a in P], "Cd": [put(a) for a in Cd], "alpha": [put(a) for a in al], "Ppart": [put(a) for a in Ppart]}
    if use_torch:
        torch.cuda.synchronize()
# cur: which of the two position sets is resident.  A whole-cloud move goes to the other set; a 1 % move takes the range to its rows of the
# other set and an UNTIMED move brings it back, so every timed move really moves its splats and changes the storage order.
cur = 0
def whole(device):
    global cur
    cur = 1 - cur
    return eng.move_device(0, dev["P"][cur], **kw(P[cur])) if device else eng.move(0, P[cur])
def part(device, k):
    return eng.move_device(part_first, dev["Ppart"][k], **kw(Ppart[k])) if device else eng.move(part_first, Ppart[k])
CASES = {
    "update Cd+alpha, device": lambda k: eng.update_attrs_device(0, Cd=dev["Cd"][k], alpha=dev["alpha"][k], **kw(Cd[k])),
    "update Cd+alpha, host": lambda k: eng.update_attrs(0, Cd=Cd_h[1 - k], alpha=al[1 - k]),
    "whole move, device": lambda k: whole(True),
    "whole move, host": lambda k: whole(False),
    "1 % move, device": lambda k: part(True, 1 - cur),
    "1 % move, host": lambda k: part(False, 1 - cur),
}
if host_only:
    CASES = {k: v for k, v in CASES.items() if k.endswith("host")}
MB = {"update Cd+alpha, device": 0.0, "update Cd+alpha, host": n * 10 / 1e6, "whole move, device": 0.0, "whole move, host": n * 12 / 1e6,
      "1 % move, device": 0.0, "1 % move, host": part_n * 12 / 1e6}
times = {label: [] for label in CASES}
changed = {label: [] for label in CASES if "move" in label}
order = eng.debug_storage_order(n)
for r in range(reps + 1):
    for label, call in CASES.items():
        eng.synchronize(); t0 = time.perf_counter()
        call(r % 2)
        dt = (time.perf_counter() - t0) * 1e3
        st = eng.stats()
        if r:                                           # (the first round allocates)
            times[label].append([dt] + (list(st["upload_ms"][4:6]) + [0.0, 0.0] if label.startswith("update") else list(st["move_ms"])))
        if label in changed:                            # (not timed) how many slots hold another splat than before the call
            now = eng.debug_storage_order(n)
            changed[label].append(int((now != order).sum()))
            order = now
        if label.startswith("1 %"):                     # (not timed) the range back to where the whole-cloud move left it
            part(not host_only, cur)
            order = eng.debug_storage_order(n)
    eng.render(cam)
print("%s: %d splats, SH %s; %s sources; median [min .. max] of %d calls, ms" % (
    name, n, "yes" if splats.has_sh else "no", "host only" if host_only else ("torch tensors" if use_torch else "raw device buffers"), reps), flush=True)
print("%-26s %9s  %-24s %-24s %-24s %-24s %-24s" % ("case", "MB link", "wall", "[0] h->d", "[1] kernels / order", "[2] repack", "[3] call"), flush=True)
for label, rows in times.items():
    a = np.asarray(rows)
    cell = lambda j: "%.3f [%.3f .. %.3f]" % (np.median(a[:, j]), a[:, j].min(), a[:, j].max())
    print("%-26s %9.1f  %-24s %-24s %-24s %-24s %-24s" % (label, MB[label], cell(0), cell(1), cell(2), cell(3), cell(4)), flush=True)
if not host_only:
    med = lambda label: float(np.median(np.asarray(times[label])[:, 0]))
    for d, h in (("update Cd+alpha, device", "update Cd+alpha, host"), ("whole move, device", "whole move, host"), ("1 % move, device", "1 % move, host")):
        print("%-26s %.3f ms against %.3f ms from the host: %s" % (d, med(d), med(h), "not longer" if med(d) <= med(h) else "LONGER"), flush=True)
print("slots whose splat changed, per timed move:", {k: (min(v[1:]), max(v[1:])) for k, v in changed.items()}, flush=True)
assert all(min(v[1:]) > 0 for v in changed.values()), "a move left the storage order as it was: the case measures a straight copy"
eng.close()
