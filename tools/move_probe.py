"""gsr_move against a full re-upload, in one session: python tools/move_probe.py [C4] [--reps 5] [--n N]
Three cases are run INTERLEAVED, `reps` times each after one unmeasured round (which allocates the spare planes, the sort scratch and
the inverse permutation): a whole-cloud move, the full re-upload of the same arrays, and a move of 1 % of the cloud (a contiguous
range in the middle).  Two position arrays alternate, the cloud's own and a copy jittered by up to 1 % of the box: in a round the
whole cloud moves to one of them, the upload stages that one, and the 1 % range then moves to ITS ROWS OF THE OTHER -- so every move
really moves its splats and changes the storage order (the tool checks that, outside the timed calls).
Prints, per case: MB host -> device, then median [min .. max] of the wall time of the call and of the four stage times --
gsr_stats.move_ms[0..3] for a move, upload_ms[0..3] for the upload: host -> device / box + codes + sort / repack or pack / whole call."""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import __graft_entry__ as ge
pkg = ge.load_package()
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
reps = int(opt("--reps", "5"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
rng = np.random.default_rng(5)
ext = splats.P.max(axis=0) - splats.P.min(axis=0)
P0 = np.ascontiguousarray(splats.P, np.float32)
P1 = (P0 + rng.uniform(-1.0, 1.0, P0.shape).astype(np.float32) * (0.01 * ext).astype(np.float32)).astype(np.float32)
part_first, part_n = n // 2, max(n // 100, 1)
g = lambda a: None if a is None else a
moved = pkg.scenes.Splats(P1, g(splats.Cd), g(splats.alpha), g(splats.scale), g(splats.orient), g(splats.shx), g(splats.shy), g(splats.shz))
row_bytes = 12 + 4 + 6 + 6 + 8 + (96 if splats.has_sh else 0)
eng = pkg.Engine(0)
eng.upload(splats)
cam = pkg.scenes.config_camera(name, pkg.camera, cfg["width"], cfg["height"], cfg["sh_order"], 0)
eng.render(cam)
times = {"whole-cloud move": [], "full upload": [], "1 % move": []}
part_rows = [np.ascontiguousarray(Q[part_first:part_first + part_n]) for Q in (P0, P1)]
changed = {label: [] for label in times}
order = eng.debug_storage_order(n)
for r in range(reps + 1):
    P, cloud, other = (P1, moved, part_rows[0]) if r % 2 == 0 else (P0, splats, part_rows[1])
    for label in times:
        eng.synchronize(); t0 = time.perf_counter()
        if label == "whole-cloud move":
            eng.move(0, P)
        elif label == "full upload":
            eng.upload(cloud)
        else:
            eng.move(part_first, other)
        dt = (time.perf_counter() - t0) * 1e3
        st = eng.stats()
        now = eng.debug_storage_order(n)                # (not timed) how many slots hold another splat than before the call
        changed[label].append(int((now != order).sum()))
        order = now
        if r:                                           # (the first round allocates)
            times[label].append([dt] + list(st["upload_ms"][:4] if label == "full upload" else st["move_ms"]))
    eng.render(cam)
print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, "yes" if splats.has_sh else "no", reps), flush=True)
print("%-18s %9s  %-24s %-24s %-24s %-24s %-24s" % ("case", "MB h->d", "wall", "[0] h->d", "[1] order", "[2] repack / pack", "[3] call"), flush=True)
mb = {"whole-cloud move": n * 12 / 1e6, "full upload": n * row_bytes / 1e6, "1 % move": part_n * 12 / 1e6}
for label, rows in times.items():
    a = np.asarray(rows)
    cell = lambda k: "%.3f [%.3f .. %.3f]" % (np.median(a[:, k]), a[:, k].min(), a[:, k].max())
    print("%-18s %9.1f  %-24s %-24s %-24s %-24s %-24s" % (label, mb[label], cell(0), cell(1), cell(2), cell(3), cell(4)), flush=True)
print("slots whose splat changed, per call:", {k: (min(v[1:]), max(v[1:])) for k, v in changed.items()},
      "(the upload re-stages what the move before it left: 0)", flush=True)
assert min(changed["whole-cloud move"][1:]) > 0 and min(changed["1 % move"][1:]) > 0, "a move left the storage order as it was: the case measures a straight copy"
eng.close()
