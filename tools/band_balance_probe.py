"""What balanced bands buy, on ONE GPU: python tools/band_balance_probe.py [T1] [--ranks 4 | 2,4,8] [--steps 60] [--warmup 20] [--n N] [--multi]
Every rank's band is rendered alone on the one GPU (an explicit band, gsr_set_row_band -- what bench.py --emulate-shard does for layout
1), along the config's orbit, under the equal split and under the boundaries the balancer (gsr_debug_balance_rows) derives from the row
work of the unsharded frame (GSR_OPT_ROW_WORK).  Prints per-rank ms per frame, the heaviest band -- what sets the frame rate of the
multi-GPU run -- and the boundaries.  Serial frames into a device target, wall clock over `steps` frames behind `warmup` unmeasured ones.
--multi: also the whole path through gsr_multi over the COPY transport (the ranks are contexts on this GPU, so their bands run one
after the other: the figure is the SUM of the bands plus the gather, not a multi-GPU frame rate) in layouts 1 and 2, the wall time of
every frame of the layout-2 run around its rebalances (what one rebalance costs, in frames) and the gain the balancer saw.
Nothing here crosses xGMI."""
import sys, time
sys.path.insert(0, '.')
import numpy as np
import __graft_entry__ as ge

pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "T1"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
rank_list, steps, warmup = [int(x) for x in opt("--ranks", "4").split(",")], int(opt("--steps", "60")), int(opt("--warmup", "20"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
W, H, order = cfg["width"], cfg["height"], cfg["sh_order"]
tiles_y = (H + 15) // 16
cams = [E.camera_struct(pkg.scenes.config_camera(name, pkg.camera, W, H, order, i)) for i in range(warmup + steps)]

import torch
target = torch.zeros((tiles_y * 16 + 16, W, 4), dtype=torch.float32, device="cuda:0")


def timed(eng):
    for c in cams[:warmup]:
        eng.render_struct_to_device(c, target.data_ptr())
    eng.synchronize()
    t0 = time.perf_counter()
    for c in cams[warmup:]:
        eng.render_struct_to_device(c, target.data_ptr())
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


eng = pkg.Engine(0)
eng.set_option(E.OPT_STAGE_TIMING, 0)
eng.set_option(E.OPT_ROW_WORK, 1)
eng.upload(splats)
full_ms = timed(eng)
work, _ = eng.read_row_work(H)
eng.set_option(E.OPT_ROW_WORK, 0)
print(f"{name}: {splats.n} splats, {W}x{H} ({tiles_y} tile rows); unsharded frame {full_ms:.4f} ms", flush=True)
for ranks in rank_list:
    print(f"-- {ranks} ranks", flush=True)
    _, equal = E.balance_rows(np.zeros(tiles_y, np.uint32), ranks)
    _, balanced = E.balance_rows(work, ranks)
    share = lambda first: [round(float(work[first[g]:first[g + 1]].astype(np.float64).sum() / max(float(work.sum()), 1.0)), 3) for g in range(ranks)]
    for label, first in (("equal split (layout 1)", equal), ("balanced (layout 2)", balanced)):
        ms = []
        for g in range(ranks):
            eng.set_row_band(int(first[g]), int(first[g + 1] - first[g]))
            ms.append(timed(eng) if first[g + 1] > first[g] else 0.0)
        print(f"{label:24s} boundaries {first.tolist()}  work share {share(first)}", flush=True)
        print(f"{'':24s} ms per rank {[round(m, 4) for m in ms]}  heaviest {max(ms):.4f} ms  lightest {min(ms):.4f} ms", flush=True)
eng.close()

if "--multi" in sys.argv:
    ranks = rank_list[0]
    ref = pkg.Engine(0)
    ref.upload(splats)
    for layout in (1, 2):
        with pkg.MultiEngine([0] * ranks, E.TRANSPORT_COPY) as M:
            M.set_option(E.OPT_SHARD_LAYOUT, layout)
            M.set_option(E.OPT_STAGE_TIMING, 0)
            M.upload(splats)
            per_frame, marks, seen = [], [], 0
            for k, c in enumerate(cams):
                M.synchronize(); t0 = time.perf_counter()
                M.render_struct_to_device(c, target.data_ptr())
                M.synchronize()
                per_frame.append((time.perf_counter() - t0) * 1e3)
                first, n = M.get_bands()
                if n != seen:
                    marks.append((k, first.tolist())); seen = n
            steady = float(np.median(per_frame[warmup:]))
            same = np.array_equal(M.render(pkg.scenes.config_camera(name, pkg.camera, W, H, order, 3)),
                                  ref.render(pkg.scenes.config_camera(name, pkg.camera, W, H, order, 3)))
            print(f"gsr_multi layout {layout}: median frame {steady:.4f} ms (bands in turn on one GPU + gather), bit-identical {same}, "
                  f"boundaries {M.get_bands()[0].tolist()}, rebalances {seen}", flush=True)
            for k, first in marks:
                # (the frame whose call rebalanced is k: the boundaries reported after it are new)
                around = [round(t, 3) for t in per_frame[max(k - 2, 0): k + 6]]
                extra = sum(t - steady for t in per_frame[k: k + 5])
                print(f"  rebalance in front of frame {k} -> {first}: frames {max(k - 2, 0)}..{k + 5} took {around} ms; "
                      f"frames {k}..{k + 4} cost {extra:.3f} ms more than five steady ones ({extra / steady:.1f} frame times)", flush=True)
    ref.close()
