"""gsr_select_density beside the sort it is built on and beside the only way there was before it, in one session:
    python tools/density_probe.py [C4] [--reps 20] [--n N] [--before 2]
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), from the verb's own clock (gsr_get_select_density:
[0] k_density_keys + k_density_count + k_density_hit, [1] copies, [2] the four-pass sort, [3] wall), every call into a DEVICE mask
(REPLACE), count = (1, 3):
 (8)   a cell chosen so that the mean occupancy n_population / n_cells is about 8, taken from the verb's own n_cells; reach 0, 1, 2
       (reach 0 searches one row: what is left of [0] beside it is the count kernel's searches)
 (x4)  a cell four times that size; reach 0, 1, 2
 (m)   the ordering stage of a gsr_move of one splat over the same cloud (gsr_stats.move_ms[1]: the box, the Morton codes, the same
       four-pass sort of n pairs, the copy of the permutation) -- the verb's [2] is that sort alone
 (0)   the only way before: Engine.read of P and alpha, the numpy restatement of tests/density_cases.py, the mask packed and copied
       back to the device
Each device mask is compared with gsr_select_density_eval over the whole cloud (the rule on the host)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import __graft_entry__ as ge
import density_cases as DC

pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
reps = int(opt("--reps", "20"))
before_reps = int(opt("--before", "2"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
words = (n + 31) // 32
cell_s = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")
COUNT = (1, 3)


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, splats.shx is not None, reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    dmask = device_room(words * 4)
    lo, hi = splats.P.min(axis=0), splats.P.max(axis=0)
    extent = float((hi - lo).max())

    def occupancy(cell):
        origin, c = E.density_grid(lo, hi, cell)
        _, _, res = eng.select_density_device(E.density_rule(c, origin, reach=0, count=COUNT), dmask.value)
        return res.n_population / max(res.n_cells, 1)

    # the cell of mean occupancy 8, from the verb's own n_cells: a few steps of cell *= cbrt(8 / occupancy)
    cell8 = max(extent / max(np.cbrt(n / 8.0), 1.0), extent / 1000.0)
    for step in range(6):
        occ = occupancy(cell8)
        if abs(occ - 8.0) < 0.4:
            break
        cell8 = max(cell8 * float(np.cbrt(8.0 / occ)), extent / 1000.0)
    print("cell of mean occupancy 8: %.6g (extent %.4g: %.0f cells across; occupancy %.2f after %d steps)" % (cell8, extent, extent / cell8, occ, step + 1), flush=True)

    sort_ms = []
    for label, cell in (("(8) ", cell8), ("(x4)", 4.0 * cell8)):
        origin, c = E.density_grid(lo, hi, cell)
        for reach in (0, 1, 2):
            rule = E.density_rule(c, origin, reach=reach, count=COUNT)
            ms = []
            for r in range(reps + 1):
                n_hit, n_set, res = eng.select_density_device(rule, dmask.value)
                if r:
                    ms.append(eng.get_select_density()["ms"])
            ms = np.asarray(ms)
            sort_ms.append(ms[:, 2])
            got = np.empty(words, np.uint32)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dmask, C.c_size_t(got.nbytes), 2) == 0
            want, wres = E.select_density_eval(rule, splats.P, splats.alpha, result=True)
            assert np.array_equal(got, E.pack_mask(want)) and wres.fields() == res.fields(), label + ": the device result is not the host rule's"
            print("%s cell %.5g reach %d: kernels %s   sort %s   copies %s   wall %s   verb / sort %.2f   occupancy %.2f   hits %d   N>=64: %d"
                  % (label, float(c), reach, cell_s(ms[:, 0]), cell_s(ms[:, 2]), cell_s(ms[:, 1]), cell_s(ms[:, 3]),
                     np.median(ms[:, 0] + ms[:, 2]) / np.median(ms[:, 2]), res.n_population / max(res.n_cells, 1), n_hit, res.count_hist[63]), flush=True)
    print("the sort inside the verb, all rows: %s" % cell_s(np.concatenate(sort_ms)), flush=True)

    # ---- the only way before: P and alpha over the link, the restatement in numpy, the mask back
    origin, c = E.density_grid(lo, hi, cell8)
    rule = E.density_rule(c, origin, reach=1, count=COUNT)
    want = E.select_density_eval(rule, splats.P, splats.alpha)
    read_ms, host_ms, back_ms = [], [], []
    for r in range(before_reps):
        t0 = time.perf_counter()
        R = eng.read(names=("P", "alpha"))
        t1 = time.perf_counter()
        sel = DC.restate(R.P, R.alpha, c, origin, reach=1, count=COUNT)[0]
        host_words = E.pack_mask(sel)
        t2 = time.perf_counter()
        assert hip.hipMemcpy(dmask, C.c_void_p(host_words.ctypes.data), C.c_size_t(host_words.nbytes), 1) == 0
        t3 = time.perf_counter()
        read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3); back_ms.append((t3 - t2) * 1e3)
        assert np.array_equal(sel, want), "the restatement is not the host rule's"
    if before_reps:
        print("(0) before, cell (8) reach 1: Engine.read of P and alpha %s   numpy restatement + packing %s   mask to the device %s   (%.0f MB over "
              "the link; %d hits)" % (cell_s(read_ms), cell_s(host_ms), cell_s(back_ms), n * 16 / 1e6, int(want.sum())), flush=True)

    # ---- the ordering of a move over the same cloud (last: it gives the context its spare planes)
    order_ms = []
    for r in range(reps // 2 + 1):
        eng.move(0, splats.P[:1])
        if r:
            order_ms.append(eng.stats()["move_ms"][1])
    print("(m) ordering stage of gsr_move (box + codes + the same sort + copy): %s" % cell_s(order_ms), flush=True)
    hip.hipFree(dmask)
