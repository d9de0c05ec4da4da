"""gsr_select_connected beside gsr_select_density -- the parent's verb over the same keys and the same sort -- and beside the only way
there was before it, in one session:
    python tools/connect_probe.py [C4|R1] [--reps 20] [--n N] [--before 1] [--before-n 200000]
Medians [min .. max] of `reps` calls after one unmeasured call (which allocates), every call into a DEVICE mask (REPLACE, size = (1, 8),
no seed, no label or size arrays), from the verb's own clocks: gsr_get_select_connected ([0] the verb's kernels, [1] copies, [2] the
four-pass sort, [3] wall) and gsr_debug_select_connected_stages (keys, sort, cell table, link, flatten + stats, scatter + hit):
 (8)   a cell chosen so that the mean occupancy n_population / n_cells is about 8, taken from the density verb's own n_cells; reach 1, 2
 (x4)  a cell four times that size; reach 1, 2                                                    (C4 only)
 (d)   gsr_select_density, count = (1, 3), at the same cell and reach, in the same loop: the yardstick
 (s)   (8) reach 1 with a seed of 1000 random splats in device memory, op ADD, seed == mask (grow in place)
 (0)   the only way before: Engine.read of P and alpha, the breadth-first restatement of tests/connect_cases.py, the mask packed and
       copied back to the device -- over the first --before-n splats of the cloud where the whole of it is impractical
Each device mask, the labels, the sizes and every field of the result are compared with gsr_select_connected_eval over the whole
cloud (the rule on the host).  R1 is bench.py's capture-shaped scene with floaters (scenes.make_config("R1"))."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import __graft_entry__ as ge
import connect_cases as CC

pkg = ge.load_package()
E = pkg.engine
name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "C4"
opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
reps = int(opt("--reps", "20"))
before_reps = int(opt("--before", "1"))
before_n = int(opt("--before-n", "200000"))
n_over = opt("--n", None)
splats, cfg = pkg.scenes.make_config(name, int(n_over)) if n_over else pkg.scenes.make_config(name)
n = splats.n
words = (n + 31) // 32
cell_s = lambda v: "%.3f [%.3f .. %.3f]" % (np.median(v), np.min(v), np.max(v))
hip = C.CDLL("libamdhip64.so")
SIZE, COUNT = (1, 8), (1, 3)
STAGES = ("keys", "sort", "table", "link", "flatten+stats", "scatter+hit")


def device_room(nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
    return p


def fetch(ptr, count):
    out = np.empty(count, np.uint32)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), ptr, C.c_size_t(out.nbytes), 2) == 0
    return out


print("%s: %d splats, SH %s; median [min .. max] of %d calls, ms" % (name, n, splats.shx is not None, reps), flush=True)
with pkg.Engine(0) as eng:
    eng.upload(splats)
    dmask, dlab, dsiz = device_room(words * 4), device_room(n * 4), device_room(n * 4)
    finite = np.isfinite(splats.P).all(axis=1)
    lo, hi = splats.P[finite].min(axis=0), splats.P[finite].max(axis=0)
    extent = float((hi - lo).max())

    def occupancy(cell):
        origin, c = E.density_grid(lo, hi, cell)
        _, _, res = eng.select_density_device(E.density_rule(c, origin, reach=0, count=COUNT), dmask.value)
        return res.n_population / max(res.n_cells, 1)

    cell8 = max(extent / max(np.cbrt(n / 8.0), 1.0), extent / 1000.0)
    for step in range(6):
        occ = occupancy(cell8)
        if abs(occ - 8.0) < 0.4:
            break
        cell8 = max(cell8 * float(np.cbrt(8.0 / occ)), extent / 1000.0)
    print("cell of mean occupancy 8: %.6g (extent %.4g: %.0f cells across; occupancy %.2f after %d steps)" % (cell8, extent, extent / cell8, occ, step + 1), flush=True)

    rows = [("(8) ", cell8)] + ([("(x4)", 4.0 * cell8)] if name != "R1" else [])
    for label, cell in rows:
        origin, c = E.density_grid(lo, hi, cell)
        for reach in (1, 2):
            rule = E.connect_rule(c, origin, reach=reach, size=SIZE)
            drule = E.density_rule(c, origin, reach=reach, count=COUNT)
            ms, st, dms = [], [], []
            for r in range(reps + 1):
                n_hit, n_set, res = eng.select_connected_device(rule, dmask.value)
                if r:
                    ms.append(eng.get_select_connected()["ms"])
                    st.append(eng.select_connected_stages())
                eng.select_density_device(drule, dmask.value)
                if r:
                    dms.append(eng.get_select_density()["ms"])
            ms, st, dms = np.asarray(ms), np.asarray(st), np.asarray(dms)
            n_hit, n_set, res = eng.select_connected_device(rule, dmask.value, labels_ptr=dlab.value, sizes_ptr=dsiz.value)
            want = E.select_connected_eval(rule, splats.P, splats.alpha, labels=True, sizes=True, result=True)
            assert np.array_equal(fetch(dmask, words), E.pack_mask(want[0])) and np.array_equal(fetch(dlab, n), want[1]) and \
                np.array_equal(fetch(dsiz, n), want[2]) and want[3].fields() == res.fields(), label + ": the device result is not the host rule's"
            print("%s cell %.5g reach %d: wall %s   kernels %s   sort %s   copies %s | %s | cells %d components %d largest %d hits %d | (d) density wall %s  "
                  "kernels %s  sort %s" % (label, float(c), reach, cell_s(ms[:, 3]), cell_s(ms[:, 0]), cell_s(ms[:, 2]), cell_s(ms[:, 1]),
                                          "   ".join("%s %s" % (k, cell_s(st[:, i])) for i, k in enumerate(STAGES)), res.n_cells, res.n_components,
                                          res.largest, n_hit, cell_s(dms[:, 3]), cell_s(dms[:, 0]), cell_s(dms[:, 2])), flush=True)
            print("     splat_hist (population by floor(log2(size))): %s" % list(res.hists()[1][:24]), flush=True)

    # ---- (s) grow in place: seed == mask in device memory, op ADD
    origin, c = E.density_grid(lo, hi, cell8)
    picked = np.zeros(n, bool)
    picked[np.random.default_rng(1).permutation(n)[:1000]] = True
    pw = E.pack_mask(picked)
    grow = E.connect_rule(c, origin, reach=1, op=E.SELECT_ADD)
    ms = []
    for r in range(reps + 1):
        assert hip.hipMemcpy(dmask, C.c_void_p(pw.ctypes.data), C.c_size_t(pw.nbytes), 1) == 0
        n_hit, n_set, res = eng.select_connected_device(grow, dmask.value, seed_ptr=dmask.value)
        if r:
            ms.append(eng.get_select_connected()["ms"])
    ms = np.asarray(ms)
    want = E.select_connected_eval(grow, splats.P, splats.alpha, seed=picked)
    assert np.array_equal(fetch(dmask, words), E.pack_mask(want | picked)), "(s): the device result is not the host rule's"
    print("(s)  grow 1000 seeds in place, cell (8) reach 1: wall %s   kernels %s   seeded components %d   set afterwards %d"
          % (cell_s(ms[:, 3]), cell_s(ms[:, 0]), res.n_seeded, n_set), flush=True)

    # ---- (0) the only way before: P and alpha over the link, the restatement in numpy, the mask back
    m = min(n, before_n)
    rule = E.connect_rule(c, origin, reach=1, size=SIZE)
    read_ms, host_ms, back_ms = [], [], []
    for r in range(before_reps):
        t0 = time.perf_counter()
        R = eng.read(names=("P", "alpha"))
        t1 = time.perf_counter()
        sel = CC.restate(R.P[:m], R.alpha[:m], c, origin, reach=1, size=SIZE)[0]
        host_words = E.pack_mask(sel)
        t2 = time.perf_counter()
        assert hip.hipMemcpy(dmask, C.c_void_p(host_words.ctypes.data), C.c_size_t(host_words.nbytes), 1) == 0
        t3 = time.perf_counter()
        read_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3); back_ms.append((t3 - t2) * 1e3)
        assert np.array_equal(sel, E.select_connected_eval(rule, splats.P[:m], splats.alpha[:m])), "the restatement is not the host rule's"
    if before_reps:
        print("(0) before, cell (8) reach 1: Engine.read of P and alpha (all %d splats) %s   the restatement over the first %d splats + packing %s   "
              "mask to the device %s" % (n, cell_s(read_ms), m, cell_s(host_ms), cell_s(back_ms)), flush=True)
    for p in (dmask, dlab, dsiz):
        hip.hipFree(p)
