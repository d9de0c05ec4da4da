"""The depth horizons a frame leaves, their pyramid and the drop rule, held to the host model of tests/horizon_ref.py BIT FOR BIT.

The end-to-end culling tests (test_gpu_parity.py::test_occlusion_culling_is_exact, test_frame_constants_gpu.py) compare pixels, and a
broken horizon is REPAIRED: the frame is rendered again without culling and its pixels stay right.  A horizon that is too near costs a
repair, one that is too far culls less; neither turns a pixel test red.  Here every intermediate is read back after every frame and
compared with the model ("How the horizons are tested"):

  (a) the raw horizons k_tile_pass left, status sign included, on every tile of the whole image == raw_horizons(the frame's tile
      bookkeeping, super-tile lists, sort keys, the pyramid it was culled against, the plan's cull / cull_dilate, the shard).
      NOT for front-slab frames: phase 1's lists, which k_slab_mid formed the finished tiles' horizons from, are gone when the frame
      ends (and k_slab_mid's raw horizons are not modelled);
  (b) level 0, the status plane and levels 1..5 == dilate_and_pyramid(the raw horizons as read back, min(policy dilation, 3)): on
      EVERY frame, front-slab ones included;
  (c) a culled frame that was not repaired has no tile that broke its promise in the model, and no frame here is repaired at all: a
      repair, a camera "jump" or a frame that was not culled where the case says it is fails the case (there is no allowance);
  (d) culled frames without a depth buffer: an unculled twin context (both cull stages off) gives the visible set, rects and keys;
      the culled frame keeps EXACTLY visible & ~k1_drops(rect, key, the pyramid read before the frame, the plan's cull_dilate), its
      cluster list holds the cluster of every kept splat, and records, rects and pixels equal the twin's.

No key of any case is clamped by the frame's key range (asserted), so a list entry's sort key is the distance^2 k_tile_pass forms from
the position.  The cloud is test_culled_frames_against_finite_horizons's: 60 000 splats of opacity 0.97 seen from 2.2 units, whose
super-tile lists run to thousands of entries -- a tile that goes opaque inside its first 1024-entry step places its horizon 2304
entries down its list, so lists beyond about 2.3 k entries are what rule c2 needs (the 4112 x 40 frame sees a thin slice of the ball and
takes 160 000).  The last test asserts that, over the module, every rule of k_tile_pass, every level of the look-up and its walk over
the top level were taken: a case that tests nothing says so."""
import collections

import numpy as np
import pytest

import horizon_ref as HR

pytestmark = pytest.mark.gpu

ORIGIN = (0.25, -0.5, 0.125)
U32 = np.uint32


def _object_matrix():
    a, b = np.deg2rad(25.0), np.deg2rad(-40.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx @ np.diag([1.3, 0.8, 1.1])
    m[:3, 3] = (0.1, -0.05, 0.2)
    return m


OBJ = _object_matrix()
SMALL, MID, WIDE = (200, 120), (656, 304), (4112, 40)        # 13 x 8, 41 x 19 and 257 x 3 tiles

# name: size (or a list of sizes, one per frame), frame numbers of the 1-degree orbit (a repeated number = a static frame; a pair = at
# another distance than 2.2), options of both contexts, shard = (layout, index, count), depth-tested, splats, big splats, frames on
# which (d) is checked, the splats' opacity
Case = collections.namedtuple("Case", "size frames opts shard depth n bigs d_frames alpha", defaults=((), None, False, 60000, 0, (1, 2), 0.97))
CASES = {
    "13x8": Case(SMALL, (0, 0, 1)),
    "41x19": Case(MID, (0, 0, 1)),
    "257x3 wide, big splats": Case(WIDE, (0, 0, 1), n=160000, bigs=400),
    # (at dilation 0 a splat sits EXACTLY on the horizon it is compared with -- the entry the tile's horizon was taken from, where it
    #  touches that tile alone: the one place where `>` and `>=` in the drop rule differ)
    "dilate 0, static": Case(SMALL, (0, 0, 0), (("OPT_CULL_DILATE", 0),)),
    # the camera backs away: every key grows against the horizons left from nearer by, the lists are cut inside the 2304 entries a
    # tile wants for its next horizon, and the old horizon, pushed out, stands in
    "dolly out": Case(SMALL, (0, 0, (0, 2.3), (0, 2.36)), d_frames=(1, 2, 3)),
    "dolly out, dilate 0": Case(SMALL, (0, 0, (0, 2.23), (0, 2.26)), (("OPT_CULL_DILATE", 0),), d_frames=(1, 2, 3)),
    "dilate 1": Case(SMALL, (0, 0, 1), (("OPT_CULL_DILATE", 1),)),
    "dilate 3": Case(MID, (0, 0, 1), (("OPT_CULL_DILATE", 3),)),
    "dilate 5": Case(MID, (0, 0, 1), (("OPT_CULL_DILATE", 5),)),
    "super-tile 4": Case(MID, (0, 0, 1), (("OPT_SUPER_TILE", 4),)),
    "super-tile 8": Case(SMALL, (0, 0, 1), (("OPT_SUPER_TILE", 8),)),
    "swizzle 1": Case(SMALL, (0, 0, 1), (("OPT_XCD_SWIZZLE", 1),)),
    "swizzle 3": Case(MID, (0, 0, 1), (("OPT_XCD_SWIZZLE", 3),)),
    "rows 1 of 3, interleaved": Case(MID, (0, 0, 1), shard=(0, 1, 3)),
    "rows 1 of 3, bands": Case(MID, (0, 0, 1), shard=(1, 1, 3)),
    "depth-tested": Case(SMALL, (0, 0, 1), depth=True, d_frames=()),
    "front slab, then culled": Case(MID, (0, 0, 1), (("OPT_FRONT_SLAB", 2),)),
    "size change": Case([MID, SMALL, MID, MID], (0, 0, 0, 0), d_frames=(3,)),
    "41x19, big splats": Case(MID, (0, 0, 1), bigs=300),
    # faint splats: tiles go opaque thousands of entries down their lists, at depths that differ from tile to tile and move with the view
    "faint": Case(SMALL, (0, 0, 1, 2, 3), d_frames=(1, 2, 3, 4), alpha=0.1),
}

TALLY = {"branch": collections.Counter(), "level": collections.Counter(), "lookup": collections.Counter(), "cases": {}}
_CLOUDS = {}


def _cloud(pkg, n, bigs, alpha):
    if (n, bigs, alpha) not in _CLOUDS:
        s = pkg.scenes.make_scene(n, seed=79, sh=True, log_scale_range=(-3.0, -2.2))
        s.alpha[:] = alpha
        if bigs:     # faint splats of every size up to the whole frame, anywhere in the ball: their look-ups are spread over the levels
            rng = np.random.default_rng(80)
            idx = rng.choice(n, bigs, replace=False)
            size = np.exp(rng.uniform(np.log(0.02), np.log(1.2), bigs))
            s.scale[idx] = pkg.scenes.f16bits(np.repeat(size[:, None], 3, axis=1))
            s.alpha[idx] = 0.05
        _CLOUDS[(n, bigs, alpha)] = s
    return _CLOUDS[(n, bigs, alpha)]


def _camera(pkg, size, frame):
    """frame: the step of the 1-degree orbit at 2.2 units, or (step, distance)"""
    kw = dict(p00=0.6) if size == WIDE else {}
    frame, distance = frame if isinstance(frame, tuple) else (frame, 2.2)
    return pkg.camera.make_camera(size[0], size[1], sh_order=3, frame=180 + frame, object_matrix=OBJ, step_deg=1.0, distance=distance, **kw)


def _context(pkg, splats, case, culling):
    E = pkg.engine
    eng = pkg.Engine(0)
    eng.upload(splats, origin=ORIGIN)
    eng.set_option(E.OPT_LAZY_COLOUR, 0)
    eng.set_option(E.OPT_SORT_CACHE, 0)                      # (a static frame is rendered like any other, in both contexts)
    eng.set_option(E.OPT_FRONT_SLAB, 0)
    for name, v in case.opts:
        if culling or name not in ("OPT_FRONT_SLAB", "OPT_CULL_DILATE"):
            eng.set_option(getattr(E, name), v)
    eng.set_option(E.OPT_OCCLUSION_CULL, 2 if culling else 0)
    eng.set_option(E.OPT_CLUSTER_CULL, 1 if culling else 0)
    if case.shard:
        eng.set_option(E.OPT_SHARD_LAYOUT, case.shard[0])
        eng.set_row_shard(case.shard[1], case.shard[2])
    return eng


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def _frame(eng, cam, depth, prev, n, tally, what):
    """render one frame, read everything back, assert (a)-(c); -> what the next frame is culled against, and this frame's outcome"""
    s0 = eng.stats()
    img = eng.render(cam) if depth is None else eng.render_depth(cam, depth)
    s1, plan, pol = eng.stats(), eng.debug_last_plan(), eng.policy_state()
    levels, meta = eng.debug_horizon_pyramid()
    tx, ty = meta["tiles_x"], meta["tiles_y"]
    assert (tx, ty) == ((cam.width + 15) // 16, (cam.height + 15) // 16) and meta["horizon_valid"] == 1
    assert meta["pyr_off"] == HR.pyr_offsets(tx, ty) and meta["rect_shift"] == (1 if max(tx, ty) > 256 else 0)
    hz = eng.debug_horizons(tx, ty)
    grew = {k: s1[k] - s0[k] for k in ("frames_culled", "frames_repaired", "frames_jumped", "frames_slab")}
    assert grew["frames_repaired"] == 0 and grew["frames_jumped"] == 0 and not plan["jumped"], f"{what}: repaired or jumped, the case tests nothing: {grew}"
    assert bool(plan["cull"]) == bool(meta["culled"]) == (grew["frames_culled"] == 1), (what, plan, grew)
    # (b) the dilation and the pyramid, from the raw horizons as read back
    assert meta["hpyr_re"] == min(pol["cull_dilate"], HR.DILATE_EXACT_MAX), (what, meta["hpyr_re"], pol)
    m_levels, m_stat = HR.dilate_and_pyramid(hz[1], meta["hpyr_re"], meta["pyr_off"])
    assert _same_bits(hz[0], levels[0]), f"{what}: the two doors disagree about level 0"
    for l in range(HR.PYR_LEVELS):
        bad = np.argwhere(levels[l].view(U32) != m_levels[l].view(U32))
        assert levels[l].shape == m_levels[l].shape and not len(bad), f"{what}: (b) level {l}: {len(bad)} cells differ, first {bad[:4].tolist()}"
    bad = np.argwhere(hz[2] != m_stat)
    assert not len(bad), f"{what}: (b) the status plane: {len(bad)} tiles differ, first {bad[:4].tolist()}"
    out = dict(levels=levels, meta=meta, stat=hz[2].copy(), raw=hz[1].copy(), plan=plan, img=img, grew=grew, branch=None)
    if plan["phase"] != 0:
        return out
    # (a) the raw horizons, (c) the promises
    shard = HR.Shard(meta["shard_index"], meta["shard_count"], meta["shard_rpb"], meta["shard_first"])
    tw = eng.debug_tile_work()
    assert tw.shape[:2] == (meta["local_tiles_y"], tx)
    ts, te, pv = eng.debug_tile_lists()
    rec = eng.debug_records(n)
    vis = rec["visible"] == 1
    assert vis[pv].all(), "a list entry of a splat that left no record"
    kb = rec["key"][vis].view(U32)
    assert (kb > meta["key_min"]).all() and (kb < meta["key_max"]).all(), f"{what}: a sort key is clamped by the frame's key range"
    assert not plan["cull"] or (prev is not None and prev["levels"][0].shape == (ty, tx))
    m_raw, broke, branch = HR.raw_horizons(
        tw, ts, te, rec["key"][pv], ty, shard, meta["super_shift"], meta["stiles_x"], meta["list_cap"],
        pyr_in=prev["levels"] if plan["cull"] else None, cull=bool(plan["cull"]), cull_dilate=plan["cull_dilate"],
        stat_in=prev["stat"] if (prev is not None and prev["stat"].shape == (ty, tx)) else None, stat_in_use=bool(meta["stat_in_use"]),
        depth_culled=bool(meta["depth_culled"]))
    bad = np.argwhere(m_raw.view(U32) != hz[1].view(U32))
    detail = [(y, x, HR.BRANCH_NAMES[branch[y, x]], float(hz[1][y, x]), float(m_raw[y, x])) for y, x in bad[:4].tolist()]
    assert not len(bad), f"{what}: (a) {len(bad)} raw horizons differ; (row, column, rule, device, model): {detail}"
    if plan["cull"]:
        assert not broke.any(), f"{what}: (c) the frame was not repaired, but tiles {np.argwhere(broke)[:4].tolist()} broke their promise in the model"
    tally["branch"].update(HR.BRANCH_NAMES[b] for b in branch.ravel().tolist())
    out["branch"] = collections.Counter(HR.BRANCH_NAMES[b] for b in branch.ravel().tolist())
    out["finite"] = int((np.abs(hz[1]) < HR.NO_HORIZON).sum())
    return out


def _check_drops(dut, plain, cam, prev, obs, n, cluster_of, tally, what):
    """(d): the culled frame `obs` of `dut` keeps exactly what the model says, given the unculled twin's frame"""
    img0 = plain.render(cam)
    rect0, _ = plain.debug_cull(n)
    rec0 = plain.debug_records(n)
    vis0 = rec0["visible"] == 1
    assert np.array_equal(vis0, rect0 != 0xffffffff)
    meta = obs["meta"]
    kb = rec0["key"][vis0].view(U32)
    assert (kb > meta["key_min"]).all() and (kb < meta["key_max"]).all(), f"{what}: a sort key is clamped by the frame's key range"
    assert obs["plan"]["cull"] and obs["plan"]["phase"] == 0, f"{what}: the frame was not culled, the case tests nothing"
    drop, level, lookup = HR.k1_drops(rect0[vis0], rec0["key"][vis0], prev["levels"], meta, obs["plan"]["cull_dilate"])
    assert 0 < int(drop.sum()) < drop.size, f"{what}: the model drops {int(drop.sum())} of {drop.size} splats, the case tests nothing"
    expect = vis0.copy()
    expect[np.flatnonzero(vis0)[drop]] = False
    rec = dut.debug_records(n)
    rect, clus = dut.debug_cull(n)
    kept = rec["visible"] == 1
    extra, missing = np.flatnonzero(kept & ~expect), np.flatnonzero(expect & ~kept)
    assert not len(extra) and not len(missing), (f"{what}: (d) the frame keeps {len(extra)} splats the rule drops (first {extra[:4].tolist()}) and drops "
                                                 f"{len(missing)} it keeps (first {missing[:4].tolist()})")
    assert np.array_equal(kept, rect != 0xffffffff)
    assert set(cluster_of[kept].tolist()) <= set(clus.tolist()), f"{what}: (d) a kept splat outside the surviving clusters"
    assert np.array_equal(rec[kept], rec0[kept]) and np.array_equal(rect[kept], rect0[kept])
    assert np.array_equal(obs["img"], img0, equal_nan=True), f"{what}: the culled frame's pixels differ from the unculled twin's"
    tally["level"].update(level[lookup == HR.LK_CORNERS].tolist())
    tally["lookup"].update(("2 x 2 corners", "4 x 4 walk", "+inf")[k] for k in lookup.tolist())
    return int(kept.sum()), int(drop.sum()), int(vis0.sum())


_DONE = {}


def _run_case(pkg, name):
    if name in _DONE:
        return _DONE[name]
    case = CASES[name]
    tally = {"branch": collections.Counter(), "level": collections.Counter(), "lookup": collections.Counter()}
    splats = _cloud(pkg, case.n, case.bigs, case.alpha)
    n = splats.n
    sizes = case.size if isinstance(case.size, list) else [case.size] * len(case.frames)
    lines = []
    dut, plain = _context(pkg, splats, case, True), None
    try:
        plain = _context(pkg, splats, case, False)
        order = dut.debug_storage_order(n)
        cluster_of = np.empty(n, np.int64)
        cluster_of[order] = np.arange(n) // 64
        depth = pkg.scenes.sphere_occluder_depth(_camera(pkg, sizes[0], 0), 2.2, 0.45) if case.depth else None
        if depth is not None:
            assert 0.02 < (depth < 1.0).mean() < 0.9, "the depth buffer holds geometry, and not everywhere"
        prev = None
        for k, (size, frame) in enumerate(zip(sizes, case.frames)):
            cam = _camera(pkg, size, frame)
            what = f"{name}, frame {k}"
            obs = _frame(dut, cam, depth, prev, n, tally, what)
            assert obs["img"][..., 3].max() > 0.5, "an empty frame checks nothing"
            line = f"{what} ({size[0]} x {size[1]}): cull {obs['plan']['cull']} phase {obs['plan']['phase']} look-up dilate {obs['plan']['cull_dilate']} " \
                   f"built-in {obs['meta']['hpyr_re']}"
            if obs["branch"] is not None:
                line += f", finite raw horizons on {obs['finite']} of {obs['raw'].size} tiles, rules {dict(obs['branch'])}"
            if k in case.d_frames:
                kept, dropped, vis0 = _check_drops(dut, plain, cam, prev, obs, n, cluster_of, tally, what)
                line += f"; kept {kept} of {vis0} visible, dropped {dropped}"
            elif k > 0 and not case.d_frames:
                assert obs["plan"]["cull"], f"{what}: the frame was not culled, the case tests nothing"
            lines.append(line)
            prev = obs
        if name == "front slab, then culled":
            assert lines and "phase 2" in lines[0], "the first frame was no front-slab frame: the case tests nothing"
    finally:
        dut.close()
        if plain is not None:
            plain.close()
        for line in lines:
            print(line)
    print(f"{name}: look-up levels {dict(sorted(tally['level'].items()))}, paths {dict(tally['lookup'])}")
    for k in ("branch", "level", "lookup"):
        TALLY[k].update(tally[k])
    TALLY["cases"][name] = tally
    _DONE[name] = True
    return True


@pytest.mark.parametrize("name", list(CASES))
def test_horizons_pyramid_and_drops_match_the_model(pkg, name):
    _run_case(pkg, name)


def test_every_rule_level_and_path_was_taken(pkg):
    """over the module: each rule of k_tile_pass on at least one tile, each level of gsr_pyr_max and its top-level walk by at least one
    splat of (d); rows of another rank read 0, never +inf"""
    for name in CASES:
        _run_case(pkg, name)
    print("rules over the module:", dict(TALLY["branch"]))
    print("look-up levels over the module:", dict(sorted(TALLY["level"].items())), "paths:", dict(TALLY["lookup"]))
    for rule in ("c2", "hold x 1.05", "c3", "none", "open", "other-rank"):
        assert TALLY["branch"][rule] > 0, f"no tile took the rule '{rule}': the cases test nothing of it"
    for level in range(HR.PYR_LEVELS):
        assert TALLY["level"][level] > 0, f"no splat was looked up at level {level}: the cases test nothing of it"
    assert TALLY["lookup"]["4 x 4 walk"] > 0, "no splat took the walk over the top level: the cases test nothing of it"
    for name in ("rows 1 of 3, interleaved", "rows 1 of 3, bands"):
        assert TALLY["cases"][name]["branch"]["other-rank"] > 0, f"{name}: no tile of another rank"
