"""The depth sort's kernels (csrc/k_sort.h) in the instantiations a FRAME launches, against numpy, bit for bit.

Engine.debug_sort_frame runs the frame's own host functions (radix_sort<uint2> with its compacting first pass, launch_local_sort,
launch_ordered_compact) on the cases of tests/sort_cases.py: K1's block-compacted layout with garbage behind every block's items,
uint2 payloads whose .y must travel with its .x, a slot count the kernels read from device memory, a live `failed` word.  The
reference is three lines of numpy (sort_cases.reference); the two tie rules are pinned apart by shuffled payloads: equal keys
leave the global passes in SLOT order and the local kernel in payload .x order.

The second half renders frames that take each production plan -- proved by the plan the slot kept (Engine.debug_last_plan) -- and
compares their depth ORDER, not their pixels, with the oracle's host sort.

354 sort calls, each below 800 k slots; the file takes 1.5 s on one MI355X (LAB_NOTES.md, "Sort kernels against numpy").
"""
import os

import numpy as np
import pytest

import sort_cases as sc

pytestmark = pytest.mark.gpu

_GROUPS = {}


def _cases(group):
    if group not in _GROUPS:
        _GROUPS[group] = sc.all_groups()[group]()
    return _GROUPS[group]


def _check(pkg, engine, case):
    base = pkg.engine.live_handles()
    k, v, failed = engine.debug_sort_frame(case.mode, case.keys, case.vals, case.cnt, **case.call_args())
    assert pkg.engine.live_handles() == base, f"{case.name}: the call left handles behind"
    if case.expect_failed:
        assert failed != 0, f"{case.name}: the local sort must give this input up"
        return
    if case.mode in sc.LOCAL_MODES:
        largest, run = sc.conditions(case)
        assert largest <= sc.BK_CAP and run <= sc.RL_MAX_RUN, (case.name, largest, run)
    assert failed == 0, f"{case.name}: spurious `failed`"
    rk, rv = sc.reference(case)
    assert k.shape[0] == rk.shape[0], f"{case.name}: kept {k.shape[0]}, the counted blocks hold {rk.shape[0]}"
    bad = np.flatnonzero(k != rk)
    assert bad.size == 0, f"{case.name}: {bad.size} keys differ, first at {bad[0]}: {k[bad[0]]:#x} for {rk[bad[0]]:#x}"
    bad = np.flatnonzero(v[:, 0] != rv[:, 0])
    assert bad.size == 0, f"{case.name}: {bad.size} payloads out of order, first at {bad[0]} (key {rk[bad[0]]:#x})"
    assert np.array_equal(v[:, 1], rv[:, 1]), f"{case.name}: a payload's .y left its .x"


def _parts(group, parts):
    return [pytest.param(group, i, parts, id=f"{group}-{i}") for i in range(parts)]


@pytest.mark.parametrize("group,part,parts", _parts("global", 4) + _parts("global_mid", 4) + _parts("local_gather", 2) + _parts("local_k1", 2) +
                         _parts("local_direct", 2) + _parts("ordered", 2))
def test_frame_sort_matches_numpy(pkg, engine, group, part, parts):
    cases = _cases(group)[part::parts]
    assert cases
    for case in cases:
        _check(pkg, engine, case)


def test_every_mode_ran_its_own_cases(pkg):
    """the groups name the hook's six modes, and the test above takes every case of every group"""
    E = pkg.engine
    want = {"global": E.SORT_GLOBAL, "global_mid": E.SORT_GLOBAL_MID, "local_gather": E.SORT_LOCAL_GATHER, "local_k1": E.SORT_LOCAL_K1,
            "local_direct": E.SORT_LOCAL_DIRECT, "ordered": E.SORT_ORDERED}
    assert set(sc.all_groups()) == set(want)
    for group, mode in want.items():
        assert {c.mode for c in _cases(group)} == {mode}
    assert (sc.GLOBAL, sc.GLOBAL_MID, sc.LOCAL_GATHER, sc.LOCAL_K1, sc.LOCAL_DIRECT, sc.ORDERED) == tuple(want.values())


def test_bad_arguments_are_refused(pkg, engine):
    E = pkg.engine
    keys, vals, cnt = np.zeros(512, np.uint32), np.zeros((512, 2), np.uint32), np.array([3, 4], np.uint32)
    base = E.live_handles()

    def refused(**kw):
        a = dict(mode=E.SORT_GLOBAL, keys=keys, vals=vals, blk_cnt=cnt)
        a.update(kw)
        with pytest.raises(pkg.GsrError) as e:
            engine.debug_sort_frame(**a)
        assert e.value.code == -1                                                  # GSR_E_INVALID
        assert E.live_handles() == base

    refused(keys=keys[:0], vals=vals[:0], blk_cnt=cnt[:0])                         # n_slots == 0
    refused(keys=keys[:255], vals=vals[:255], blk_cnt=cnt[:1])                     # no multiple of 256
    refused(keys=keys[:300], vals=vals[:300])
    refused(n_slots_dev=100)
    refused(n_slots_dev=768)                                                       # beyond the host's bound
    refused(blk_cnt=np.array([3, 257], np.uint32))                                 # more items than a block has slots
    refused(mode=6)
    refused(key_bits=0)
    refused(key_bits=33)
    refused(mode=E.SORT_LOCAL_DIRECT, shift=32)
    refused(mode=E.SORT_LOCAL_DIRECT, range_dev=True)                              # only the per-wave scatter reads a range on the device
    refused(mode=E.SORT_LOCAL_K1, k1_grid=0)
    k, v, failed = engine.debug_sort_frame(E.SORT_GLOBAL, keys, vals, cnt, n_slots_dev=0)    # nothing counts: nothing comes back
    assert k.shape[0] == 0 and failed == 0


# ---------------------------------------------------------------------------------------------
# the production plans end to end, by order
N_SPLATS = 70001


@pytest.fixture(scope="module")
def tied_scene(pkg):
    splats = pkg.scenes.make_scene(N_SPLATS, seed=5, sh=False)
    splats.P[1000:1100] = splats.P[2000:2100]      # exact ties -> storage order
    return splats


@pytest.fixture(scope="module")
def order_ref(oracle, tied_scene):
    """oracle.host_sort_only per camera position, computed once"""
    memo = {}

    def ref(cam):
        key = cam.cam_pos.tobytes()
        if key not in memo:
            memo[key] = oracle.host_sort_only(tied_scene.P, cam.cam_pos)
        return memo[key]
    return ref


def _engine_under(pkg, env):
    """a context made under A/B hooks of the environment (they are read when a context is created), the environment put back"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Engine(0)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


PLANS = {
    # name: (environment, options, second camera turns in place?, the plan flags the second frame must show)
    "mid_global": ({}, {"OPT_LOCAL_SORT": 0}, False, dict(local=0, ordered=0, cache_hit=0, mid_sort=1)),
    "local_k1_scatters": ({}, {"OPT_LOCAL_SORT": 2}, False, dict(local=1, ordered=0, cache_hit=0, k1_scatters=1)),
    "local_direct": ({"GSR_K1_SCATTER": "0", "GSR_SCATTER_DIRECT": "2"}, {"OPT_LOCAL_SORT": 2}, False,
                     dict(local=1, ordered=0, cache_hit=0, k1_scatters=0, scatter_direct=1)),
    "local_per_wave": ({"GSR_K1_SCATTER": "0", "GSR_SCATTER_DIRECT": "0"}, {"OPT_LOCAL_SORT": 2}, False,
                       dict(local=1, ordered=0, cache_hit=0, k1_scatters=0, scatter_direct=0)),
    "local_gather": ({"GSR_K1_SCATTER": "0", "GSR_SCATTER_DIRECT": "-1"}, {"OPT_LOCAL_SORT": 2}, False,
                     dict(local=1, ordered=0, cache_hit=0, k1_scatters=0, scatter_direct=0)),
    "ordered": ({}, {"OPT_SORT_CACHE": 2}, True, dict(local=0, ordered=1, cache_hit=0)),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_depth_order_of_every_sort_plan_matches_oracle(pkg, oracle, tied_scene, order_ref, plan):
    """the second frame of a context takes the plan (its slot's first frame left the hints the plan is chosen from); its depth order
    is the oracle's (distance^2, storage position) order restricted to the splats it kept.  No occlusion culling: the plans differ in
    the sort alone, and the sort sees every splat in the frustum"""
    env, options, turn, flags = PLANS[plan]
    E = pkg.engine
    n = tied_scene.n
    cam1 = pkg.camera.make_camera(256, 256, sh_order=0, frame=9)
    cam2 = pkg.camera.rotated_in_place(cam1, 1.0) if turn else pkg.camera.make_camera(256, 256, sh_order=0, frame=10)
    eng = _engine_under(pkg, env)
    try:
        eng.set_option(E.OPT_FRAMES_IN_FLIGHT, 1)                                  # (one slot: the second frame reads the first one's hints)
        eng.set_option(E.OPT_OCCLUSION_CULL, 0)
        for name, value in options.items():
            eng.set_option(getattr(E, name), value)
        eng.upload(tied_scene)
        eng.render(cam1)
        first = eng.debug_last_plan()
        assert first["local"] == 0 and first["ordered"] == 0 and first["mid_sort"] == 0 and first["phase"] == 0   # (the 12-item global sort)
        eng.render(cam2)
        p = eng.debug_last_plan()
        dev = eng.debug_depth_order(n)
        st = eng.stats()
        order0 = eng.debug_storage_order(n)
    finally:
        eng.close()
    print(f"{plan}: kept {dev.shape[0]} of {n}, plan {p}")
    for name, value in flags.items():
        assert p[name] == value, f"{plan}: the frame's plan has {name} = {p[name]}"
    assert p["phase"] == 0 and p["cull"] == 0 and p["n_slots"] == -(-(-(-n // 64)) // 4) * 256 and 10 <= p["key_bits"] <= 32
    assert st["frames_resorted"] == 0                                              # (no local sort gave up and hid behind the global one)
    assert np.array_equal(order0, oracle.storage_order(tied_scene.P))
    ref = order_ref(cam2)
    assert dev.shape[0] > 0.8 * n
    keep = np.zeros(n, bool)
    keep[dev] = True
    assert keep.sum() == dev.shape[0]                                              # no splat twice
    assert np.array_equal(dev, ref[keep[ref]])
    assert keep[1000:1100].sum() > 70 and keep[2000:2100].sum() > 70               # the exact ties are in play
