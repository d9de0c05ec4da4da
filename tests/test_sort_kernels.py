"""The inputs of tests/test_sort_kernels_gpu.py, checked without a GPU: every generator runs, the cases hold the shapes they are
made for, the ones that must succeed stay inside what the local sort can do, and the numpy reference agrees with a model that
needs no sorting routine at all."""
import numpy as np
import pytest

import sort_cases as sc


@pytest.fixture(scope="module")
def groups():
    return {name: make() for name, make in sc.all_groups().items()}


def _dict_model(case):
    """keys -> the payloads that carry them, in slot order; the local modes order each list by .x"""
    m = case.n_slots_dev // sc.BLOCK
    lists = {}
    for b in range(m):
        for t in range(int(case.cnt[b])):
            s = b * sc.BLOCK + t
            lists.setdefault(int(case.keys[s]), []).append((int(case.vals[s, 0]), int(case.vals[s, 1])))
    ks, vs = [], []
    for key in sorted(lists):
        pairs = sorted(lists[key], key=lambda p: p[0]) if case.mode in sc.LOCAL_MODES else lists[key]
        ks += [key] * len(pairs)
        vs += pairs
    return np.array(ks, np.uint32), np.array(vs, np.uint32).reshape(-1, 2)


def test_reference_agrees_with_a_dict_of_lists():
    g = sc.global_case(sc.GLOBAL, 4 * 256, 3 * 256, "random", 6, True, "third", seed=1, shuffle_x=True)
    rng = np.random.default_rng(2)
    cnt, item_keys, n_dev = sc.local_layout(rng, 4, 100, 16, {0: 40, 3: 65, 9: 17, 1023: 90}, extra_blocks=1)
    keys, vals = sc.lay_out(rng, cnt, item_keys, shuffle_x=True)
    loc = sc.Case("small-local", sc.LOCAL_DIRECT, keys, vals, cnt, n_dev, key_bits=16, lo=100, shift=4)
    for case in (g, loc):
        k, v = sc.reference(case)
        mk, mv = _dict_model(case)
        assert k.shape[0] > 100 and np.unique(k).shape[0] < k.shape[0]            # (ties are in play)
        assert np.array_equal(k, mk) and np.array_equal(v, mv)
    # the two tie rules differ on shuffled payloads: slot order is not .x order
    k, v = sc.reference(g)
    assert not np.array_equal(v, v[np.lexsort((v[:, 0], k))])
    # ORDERED: the counted blocks' heads as they are
    o = sc.ordered_cases()[0]
    k, v = sc.reference(o)
    assert np.array_equal(k, o.keys[: int(o.cnt[0])]) and np.array_equal(v, o.vals[: int(o.cnt[0])])


def test_every_case_is_well_formed(groups):
    names = set()
    for cases in groups.values():
        for c in cases:
            assert c.name not in names, c.name
            names.add(c.name)
            assert 0 < c.n_slots < 1_000_000 and c.n_slots % sc.BLOCK == 0
            assert 0 < c.n_slots_dev <= c.n_slots and c.n_slots_dev % sc.BLOCK == 0
            assert c.cnt.shape[0] == c.n_slots // sc.BLOCK and c.cnt.max() <= sc.BLOCK
            idx = sc.counted_slots(c.cnt, c.n_slots)
            item = np.zeros(c.n_slots, bool)
            item[idx] = True
            assert (c.keys[~item] == sc.GARBAGE).all()                             # what must never come out
            assert np.unique(c.vals[item, 0]).shape[0] == idx.shape[0]            # payload .x is unique
            assert (c.keys[item].astype(np.uint64) >> c.key_bits == 0).all()       # the keys fit the width that is sorted


def _shuffled(c):
    idx = sc.counted_slots(c.cnt, c.n_slots)
    x = c.vals[idx, 0]
    return bool((np.diff(x.astype(np.int64)) < 0).any())


def test_cases_that_must_succeed_meet_the_kernels_conditions(groups):
    for name, cases in groups.items():
        local = name.startswith("local")
        failing = [c.name for c in cases if c.expect_failed]
        assert len(failing) == (2 if local else 0), failing                        # exactly: a bucket of 8193, a run of 65
        for c in cases:
            if not local:
                continue
            largest, run = sc.conditions(c)
            if c.expect_failed:
                assert (largest == sc.BK_CAP + 1 and run <= sc.RL_MAX_RUN) or (run == sc.RL_MAX_RUN + 1 and largest <= sc.BK_CAP), c.name
            else:
                assert largest <= sc.BK_CAP and run <= sc.RL_MAX_RUN, (c.name, largest, run)


@pytest.mark.parametrize("mode", sc.LOCAL_MODES)
def test_local_cases_hold_the_named_populations_and_tie_runs(groups, mode):
    cases = [c for c in groups[sc.MODE_NAMES[mode]] if not c.expect_failed]
    passes = set()
    for shift in sc.SHIFTS:
        mine = [c for c in cases if c.shift == shift and "-shift" in c.name]
        seen, feats, bits = set(), set(), set()
        for c in mine:
            pops = sc.bucket_populations(c)
            for d, p in c.named.items():
                assert pops[d] == p, (c.name, d, p, int(pops[d]))                  # the named bucket holds exactly what it was built for
                seen.add(p)
            assert pops.sum() == sum(c.named.values())
            feats |= sc.tie_features(c)
            bits.add(c.key_bits)
            assert pops[0] > 0 or pops[sc.BUCKETS - 1] > 0                         # keys outside the range are in play
        assert seen >= set(sc.POPULATIONS), (shift, sorted(set(sc.POPULATIONS) - seen))
        assert feats >= {"run2", "run64", "start", "end", "straddle", "small"}, (shift, feats)
        assert "run65" not in feats
        passes.add((shift + 7) // 8)
        assert any(c.n_slots_dev < c.n_slots for c in mine)
    assert passes == {0, 1, 2, 3}
    assert {c.key_bits for c in cases} == {10, 24, 32}
    assert any(_shuffled(c) for c in cases)
    if mode == sc.LOCAL_K1:
        extra = [c for c in cases if "blocks4k" in c.name]
        assert {(c.n_slots_dev // sc.BLOCK) % 4 for c in extra} == {1, 2, 3}
        assert any(c.k1_grid == 1 for c in extra) and any(1 < c.k1_grid < -(-(c.n_slots // sc.BLOCK) // 4) for c in extra)
        assert any(c.range_dev for c in extra) and any(c.n_slots_dev < c.n_slots for c in extra)
    failing = {c.name.split("-", 1)[1]: c for c in groups[sc.MODE_NAMES[mode]] if c.expect_failed}
    assert sc.conditions(failing["bucket-8193"])[0] == sc.BK_CAP + 1 and "run65" in sc.tie_features(failing["run-65"])


@pytest.mark.parametrize("mode", (sc.GLOBAL, sc.GLOBAL_MID))
def test_global_cases_cover_sizes_fills_widths_and_duplicates(groups, mode):
    cases = groups[sc.MODE_NAMES[mode]]
    t = sc.TILE[mode]
    sizes = {(c.n_slots, c.n_slots_dev) for c in cases}
    assert sizes >= set(sc.global_sizes(mode)) and {(17 * t, 8 * t + 256), (17 * t, 256)} <= sizes
    combos = {tuple(c.name.split("-")[1:4]) for c in cases}
    assert combos >= {(str(n), str(d), f) for n, d in sc.global_sizes(mode) for f in sc.GLOBAL_FILLS}
    widths = {(c.key_bits, c.allow9, c.name.split("-")[5]) for c in cases}
    assert widths >= {(b, a, d) for b, a in sc.GLOBAL_BITS for d in sc.GLOBAL_DUPS}
    assert {(18, False), (27, False)} <= {(c.key_bits, c.allow9) for c in cases}
    assert sum(_shuffled(c) for c in cases) >= 3
    for c in cases:
        idx = sc.counted_slots(c.cnt, c.n_slots_dev)
        k = c.keys[idx]
        fill, dup = c.name.split("-")[3], c.name.split("-")[5]
        m = c.n_slots_dev // sc.BLOCK
        if fill == "empty":
            assert idx.size == 0
        if fill == "last_only":
            assert idx.size == 1 and c.cnt[m - 1] == 1
        if fill == "wave_00k" and m >= 3:
            assert (c.cnt[0], c.cnt[1]) == (0, 0) and c.cnt[2] > 0
        if dup == "two" and idx.size > 40:
            assert set(np.unique(k).tolist()) == {0, (1 << c.key_bits) - 1}        # at 32 bits: the kernels' own filler is a key
        if dup == "all_equal" and idx.size:
            assert np.unique(k).shape[0] == 1
        if dup == "third" and idx.size > 40:
            assert k.min() == 0 and k.max() == (1 << c.key_bits) - 1 and np.unique(k).shape[0] <= k.shape[0] - k.shape[0] // 3 + 2


def test_ordered_cases_cover_the_scan_loop(groups):
    cases = groups["ordered"]
    assert {c.n_slots_dev // sc.BLOCK for c in cases} == set(sc.ORDERED_BLOCKS)
    assert all(c.n_slots_dev < c.n_slots for c in cases)
    for m in sc.ORDERED_BLOCKS:
        sums = sorted(int(c.cnt[:m].astype(np.int64).sum()) for c in cases if c.n_slots_dev == m * sc.BLOCK)
        assert sums[0] == 0 and sums[-1] == m * sc.BLOCK and 0 < sums[1] < m * sc.BLOCK
