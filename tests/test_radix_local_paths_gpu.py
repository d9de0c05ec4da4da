"""k_radix_local (csrc/k_sort.h) at every boundary between its paths, through Engine.debug_sort_frame, against numpy bit for bit.

The kernel requests its bucket's count, the first RL_SPEC_ROWS * 256 slots of its region and the counts of the buckets before it in
one trip, and then takes one of four paths: up to 64 keys are ranked by counting; up to RL_CHUNK (2048) keys are distributed over
1024 sub-bins on the top ten of the bits the bucket sorts on and ranked inside their sub-bin; a bucket with a sub-bin beyond
RL_SUB_MAX (= RL_MAX_RUN, 64) items falls back to the LSD passes and the tie pass; beyond RL_CHUNK keys the passes go through
global memory.  The cases here sit on those edges: populations around 64, 256 (a row of the workgroup), 512 (the rows requested
ahead of the count) and 2048, in middle buckets and in the first and the last one (which sort on all key bits); bucket widths
with fewer sub-bins than 1024, the width a culled C4 frame was found to use (2^14), one above it and 2^22; sub-bins at the bound
and one beyond; tie runs of RL_MAX_RUN (must succeed) and RL_MAX_RUN + 1 (must raise `failed`); an empty last bucket; and regions
whose slots behind the count hold keys of an earlier, larger sort that WOULD belong to the bucket.

Every case is checked on the CPU where it is built (sort_cases.conditions: largest bucket <= BK_CAP, longest run <= RL_MAX_RUN
unless it is meant to fail; the named buckets hold what they were built to hold).  123 sort calls of at most 30 k slots.
"""
import numpy as np
import pytest

import sort_cases as sc

POPS = (0, 1, 63, 64, 65, 66, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049)
C4_SHIFT = 14                      # bk_shift of culled C4 frames (Engine.debug_last_plan; LAB_NOTES.md, "Small-frame sort: one trip, one pass")
SHIFTS = (0, 1, 9, C4_SHIFT, C4_SHIFT + 1, 22)
SUB_BINS = 1024                    # RL_SUB_BINS
SUB_MAX = sc.RL_MAX_RUN            # RL_SUB_MAX
FIRST, LAST = 0, sc.BUCKETS - 1
MODES = [pytest.param(m, id=sc.MODE_NAMES[m]) for m in sc.LOCAL_MODES]


def _range_of(shift):
    """(lo, key_bits) of the calls at one bucket width: the last bucket is never empty of key values"""
    if shift >= 22:
        return 4099, 32
    if shift >= 9:
        return 5000, 25            # (the key width of C4: lo + 1023 << 15 is still below 2^25)
    return 3000, 32


def _validate(case):
    largest, run = sc.conditions(case)
    assert largest <= sc.BK_CAP, (case.name, largest)
    assert (run > sc.RL_MAX_RUN) == case.expect_failed, (case.name, run)
    pops = sc.bucket_populations(case)
    for d, p in case.named.items():
        assert pops[d] == p, (case.name, d, int(pops[d]), p)
    assert int(pops.sum()) == sum(case.named.values()), case.name
    return case


def _named_case(name, mode, seed, shift, named, shuffle_x=False):
    lo, key_bits = _range_of(shift)
    rng = np.random.default_rng(seed)
    cnt, item_keys, n_dev = sc.local_layout(rng, shift, lo, key_bits, named, extra_blocks=2)
    keys, vals = sc.lay_out(rng, cnt, item_keys, shuffle_x=shuffle_x)
    return _validate(sc.Case(name, mode, keys, vals, cnt, n_dev, key_bits=key_bits, lo=lo, shift=shift, named=dict(named)))


def _keys_case(name, mode, seed, shift, buckets, shuffle_x=False, expect_failed=False):
    """buckets: bucket -> its keys (any order), written out by the caller"""
    lo, key_bits = _range_of(shift)
    rng = np.random.default_rng(seed)
    item_keys = rng.permutation(np.concatenate([np.asarray(k, np.int64) for k in buckets.values()])).astype(np.uint32)
    m = max(1, -(-item_keys.shape[0] // 160))
    cnt = sc.random_counts(rng, m, item_keys.shape[0])
    keys, vals = sc.lay_out(rng, cnt, item_keys, shuffle_x=shuffle_x)
    return _validate(sc.Case(name, mode, keys, vals, cnt, m * sc.BLOCK, key_bits=key_bits, lo=lo, shift=shift, expect_failed=expect_failed,
                             named={d: len(k) for d, k in buckets.items()}))


def population_cases(mode):
    """every population in a middle bucket, in the first and in the last bucket, at C4's bucket width: fifteen calls, the first
    bucket walking up POPS while the last one walks down (so either end is empty once, with keys elsewhere)"""
    out = []
    for j, p in enumerate(POPS):
        named = {3 + 7 * i: q for i, q in enumerate(POPS[j::5])}          # (a few middle buckets; all of POPS over the calls)
        named[17 + 11 * j] = p
        named[FIRST], named[LAST] = p, POPS[len(POPS) - 1 - j]
        out.append(_named_case(f"pops-{j}", mode, 7100 + 20 * mode + j, C4_SHIFT, named, shuffle_x=(j % 3 == 1)))
    return out


def width_cases(mode):
    """every population at every bucket width.  A middle bucket is 2^shift keys wide and no key may come more than RL_MAX_RUN times:
    at 2^0 and 2^1 the populations beyond that live in the first and the last bucket"""
    out = []
    seed = 7300 + 100 * mode
    for shift in SHIFTS:
        if shift >= 9:
            named = {3 + 7 * i: p for i, p in enumerate(POPS)}
            named[FIRST], named[LAST] = 300, 1200
            seed += 1
            out.append(_named_case(f"width-{shift}", mode, seed, shift, named, shuffle_x=(shift == 9)))
            continue
        cap = sc.RL_MAX_RUN << shift
        small, big = [p for p in POPS if p <= cap], [p for p in POPS if p > cap]
        for i in range(0, len(big), 2):
            named = {5 + 11 * j: p for j, p in enumerate(small)}
            named[LAST] = big[i]
            if i + 1 < len(big):
                named[FIRST] = big[i + 1]
            seed += 1
            out.append(_named_case(f"width-{shift}-{i // 2}", mode, seed, shift, named, shuffle_x=(i == 2)))
    return out


def _spread(rng, base, sub_width, first_sub, count):
    """count keys, one per sub-bin from first_sub on"""
    assert first_sub + count <= SUB_BINS
    return base + (first_sub + np.arange(count, dtype=np.int64)) * sub_width + rng.integers(0, sub_width, count)


def subbin_cases(mode):
    """300 distinct keys in ONE sub-bin (the fallback: correct, and never `failed`); a sub-bin of exactly RL_SUB_MAX distinct keys and
    one of RL_SUB_MAX + 1 among keys that are spread one per sub-bin.  Width 2^22: a sub-bin is 4096 keys wide"""
    shift = 22
    lo, _ = _range_of(shift)
    sub_width = (1 << shift) // SUB_BINS
    rng = np.random.default_rng(7500 + mode)
    base = lambda d: lo + (d << shift)
    one = {40: base(40) + 7 * sub_width + rng.choice(sub_width, 300, replace=False),
           41: _spread(rng, base(41), sub_width, 0, 300)}
    out = [_keys_case("one-sub-bin", mode, 7510 + mode, shift, one, shuffle_x=True)]
    for extra in (0, 1):
        filled = lambda d: np.concatenate([base(d) + 5 * sub_width + rng.choice(sub_width, SUB_MAX + extra, replace=False),
                                           _spread(rng, base(d), sub_width, 10, 336)])
        last_sub = np.concatenate([base(91) + (SUB_BINS - 1) * sub_width + rng.choice(sub_width, SUB_MAX + extra, replace=False),
                                   _spread(rng, base(91), sub_width, 0, 700)])      # (the sub-bin whose end is the bucket's count)
        out.append(_keys_case(f"sub-bin-{SUB_MAX + extra}", mode, 7520 + 10 * extra + mode, shift, {90: filled(90), 91: last_sub, 300: filled(300)}))
    return out


def tie_cases(mode):
    """a run of exactly RL_MAX_RUN equal keys in buckets of 65, 300 and 512 keys must be ordered by payload .x (shuffled); one key
    more and the call must raise `failed`.  C4's width: a sub-bin is 16 keys wide, the other keys sit one per sub-bin"""
    shift = C4_SHIFT
    lo, _ = _range_of(shift)
    sub_width = (1 << shift) // SUB_BINS
    out = []
    for run in (sc.RL_MAX_RUN, sc.RL_MAX_RUN + 1):
        for pop in (65, 300, 512):
            rng = np.random.default_rng(7600 + 10 * mode + pop + run)
            d = 200 + pop
            base = lo + (d << shift)
            bucket = np.concatenate([np.full(run, base + 3, np.int64), _spread(rng, base, sub_width, 1, pop - run)])
            other = _spread(rng, lo + (77 << shift), sub_width, 0, 100)
            out.append(_keys_case(f"run-{run}-in-{pop}", mode, 7700 + mode + pop + run, shift, {d: bucket, 77: other}, shuffle_x=True,
                                  expect_failed=run > sc.RL_MAX_RUN))
    return out


def garbage_cases(mode):
    """two calls over the same buckets at the same range: the first fills them beyond RL_CHUNK, the second leaves a few keys at their
    heads -- behind the count lie keys of the first call, all of which would sort into the bucket"""
    buckets = (FIRST, 9, 100, 511, 512, 800, 1022, LAST)
    big = _named_case("garbage-fill", mode, 7800 + mode, C4_SHIFT, {d: 2049 + 10 * i for i, d in enumerate(buckets)})
    small = _named_case("garbage-heads", mode, 7810 + mode, C4_SHIFT, dict(zip(buckets, (1, 63, 65, 300, 511, 513, 64, 0))))
    return [big, small]


GROUPS = {"populations": population_cases, "widths": width_cases, "sub_bins": subbin_cases, "ties": tie_cases, "garbage": garbage_cases}
_BUILT = {}


def _cases(group, mode):
    if (group, mode) not in _BUILT:
        _BUILT[group, mode] = GROUPS[group](mode)
    return _BUILT[group, mode]


def test_cases_hold_what_they_promise():
    """no GPU: every case builds (its conditions are asserted where it is built), and together they cover what the header lists"""
    for mode in sc.LOCAL_MODES:
        cases = [c for g in GROUPS for c in _cases(g, mode)]
        assert all(c.mode == mode for c in cases) and len({c.name for c in cases}) == len(cases)
        at = {where: set() for where in ("first", "middle", "last")}
        for c in _cases("populations", mode):
            for d, p in c.named.items():
                at["first" if d == FIRST else "last" if d == LAST else "middle"].add(p)
        assert all(v == set(POPS) for v in at.values()), at
        for shift in SHIFTS:
            held = set()
            for c in _cases("widths", mode):
                if c.shift == shift:
                    held |= set(c.named.values())
            assert set(POPS) <= held, (shift, sorted(set(POPS) - held))
        assert any(c.named.get(LAST, 0) == 0 and sum(c.named.values()) > 0 for c in _cases("populations", mode))
        assert sum(c.expect_failed for c in _cases("ties", mode)) == 3
        assert any(c.vals[sc.counted_slots(c.cnt, c.n_slots_dev), 0].tolist() != sorted(c.vals[sc.counted_slots(c.cnt, c.n_slots_dev), 0].tolist())
                   for c in _cases("ties", mode))                        # (shuffled payloads)
        fill, heads = _cases("garbage", mode)
        assert (fill.lo, fill.shift, fill.key_bits) == (heads.lo, heads.shift, heads.key_bits)
        assert all(fill.named[d] >= 512 + 513 and fill.named[d] > heads.named[d] for d in heads.named)


def _check(pkg, engine, case):
    base = pkg.engine.live_handles()
    k, v, failed = engine.debug_sort_frame(case.mode, case.keys, case.vals, case.cnt, **case.call_args())
    assert pkg.engine.live_handles() == base, f"{case.name}: the call left handles behind"
    if case.expect_failed:
        assert failed != 0, f"{case.name}: the local sort must give this input up"
        return
    assert failed == 0, f"{case.name}: spurious `failed`"
    rk, rv = sc.reference(case)
    assert k.shape[0] == rk.shape[0], f"{case.name}: kept {k.shape[0]}, the counted blocks hold {rk.shape[0]}"
    bad = np.flatnonzero(k != rk)
    assert bad.size == 0, f"{case.name}: {bad.size} keys differ, first at {bad[0]}: {k[bad[0]]:#x} for {rk[bad[0]]:#x}"
    bad = np.flatnonzero(v[:, 0] != rv[:, 0])
    assert bad.size == 0, f"{case.name}: {bad.size} payloads out of order, first at {bad[0]} (key {rk[bad[0]]:#x})"
    assert np.array_equal(v[:, 1], rv[:, 1]), f"{case.name}: a payload's .y left its .x"


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("mode", MODES)
def test_local_sort_paths_match_numpy(pkg, engine, mode, group):
    """(the cases of a group run in the order they were built: the garbage pair depends on it)"""
    for case in _cases(group, mode):
        _check(pkg, engine, case)
