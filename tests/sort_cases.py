"""Inputs and the numpy reference for the depth sort's kernels (csrc/k_sort.h), driven through Engine.debug_sort_frame.

A case is K1's block-compacted layout: `cnt[b]` items at the head of slots [256 b, 256 b + 256), the other slots garbage; only
the blocks below n_slots_dev / 256 count.  The generators need no GPU (tests/test_sort_kernels.py runs every one of them and
checks what they promise); tests/test_sort_kernels_gpu.py sorts them on the device and compares bit for bit.
"""
from dataclasses import dataclass, field

import numpy as np

BLOCK = 256            # RS_SRC_BLOCK: slots of one K1 workgroup-iteration
BUCKETS = 1024         # BK_BUCKETS
BK_CAP = 8192          # slots of a bucket's region: a bucket beyond it makes the local sort give up
RL_MAX_RUN = 64        # longest run of equal keys the local kernel re-orders
RL_CHUNK = 2048        # keys a workgroup of the local kernel holds at once
GARBAGE = 0xDEADBEEF   # what the slots behind a block's items hold
TILE = {0: 3072, 1: 1024}   # slots per workgroup of the global passes: GLOBAL, GLOBAL_MID

GLOBAL, GLOBAL_MID, LOCAL_GATHER, LOCAL_K1, LOCAL_DIRECT, ORDERED = range(6)
LOCAL_MODES = (LOCAL_GATHER, LOCAL_K1, LOCAL_DIRECT)
MODE_NAMES = ("global", "global_mid", "local_gather", "local_k1", "local_direct", "ordered")

POPULATIONS = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 8191, 8192)
SHIFTS = (0, 1, 8, 9, 16, 17, 22)
GLOBAL_BITS = ((1, True), (8, True), (9, True), (10, True), (16, True), (17, True), (18, True), (18, False), (19, True), (27, True),
               (27, False), (28, True), (32, True))
GLOBAL_FILLS = ("full", "empty", "alternate", "random", "last_only", "wave_00k")
GLOBAL_DUPS = ("all_equal", "two", "third")
ORDERED_BLOCKS = (1, 1023, 1024, 1025, 2049, 3073)


@dataclass
class Case:
    name: str
    mode: int
    keys: np.ndarray            # [n_slots] uint32
    vals: np.ndarray            # [n_slots, 2] uint32
    cnt: np.ndarray             # [n_slots / 256] uint32
    n_slots_dev: int
    key_bits: int = 32
    allow9: bool = True
    lo: int = 0
    shift: int = 0
    range_dev: bool = False
    k1_grid: int = 1 << 30
    expect_failed: bool = False
    named: dict = field(default_factory=dict)   # local cases: bucket -> the population it was built to hold

    @property
    def n_slots(self):
        return int(self.keys.shape[0])

    def call_args(self):
        return dict(n_slots_dev=self.n_slots_dev, key_bits=self.key_bits, allow9=self.allow9, lo=self.lo, shift=self.shift,
                    range_dev=self.range_dev, k1_grid=self.k1_grid)


# ---------------------------------------------------------------------------------------------
# the reference
def counted_slots(cnt, n_slots_dev):
    """slots of the items that count, in slot order"""
    m = n_slots_dev // BLOCK
    c = np.asarray(cnt[:m], np.int64)
    if c.sum() == 0:
        return np.zeros(0, np.int64)
    first = np.repeat(np.arange(m, dtype=np.int64) * BLOCK, c)
    within = np.arange(c.sum(), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    return first + within


def reference(case):
    """(keys, vals[., 2]) as the device must return them: GLOBAL* equal keys in slot order, LOCAL_* equal keys in the order of
    vals[., 0], ORDERED the sequence itself"""
    idx = counted_slots(case.cnt, case.n_slots_dev)
    k, v = case.keys[idx], case.vals[idx]
    if case.mode in (GLOBAL, GLOBAL_MID):
        o = np.argsort(k, kind="stable")
    elif case.mode in LOCAL_MODES:
        o = np.lexsort((v[:, 0], k))
    else:
        o = np.arange(k.shape[0])
    return k[o], v[o]


def bucket_of(keys, lo, shift):
    """rs_digit<CLAMP>: min((key - lo) >> shift, 1023), 0 for keys not above lo"""
    k = np.asarray(keys, np.int64)
    return np.where(k > lo, (k - lo) >> shift, 0).clip(0, BUCKETS - 1)


def conditions(case):
    """(largest bucket, longest run of equal keys) among the items that count -- what decides whether the local sort holds"""
    idx = counted_slots(case.cnt, case.n_slots_dev)
    if idx.size == 0:
        return 0, 0
    k = case.keys[idx]
    pops = np.bincount(bucket_of(k, case.lo, case.shift), minlength=BUCKETS)
    return int(pops.max()), int(np.unique(k, return_counts=True)[1].max())


def bucket_populations(case):
    idx = counted_slots(case.cnt, case.n_slots_dev)
    return np.bincount(bucket_of(case.keys[idx], case.lo, case.shift), minlength=BUCKETS)


def tie_features(case):
    """which of the tie shapes the case holds, from the sorted keys of every bucket"""
    idx = counted_slots(case.cnt, case.n_slots_dev)
    k = np.sort(case.keys[idx])
    b = bucket_of(k, case.lo, case.shift)
    found = set()
    edges = np.flatnonzero(np.diff(b)) + 1
    for kb in np.split(k, edges):
        p = kb.shape[0]
        if p < 2:
            continue
        _, starts, lens = np.unique(kb, return_index=True, return_counts=True)
        for length in (2, 64, 65):
            if (lens == length).any():
                found.add(f"run{length}")
        if kb[0] == kb[1]:
            found.add("start")
        if kb[-1] == kb[-2]:
            found.add("end")
        if p > RL_CHUNK and kb[RL_CHUNK - 1] == kb[RL_CHUNK]:
            found.add("straddle")
        if p <= 64 and (lens > 1).any():
            found.add("small")
    return found


# ---------------------------------------------------------------------------------------------
# layouts
def random_counts(rng, n_blocks, total):
    """n_blocks counts in [0, 256] that sum to total"""
    assert 0 <= total <= n_blocks * BLOCK
    c = rng.integers(0, BLOCK + 1, n_blocks).astype(np.int64)
    diff = int(total - c.sum())
    for b in rng.permutation(n_blocks):
        if diff == 0:
            break
        step = min(BLOCK - c[b], diff) if diff > 0 else -min(c[b], -diff)
        c[b] += step
        diff -= step
    assert c.sum() == total
    return c.astype(np.uint32)


def lay_out(rng, cnt, item_keys, shuffle_x=False):
    """keys / vals of the layout: block b's first cnt[b] slots take the next cnt[b] of item_keys, the rest GARBAGE.  Payload .x is
    unique and grows with the slot (what K1 writes) unless shuffle_x; .y is random bits"""
    n_blocks = cnt.shape[0]
    n_slots = n_blocks * BLOCK
    assert item_keys.shape[0] == int(cnt.astype(np.int64).sum())
    keys = np.full(n_slots, GARBAGE, np.uint32)
    vals = np.full((n_slots, 2), 0xFFFFFFFF, np.uint32)
    idx = counted_slots(cnt, n_slots)
    keys[idx] = item_keys
    x = idx.astype(np.uint32) * np.uint32(3) + np.uint32(7)          # unique, increasing with the slot
    vals[idx, 0] = rng.permutation(x) if shuffle_x else x
    vals[idx, 1] = rng.integers(0, 1 << 32, idx.shape[0], dtype=np.uint64).astype(np.uint32)
    return keys, vals


# ---------------------------------------------------------------------------------------------
# the global passes
def _fill(rng, fill, m):
    if fill == "full":
        return np.full(m, BLOCK, np.uint32)
    if fill == "empty":
        return np.zeros(m, np.uint32)
    if fill == "alternate":
        return (np.arange(m) % 2 * BLOCK).astype(np.uint32)
    if fill == "random":
        return rng.integers(0, BLOCK + 1, m).astype(np.uint32)
    if fill == "last_only":
        c = np.zeros(m, np.uint32)
        c[-1] = 1
        return c
    if fill == "wave_00k":            # (GLOBAL: a wave's three blocks; GLOBAL_MID: three waves of one block each)
        c = rng.integers(1, BLOCK + 1, m).astype(np.uint32)
        c[np.arange(m) % 3 != 2] = 0
        return c
    raise ValueError(fill)


def _global_keys(rng, n, bits, dup):
    top = (1 << bits) - 1
    if dup == "all_equal":
        return np.full(n, int(rng.integers(0, top + 1)), np.uint32)
    if dup == "two":
        return np.where(rng.integers(0, 2, n) == 1, top, 0).astype(np.uint32)
    k = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
    if n >= 3:                        # a third of the keys repeated: stability matters
        k[: n // 3] = k[n // 3: 2 * (n // 3)]
    if n >= 2:                        # the ends of the key range (at 32 bits: the kernels' own filler for missing items)
        where = rng.choice(n, 2, replace=False)
        k[where[0]], k[where[1]] = 0, top
    return k


def global_sizes(mode):
    t = TILE[mode]
    own = [256, t - 256, t, t + 256, 8 * t + 256, 9 * t, 17 * t]
    return [(n, n) for n in own] + [(17 * t, 8 * t + 256), (17 * t, 256)]


def global_case(mode, n_slots, n_dev, fill, bits, allow9, dup, seed, shuffle_x=False):
    rng = np.random.default_rng(seed)
    m, m_all = n_dev // BLOCK, n_slots // BLOCK
    cnt = np.concatenate([_fill(rng, fill, m), rng.integers(1, BLOCK + 1, m_all - m).astype(np.uint32)])   # (decoys behind n_dev)
    total = int(cnt.astype(np.int64).sum())
    counted = int(cnt[:m].astype(np.int64).sum())
    item_keys = np.concatenate([_global_keys(rng, counted, bits, dup), _global_keys(rng, total - counted, bits, "third")])
    keys, vals = lay_out(rng, cnt, item_keys, shuffle_x)
    name = f"{MODE_NAMES[mode]}-{n_slots}-{n_dev}-{fill}-{bits}{'' if allow9 else 'x'}-{dup}-{seed}{'-shuffled' if shuffle_x else ''}"
    return Case(name, mode, keys, vals, cnt, n_dev, key_bits=bits, allow9=allow9)


def global_cases(mode):
    """every size with every fill (key widths and duplicate regimes taking turns), then every key width with every duplicate regime
    at two sizes, then shuffled payloads: equal keys must leave in SLOT order whatever .x says"""
    out = []
    t = TILE[mode]
    turn = 0
    for n_slots, n_dev in global_sizes(mode):
        for fill in GLOBAL_FILLS:
            bits, allow9 = GLOBAL_BITS[turn % len(GLOBAL_BITS)]
            out.append(global_case(mode, n_slots, n_dev, fill, bits, allow9, GLOBAL_DUPS[turn % 3], 1000 + turn))
            turn += 1
    for bits, allow9 in GLOBAL_BITS:
        for dup in GLOBAL_DUPS:
            for n_slots, n_dev, fill in ((8 * t + 256, 8 * t + 256, "random"), (17 * t, 9 * t + 512, "full")):
                out.append(global_case(mode, n_slots, n_dev, fill, bits, allow9, dup, 2000 + turn))
                turn += 1
    for bits, dup, fill in ((32, "third", "random"), (9, "two", "wave_00k"), (17, "all_equal", "alternate")):
        out.append(global_case(mode, 9 * t, 9 * t, fill, bits, True, dup, 3000 + turn, shuffle_x=True))
        turn += 1
    return out


# ---------------------------------------------------------------------------------------------
# the small-frame sort
def _bucket_keys(rng, base, width, pop, ties):
    """pop sorted keys of [base, base + width), no key more than RL_MAX_RUN times; ties: runs to plant, (position, length) in
    the sorted sequence (planted only where the keys around them are distinct)"""
    if pop == 0:
        return np.zeros(0, np.uint32)
    assert pop <= width * RL_MAX_RUN, "the bucket cannot hold that many keys without a run that defeats the kernel"
    if width >= 2 * pop:
        off = np.zeros(0, np.int64)
        while off.shape[0] < pop:
            off = np.unique(np.concatenate([off, rng.integers(0, width, 2 * pop)]))
        off = np.sort(rng.choice(off, pop, replace=False))
        for pos, length in ties:
            if pos >= 0 and pos + length <= pop:
                off[pos: pos + length] = off[pos]
    else:                             # a narrow bucket: every key about pop / width times
        q, r = divmod(pop, width)
        off = np.repeat(np.arange(width, dtype=np.int64), q + (np.arange(width) < r))
    k = base + off
    assert k.min() >= base and k.max() < base + width and np.unique(k, return_counts=True)[1].max() <= RL_MAX_RUN
    return k.astype(np.uint32)


def _ties_for(pop):
    """the runs planted in a wide bucket of `pop` keys: 2 at the start and the end, 64 inside, one across sorted positions 2047 / 2048"""
    t = []
    if pop >= 4:
        t += [(0, 2), (pop - 2, 2)]
    if pop >= 200:
        t.append((70, 64))
    if pop > RL_CHUNK + 8:
        t.append((RL_CHUNK - 3, 6))
    if 8 <= pop <= 64:
        t.append((3, 3))
    return t


def local_layout(rng, shift, lo, key_bits, named, n_blocks_mod=None, extra_blocks=0):
    """named: bucket -> population.  Returns (cnt, item keys in a random order, n_dev): bucket d takes keys of its own range (the first
    bucket: everything below lo + 2^shift, the last: everything from lo + 1023 * 2^shift up to the key width)"""
    top = 1 << key_bits
    parts = []
    for d, pop in named.items():
        if d == 0:
            base, width = 0, min(lo + (1 << shift), top)
        elif d == BUCKETS - 1:
            base = lo + ((BUCKETS - 1) << shift)
            width = top - base
        else:
            base, width = lo + (d << shift), 1 << shift
        assert width > 0 and base + width <= top, (d, shift, lo, key_bits)
        parts.append(_bucket_keys(rng, base, width, pop, _ties_for(pop)))
    item_keys = rng.permutation(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)
    total = item_keys.shape[0]
    m = max(1, -(-total // 160))      # (blocks about five eighths full)
    if n_blocks_mod is not None:
        while m % 4 != n_blocks_mod:
            m += 1
    cnt = random_counts(rng, m, total)
    if extra_blocks:                  # decoys behind n_slots_dev, with keys that would land in real buckets
        dec = rng.integers(1, BLOCK + 1, extra_blocks).astype(np.uint32)
        cnt = np.concatenate([cnt, dec])
        decoys = rng.integers(0, top, int(dec.sum()), dtype=np.uint64).astype(np.uint32)
        item_keys = np.concatenate([item_keys, decoys])
    return cnt, item_keys, m * BLOCK


def _local_plans(shift):
    """(lo, key_bits, {bucket: population}) per call: together the calls of one shift give every POPULATIONS entry a bucket.  A
    middle bucket is 2^shift keys wide and no key may come more than 64 times, so at shift 0 and 1 the large populations
    live in the first and the last bucket, which take everything outside the range and are sorted on all key bits"""
    first, last = 0, BUCKETS - 1
    if shift >= 8:
        key_bits = 24 if shift <= 9 else 32
        lo = 5000 if shift < 22 else 4099         # (shift 22: lo + 1023 * 2^22 is still below 2^32)
        named = {3 + 7 * i: p for i, p in enumerate(POPULATIONS)}
        named[first], named[last] = 300, 2500
        return [(lo, key_bits, named)]
    cap = RL_MAX_RUN << shift                     # what a middle bucket can hold
    small = [p for p in POPULATIONS if p <= cap]
    big = [p for p in POPULATIONS if p > cap]
    plans = []
    for i in range(0, len(big), 2):
        named = {5 + 11 * j: p for j, p in enumerate(small)}
        named[last] = big[i]
        if i + 1 < len(big):
            named[first] = big[i + 1]
        plans.append((3000, 32, named))
    # ... and 10-bit keys: the range ends beyond the keys, what lies below lo is sorted on the ten bits
    plans.append((600, 10, {first: 2049, **{5 + 11 * j: p for j, p in enumerate(small)}}))
    return plans


def local_cases(mode):
    """the calls of one scatter: every shift's plans; n_slots_dev < n_slots; LOCAL_K1 also small grids, block counts 4k + 1 / 2 / 3
    and the range in device memory; shuffled payloads (equal keys leave in .x order); the two inputs that must raise `failed`"""
    out = []
    seed = 5000 + 100 * mode
    for shift in SHIFTS:
        for i, (lo, key_bits, named) in enumerate(_local_plans(shift)):
            seed += 1
            rng = np.random.default_rng(seed)
            cnt, item_keys, n_dev = local_layout(rng, shift, lo, key_bits, named, extra_blocks=3 if i == 0 else 0)
            keys, vals = lay_out(rng, cnt, item_keys, shuffle_x=(shift in (1, 9, 17) and i == 0))
            out.append(Case(f"{MODE_NAMES[mode]}-shift{shift}-{i}", mode, keys, vals, cnt, n_dev, key_bits=key_bits, lo=lo, shift=shift,
                            named=dict(named)))
    if mode == LOCAL_K1:
        named = {3 + 7 * i: p for i, p in enumerate(POPULATIONS[:11])}
        for mod in (1, 2, 3):
            for grid, extra, range_dev in ((1, 0, False), (3, 2, True), (1 << 30, 0, mod == 2)):
                seed += 1
                rng = np.random.default_rng(seed)
                cnt, item_keys, n_dev = local_layout(rng, 9, 5000, 24, named, n_blocks_mod=mod, extra_blocks=extra)
                keys, vals = lay_out(rng, cnt, item_keys)
                out.append(Case(f"local_k1-blocks4k+{mod}-grid{min(grid, 999)}-{'dev' if range_dev else 'arg'}", mode, keys, vals, cnt, n_dev,
                                key_bits=24, lo=5000, shift=9, range_dev=range_dev, k1_grid=grid, named=dict(named)))
    # the two inputs the kernel is entitled to give up: a bucket one key beyond its region, a run one key beyond RL_MAX_RUN
    rng = np.random.default_rng(seed + 50)
    cnt, item_keys, n_dev = local_layout(rng, 16, 5000, 32, {9: BK_CAP + 1, 40: 100})
    keys, vals = lay_out(rng, cnt, item_keys)
    out.append(Case(f"{MODE_NAMES[mode]}-bucket-8193", mode, keys, vals, cnt, n_dev, key_bits=32, lo=5000, shift=16, expect_failed=True))
    cnt, item_keys, n_dev = local_layout(rng, 16, 5000, 32, {9: 500, 40: 100})
    item_keys = np.sort(item_keys)
    item_keys[200: 200 + RL_MAX_RUN + 1] = item_keys[200]
    keys, vals = lay_out(rng, cnt, rng.permutation(item_keys))
    out.append(Case(f"{MODE_NAMES[mode]}-run-65", mode, keys, vals, cnt, n_dev, key_bits=32, lo=5000, shift=16, expect_failed=True))
    return out


# ---------------------------------------------------------------------------------------------
# the position-keyed order
def ordered_cases():
    out = []
    seed = 9000
    for m in ORDERED_BLOCKS:
        for fill in ("random", "empty", "full"):
            seed += 1
            rng = np.random.default_rng(seed)
            extra = 5
            cnt = np.concatenate([_fill(rng, fill, m), rng.integers(1, BLOCK + 1, extra).astype(np.uint32)])
            item_keys = rng.integers(0, 1 << 32, int(cnt.astype(np.int64).sum()), dtype=np.uint64).astype(np.uint32)
            keys, vals = lay_out(rng, cnt, item_keys)
            out.append(Case(f"ordered-{m}-{fill}", ORDERED, keys, vals, cnt, m * BLOCK))
    return out


def all_groups():
    """name -> a function that makes the group's cases (one parametrised GPU test each)"""
    g = {"global": lambda: global_cases(GLOBAL), "global_mid": lambda: global_cases(GLOBAL_MID), "ordered": ordered_cases}
    for mode in LOCAL_MODES:
        g[MODE_NAMES[mode]] = (lambda m: lambda: local_cases(m))(mode)
    return g
