"""Removal without a GPU: gsr_remove_map (where gsr_remove puts the survivors) against a numpy model, the Python argument handling of
Engine.remove / engine.remove_map, the NULL-handle refusals, and the resources the compiler gives the kernels of k_remove.h."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
SIZES = (0, 1, 31, 32, 33, 357)


def _masks(n):
    """name -> boolean mask of n splats, True = goes"""
    rng = np.random.default_rng(1000 + n)
    one = np.zeros(n, bool)
    if n:
        one[n // 2] = True
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "one": one, "alternating": np.arange(n) % 2 == 0,
            "random": rng.random(n) < 0.4}


def _model(gone):
    """the rule of include/gsplat_hip.h: survivor i becomes the number of survivors before it; a removed splat -1"""
    kept = ~gone
    idx = (np.cumsum(kept) - kept).astype(np.int32)
    idx[gone] = -1
    return idx, int(kept.sum())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("garbage", (False, True))
def test_remove_map_matches_the_cumsum_model(pkg, n, garbage):
    L = pkg.load_library()
    for name, gone in _masks(n).items():
        words = pkg.engine.pack_mask(gone)
        if words.size == 0:
            words = np.zeros(1, np.uint32)
        if garbage and n % 32:
            words[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)          # bits at and behind n in the last word: ignored
        if garbage and n % 32 == 0:
            words = np.concatenate([words, np.full(1, 0xffffffff, np.uint32)])     # ... and a whole word behind n is never read
        want, left = _model(gone)
        got, n_left = np.full(n + 1, 12345, np.int32), C.c_int64(-5)
        assert L.gsr_remove_map(words.ctypes.data, n, got.ctypes.data, C.byref(n_left)) == 0, (n, name)
        assert n_left.value == left, (n, name)
        assert np.array_equal(got[:n], want), (n, name)
        assert got[n] == 12345, "wrote behind n"
        # either out pointer may be NULL
        assert L.gsr_remove_map(words.ctypes.data, n, None, C.byref(n_left)) == 0 and n_left.value == left
        assert L.gsr_remove_map(words.ctypes.data, n, got.ctypes.data, None) == 0


def test_remove_map_refusals(pkg):
    L = pkg.load_library()
    w = np.zeros(1, np.uint32)
    assert L.gsr_remove_map(None, 1, None, None) == GSR_E_INVALID
    assert L.gsr_remove_map(w.ctypes.data, -1, None, None) == GSR_E_INVALID
    assert L.gsr_remove_map(None, 0, None, None) == 0                   # no splats: no word is read


def test_null_handles_and_constants(pkg):
    L, E = pkg.load_library(), pkg.engine
    w = np.zeros(1, np.uint32)
    assert L.gsr_remove(None, w.ctypes.data, 0, 0, None) == GSR_E_INVALID
    assert L.gsr_multi_remove(None, w.ctypes.data, 0, None) == GSR_E_INVALID
    assert L.gsr_get_removal(None, None, None, None) == GSR_E_INVALID
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_REMOVE_BLOCK\s+(\d+)", hdr).group(1)) == E.REMOVE_BLOCK
    assert int(re.search(r"#define GSR_REMOVE_HIDDEN\s+(\d+)", hdr).group(1)) == E.REMOVE_HIDDEN
    assert E.REMOVE_BLOCK % 64 == 0


def test_python_mask_handling(pkg):
    E = pkg.engine
    rng = np.random.default_rng(3)
    gone = rng.random(357) < 0.5
    words = E.removal_mask(gone)
    assert words.dtype == np.uint32 and words.size == 12 and np.array_equal(words, E.pack_mask(gone))
    assert E.removal_mask(words) is not None and np.array_equal(E.removal_mask(words), words)       # packed words pass through
    assert E.removal_mask(np.zeros(0, bool)).size == 1                                              # never an empty buffer
    with pytest.raises(E.GsrError):
        E.removal_mask(np.zeros(4, np.float32))
    want, left = _model(gone)
    got, n_left = E.remove_map(gone)
    assert n_left == left and np.array_equal(got, want)
    got, n_left = E.remove_map(words, 357)
    assert n_left == left and np.array_equal(got, want)
    got, n_left = E.remove_map(words, 300)                              # the same words over fewer splats
    want300, left300 = _model(gone[:300])
    assert n_left == left300 and np.array_equal(got, want300)
    assert np.array_equal(E.removal_words(gone, 357), words) and E.removal_words(None, 357) is None
    assert np.array_equal(E.removal_words(words, 357), words) and np.array_equal(E.removal_words(words, 12 * 32), words)
    for bad_mask, bad_n in ((gone, 356), (gone, 358), (words, 12 * 32 + 1), (words[:11], 357)):
        with pytest.raises(E.GsrError):
            E.removal_words(bad_mask, bad_n)                            # what Engine.remove refuses before the library reads the words
    with pytest.raises(E.GsrError):
        E.remove_map(words)                                             # packed words do not say n
    with pytest.raises(E.GsrError):
        E.remove_map(words, 12 * 32 + 1)                                # more splats than the words cover
    for bad in ("a string", 1.5, None):
        with pytest.raises(E.GsrError):
            E.Engine.remove_device(None, bad)                           # refused before the library is reached


def test_removal_kernels_stay_within_k_packs_budget():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): every kernel of k_remove.h uses no
    scratch, and no more vector registers or LDS than k_pack<true>"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    pack = [v for k, v in rows.items() if k.startswith("_Z6k_packILb1E")]
    assert len(pack) == 1
    pack = pack[0]
    mine = {k: v for k, v in rows.items() if re.match(r"_Z\d+k_remove_", k)}
    names = set()
    for k in mine:                                                      # _Z<length><name>[I<template arguments>E]...
        length = int(re.match(r"_Z(\d+)", k).group(1))
        rest = k[2 + len(str(length)):]
        names.add((rest[:length], rest[length:length + 5] if rest[length:length + 1] == "I" else None))
    assert names == {("k_remove_mark", "ILb0E"), ("k_remove_mark", "ILb1E"), ("k_remove_scan", None),
                     ("k_remove_compact", "ILb0E"), ("k_remove_compact", "ILb1E")}, sorted(mine)
    for name, (vg, sg, lds, scratch) in sorted(mine.items()):
        print(f"{name[:40]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}; k_pack<true>: vgpr {pack[0]} lds {pack[2]}")
        assert scratch == 0 and vg <= pack[0] and lds <= pack[2], (name, (vg, sg, lds, scratch), pack)
