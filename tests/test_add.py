"""Adding without a GPU: gsr_add_capacity (the capacity policy) against the rule of include/gsplat_hip.h, the NULL-handle refusals of
the verbs, the Python argument handling in front of the library, and the resources the compiler gives k_add_pack."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
MAX = 0x7fffffff


def _rule(cap, need):
    """include/gsplat_hip.h: what fits keeps the capacity; otherwise 25 % headroom, clamped"""
    return cap if need <= cap else min(need + need // 4, MAX)


def test_add_capacity_follows_the_rule(pkg):
    E = pkg.engine
    cases = [(0, 0), (0, 1), (1, 1), (1, 2), (1, 5), (357, 0), (357, 356), (357, 357), (357, 358), (357, 375), (468, 468), (468, 469),
             (6_000_000, 6_300_000), (MAX, MAX), (MAX - 1, MAX), (0, MAX), (10, 1_717_986_918), (10, 1_717_986_919), (10, 1_717_986_920),
             (2 ** 40, 5)]
    for cap, need in cases:
        assert E.add_capacity(cap, need) == _rule(cap, need), (cap, need)
    assert E.add_capacity(357, 357) == 357                      # need == cap: it fits
    assert E.add_capacity(357, 358) == 358 + 89                 # cap + 1: 25 % of what is needed, rounded down
    assert E.add_capacity(4, 7) == 8 and E.add_capacity(0, 3) == 3
    assert E.add_capacity(10, 1_717_986_918) == 1_717_986_918 + 429_496_729 == MAX          # exactly the clamp value, unclamped
    assert E.add_capacity(10, 1_717_986_919) == MAX                                          # one more: clamped
    assert E.add_capacity(10, MAX) == MAX
    # a run of adds of 5 % grows now and then, not every time
    cap, n, grows = 1000, 1000, 0
    for _ in range(20):
        n += 50
        new = E.add_capacity(cap, n)
        grows += new != cap
        cap = new
        assert cap >= n
    assert 0 < grows < 10


def test_add_capacity_refusals(pkg):
    L, E = pkg.load_library(), pkg.engine
    for cap, need in ((-1, 5), (5, -1), (-1, -1), (0, MAX + 1), (MAX + 5, MAX + 1), (-2 ** 63, 0)):
        assert L.gsr_add_capacity(cap, need) == GSR_E_INVALID, (cap, need)
        assert b"gsr_add_capacity" in L.gsr_last_error()
        with pytest.raises(E.GsrError):
            E.add_capacity(cap, need)
    with pytest.raises(E.GsrError):
        E.add_capacity(2 ** 63, 1)                              # not a 64-bit count: never reaches the library


def test_null_handles_and_symbols(pkg):
    L, E = pkg.load_library(), pkg.engine
    P, h, a = np.zeros((1, 3), np.float32), np.zeros(16, np.uint16), np.ones(1, np.float32)
    total = C.c_int64(-7)
    args = (P.ctypes.data, h.ctypes.data, a.ctypes.data, h.ctypes.data, h.ctypes.data, None, None, None)
    assert L.gsr_add(None, 1, *args, C.byref(total)) == GSR_E_INVALID and b"gsr_add" in L.gsr_last_error()
    assert L.gsr_add(None, 0, *args, C.byref(total)) == GSR_E_INVALID
    d = E.gsr_device_attrs()
    assert L.gsr_add_device(None, 1, C.byref(d), C.byref(total)) == GSR_E_INVALID and b"gsr_add_device" in L.gsr_last_error()
    assert L.gsr_multi_add(None, 1, *args, C.byref(total)) == GSR_E_INVALID
    assert L.gsr_get_add(None, None, None, None, None, None) == GSR_E_INVALID
    assert total.value == -7
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gsr_add", "gsr_add_device", "gsr_add_capacity", "gsr_get_add", "gsr_multi_add"):
        assert name in E.C_ABI_SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name)
    assert re.search(r"int64_t\s+gsr_add_capacity\(int64_t capacity, int64_t n_needed\)", hdr)


def test_python_argument_handling(pkg):
    E, S = pkg.engine, pkg.scenes
    A = S.make_scene(20, seed=1, sh=True)
    B = S.make_scene(7, seed=2, sh=True)
    # Splats.concat: this cloud, then the other, every array
    AB = A.concat(B)
    assert AB.n == 27 and AB.has_sh
    for name in ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz"):
        got = getattr(AB, name)
        assert got.flags["C_CONTIGUOUS"] and got.dtype == getattr(A, name).dtype
        assert np.array_equal(got[:20], getattr(A, name)) and np.array_equal(got[20:], getattr(B, name)), name
    assert A.concat(A.subset(slice(0, 0))).n == 20
    plain = S.make_scene(7, seed=2, sh=False)
    assert not plain.concat(plain).has_sh and plain.concat(plain).n == 14
    with pytest.raises(ValueError):
        A.concat(plain)
    # add_arrays: what Engine.add hands the library
    arr = E.add_arrays(B)
    assert arr.n == 7 and all(p is not None for p in arr.ptrs())
    assert E.add_arrays(plain).ptrs()[5:] == [None, None, None]
    assert E.add_arrays(B, has_sh=True).n == 7 and E.add_arrays(plain, has_sh=False).n == 7
    for cloud, has in ((B, False), (plain, True)):
        with pytest.raises(E.GsrError):
            E.add_arrays(cloud, has_sh=has)                     # SH presence against the resident cloud's
    for missing in ("P", "Cd", "alpha", "scale", "orient"):
        broken = S.Splats(**{k: (None if k == missing else getattr(B, k)) for k in ("P", "Cd", "alpha", "scale", "orient")})
        with pytest.raises(E.GsrError):
            E.add_arrays(broken)                                # refused before the library is reached
        with pytest.raises(E.GsrError):
            E.Engine.add(None, broken)
        with pytest.raises(E.GsrError):
            E.MultiEngine.add(None, broken)
    for bad in ("a string", None, 3, {"Cd": 5}, {"P": None}):
        with pytest.raises(E.GsrError):
            E.Engine.add_device(None, bad)                      # no dict of device arrays, or no P
    with pytest.raises(E.GsrError):
        E.Engine.add_device(None, {"P": 4096})                  # a raw device pointer does not say n
    with pytest.raises(E.GsrError):
        E.Engine.add_device(None, {"P": 4096, "sh": 8192}, n=3)  # ... nor does a raw sh pointer say sh_vec3_per_point
    with pytest.raises(E.GsrError):
        E.Engine.add_device(None, {"P": 4096, "colour": 8192}, n=3)


def test_add_pack_stays_within_k_packs_budget():
    """from the code object, as tools/kernel_resources.py reads it (a cross-compile: no GPU): both instantiations of k_add_pack exist,
    use no scratch, no more LDS than k_pack<true>, and at most 64 vector registers -- eight waves per SIMD (512 / 64)"""
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
    mine = {k: v for k, v in rows.items() if k.startswith("_Z10k_add_packILb")}
    assert sorted(k[:21] for k in mine) == ["_Z10k_add_packILb0EEv", "_Z10k_add_packILb1EEv"], sorted(rows)
    for name, (vg, sg, lds, scratch) in sorted(mine.items()):
        print(f"{name[:24]}: vgpr {vg} sgpr {sg} lds {lds} scratch {scratch}; k_pack<true>: vgpr {pack[0]} lds {pack[2]}")
        assert scratch == 0 and lds <= pack[2] and vg <= 64, (name, (vg, sg, lds, scratch), pack)
    ext = [v for k, v in rows.items() if k.startswith("_Z17k_add_mask_extend")]
    assert len(ext) == 1 and ext[0][3] == 0 and ext[0][2] == 0
