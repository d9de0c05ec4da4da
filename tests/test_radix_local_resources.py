"""k_radix_local keeps all of its 1024 workgroups resident at once (no GPU: a cross-compile, tools/kernel_resources.py).

The small-frame sort's local kernel is bound by how long its slowest workgroup takes, so every bucket's workgroup must start with
the launch: 1024 workgroups of 256 threads over 256 CUs are four per CU, one wave of each per SIMD.  That holds while a workgroup
takes at most 40 KB of the CU's 160 KB of LDS and a wave at most 128 of the SIMD's 512 registers per lane."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 40 * 1024
VGPR_MAX = 128


def test_radix_local_stays_four_workgroups_per_cu():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", ln)
        if m and m.group(1).startswith("_Z13k_radix_localI"):
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert len(rows) == 2, sorted(rows)                       # <uint2> (frames) and <uint32_t> (gsr_debug_sort_pairs_local)
    for name, (vgpr, sgpr, lds, scratch) in rows.items():
        print(f"{name}: vgpr {vgpr} lds {lds} scratch {scratch}")
        assert lds <= LDS_MAX, (name, lds)
        assert vgpr <= VGPR_MAX, (name, vgpr)
        assert scratch == 0, (name, scratch)
