"""K1 and k_cluster_cull keep the frame constants out of VGPR lanes (no GPU: a cross-compile, tools/kernel_resources.py).

A kernel that holds the whole GsrFrame -- about a hundred scalars -- beside its two dozen pointers overflows the scalar register file, and
the compiler parks the excess in the lanes of a VGPR: one v_writelane_b32 to put a scalar away, one v_readlane_b32 to fetch it back, both
issued on the vector ALU of a kernel that is short of exactly that.  With the project's flags the parent of this change held

    k_preprocess 375   k_preprocess_lazy 368   k_preprocess_depth 421   k_preprocess_lazy_depth 424   k_cluster_cull<false> 111   <true> 111

such moves (a quarter of K1's vector instructions).  Read from the argument segment phase by phase (csrc/gsr_device.h: gsr_frame_fetch)
the build has 18 / 6 / 36 / 32 / 12 / 30: what is left are exec masks of nested branches and a few loop invariants, none of them a frame
field.  The bound is a little above the largest of those and a tenth of the smallest parent count of K1; a frame that creeps back into the
registers costs a hundred moves or more, not four."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_MOVES_MAX = 40
KERNELS = ("_Z12k_preprocessjj", "_Z17k_preprocess_lazyjj", "_Z18k_preprocess_depth", "_Z23k_preprocess_lazy_depth", "_Z14k_cluster_cullILb0E", "_Z14k_cluster_cullILb1E")


def test_k1_and_cluster_cull_do_not_park_the_frame_in_vgpr_lanes():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = {}
    for ln in res.stdout.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+\d+\s+sgpr\s+\d+\s+lds\s+\d+\s+scratch\s+(\d+)\s+lanemov\s+(\d+)\s+vector\s+(\d+)\s+scalar\s+(\d+)\s+sload\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert len(rows) > 50, "every kernel of the code object has a row with the appended columns"
    for prefix in KERNELS:
        hit = [(k, v) for k, v in rows.items() if k.startswith(prefix)]
        assert len(hit) == 1, (prefix, [k for k, _ in hit])
        scratch, lanemov, vector, scalar, sload = hit[0][1]
        print(f"{prefix:32s} lane moves {lanemov:3d} vector {vector:5d} scalar {scalar:5d} scalar loads {sload:3d} scratch {scratch}")
        assert lanemov <= LANE_MOVES_MAX, (prefix, lanemov)
        assert scratch == 0, (prefix, scratch)          # (the shading K1's 12 bytes went with the spill registers)
        assert vector > 500 and scalar > 100 and sload > 10, "the counts are of a real kernel body"
