#!/usr/bin/env python3
"""Compile csrc/gsr_api.hip for gfx950 with -save-temps (into a scratch directory) and print, per kernel, the
registers / LDS / scratch the compiler allocated and, behind them, static instruction counts of its body: lanemov (v_readlane_b32 + v_writelane_b32:
scalars parked in VGPR lanes), vector, scalar, sload (instruction_counts()).  `--isa NAME` also dumps that kernel's assembly; `-D...` flags are
passed through.  No GPU needed (hipcc cross-compiles).   python tools/kernel_resources.py [--isa k_blend] [-DBL_ROUND=64]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "houdini-gsplat-renderer_amd", "csrc", "gsr_api.hip")


def instruction_counts(asm):
    """Static instruction counts per kernel, from its text between `name:` and `.Lfunc_end`: `lanemov` = v_readlane_b32 + v_writelane_b32
    (how the compiler parks scalars in lanes of a VGPR when the scalar file is full; v_readfirstlane is not counted), `vector` = every v_*
    (the lane moves among them), `scalar` = every s_*, `sload` = the scalar memory loads among those."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", asm, re.S | re.M):
        c = {"lanemov": 0, "vector": 0, "scalar": 0, "sload": 0}
        for ln in m.group(2).splitlines():
            op = ln.split(None, 1)[0] if ln.strip() else ""
            if op.startswith("v_"):
                c["vector"] += 1
                if op in ("v_readlane_b32", "v_writelane_b32"):
                    c["lanemov"] += 1
            elif op.startswith("s_"):
                c["scalar"] += 1
                if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
                    c["sload"] += 1
        out[m.group(1)] = c
    return out


def main():
    isa = None
    extra = []
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a == "--isa":
            isa = args.pop(0)
        else:
            extra.append(a)
    tmp = tempfile.mkdtemp(prefix="gsr_res_")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c",
           "-save-temps=obj", "-o", os.path.join(tmp, "gsr_api.o"), SRC] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    asm = open(os.path.join(tmp, "gsr_api-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    static = instruction_counts(asm)
    for blk in re.findall(r"- \.agpr_count.*?\.wavefront_size:\s+\d+", asm, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda k: re.search(r"\." + k + r":\s+(\d+)", blk).group(1)
        c = static.get(name, {})
        print(f"{name[:70]:70s} vgpr {g('vgpr_count'):>3s} sgpr {g('sgpr_count'):>3s} lds {g('group_segment_fixed_size'):>6s} "
              f"scratch {g('private_segment_fixed_size'):>4s} lanemov {c.get('lanemov', 0):>4d} vector {c.get('vector', 0):>5d} "
              f"scalar {c.get('scalar', 0):>5d} sload {c.get('sload', 0):>4d}")
    if isa:
        m = re.search(r"^(_Z\w*" + re.escape(isa) + r"\w*):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", asm, re.S | re.M)   # (a kernel may hold several s_endpgm)
        if m:
            out = os.path.join(tmp, isa + ".s")
            open(out, "w").write(m.group(0))
            print("ISA of", m.group(1), "->", out)


if __name__ == "__main__":
    main()
