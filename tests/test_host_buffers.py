"""CPU tests of the owning handles (csrc/gsr_host_buffers.h: DevMem, PinnedMem, Event, Stream, DevVec, StageBuf, the groups).

tests/host_buffers_main.cpp includes the header through tests/hip_stub/hip/hip_runtime.h -- the HIP calls the header uses, backed by
malloc / free, with a count of live objects per kind and a way to fail the k-th acquisition -- and is built here with the host
compiler under the address and undefined-behaviour sanitizers, then run as a program of its own.  The program checks scope exit, move
construction and assignment, swap, reset, alloc(0), failed allocations, the growing buffers (DevVec: what grows, what drains, what
a failure leaves), StageBuf, the groups that share a capacity (every member or none) and the pinned aliases, and that every
counter is 0 at its end (its exit status); the sanitizers add use-after-free, double free and leaks."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def test_handles_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "host_buffers_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(TESTS, "hip_stub"), "-o", exe, os.path.join(TESTS, "host_buffers_main.cpp")]
    # (the sanitizer runtimes inside the program where the compiler has them as archives: it then starts whatever else the loader brings)
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)   # (the runtimes are linked in: nothing is preloaded)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.strip().splitlines()[-1] == "0 checks failed"


def test_live_handles_without_a_context(pkg):
    """gsr_debug_live_handles needs no context and no GPU: a process that never created a context reads four zeros"""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; pkg = g.load_package(); "
            "print(pkg.engine.live_handles())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "(0, 0, 0, 0)"
    assert pkg.load_library().gsr_debug_live_handles(None) == -1
    assert "gsr_debug_live_handles" in pkg.engine.C_ABI_SYMBOLS
