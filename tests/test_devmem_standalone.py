"""The owners of the engine's device memory stand alone: tests/integration/devmem_selftest.cpp includes csrc/devmem.hpp,
defines the ten HIP entry points the header calls on top of malloc (live allocations, a log of the calls, a switch that fails
the k-th call) and is compiled by the host compiler WITHOUT the HIP runtime, with AddressSanitizer and
UndefinedBehaviorSanitizer where the compiler has their runtimes, and run as a program of its own: nothing stays allocated
after any life of a buffer, a growth waits once and allocates what the caller's policy says, a reserve that has room makes no
call, every single failed call leaves an empty object that works again, the busy event is waited for once, and send delivers
the bytes."""
import os
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "tests", "integration", "devmem_selftest.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the runtimes linked statically first: the program then also starts where the environment preloads some other library
ATTEMPTS = [SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []]


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    return None


def test_device_memory_owners_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    inc = _rocm_include()
    if cxx is None or inc is None:
        pytest.skip("no host C++ compiler, or no HIP headers")
    exe = str(tmp_path / "devmem_selftest")
    for flags in ATTEMPTS:   # a host compiler without sanitizer runtimes fails to link with them: then build without
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I" + inc]
                               + flags + [SELFTEST, "-o", exe], capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-2000:]
    print("built with", flags or "no sanitizer (none available)")
    t0 = time.perf_counter()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    took = time.perf_counter() - t0
    assert r.returncode == 0 and "devmem selftest ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert took < 1.0, "the self-test is meant to run in well under a second, took %.2f s" % took
