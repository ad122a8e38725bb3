"""The derivation of a context stands alone: tests/integration/ctx_params_selftest.cpp is compiled together with
csrc/ctx_params.cpp ONLY (no HIP runtime, no kernels, no libbce_amd.so; kernel_class is scripted by the self-test) by the host
compiler, with AddressSanitizer and UndefinedBehaviorSanitizer where the compiler has their runtimes, and run as a program of
its own: valid shapes out to Q = 2^40 - 1, baseG = 2^31 and qKS = 2^32 - 1, every rejected argument, and what kernel_class
reports (no kernel, LDS does not fit, no folded build, LDS bytes) reaching the caller."""
import os
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "tests", "integration", "ctx_params_selftest.cpp")
MODULE = os.path.join(ROOT, "openfhe-boolean-circuit-evaluator_amd", "csrc", "ctx_params.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# csrc/kernels.hpp (for DevParams and KernelClass) also includes the HIP header with the launch templates of hipcc's own
# syntax, which a host compiler cannot read: its include guard is predefined, the module uses nothing of it
HIPCC_ONLY = "-DHIP_INCLUDE_HIP_HIP_EXT_H"
# the runtimes linked statically first: the program then also starts where the environment preloads some other library
ATTEMPTS = [SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []]


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    return None


def test_context_derivation_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    inc = _rocm_include()
    if cxx is None or inc is None:
        pytest.skip("no host C++ compiler, or no HIP headers")
    exe = str(tmp_path / "ctx_params_selftest")
    for flags in ATTEMPTS:   # a host compiler without sanitizer runtimes fails to link with them: then build without
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", HIPCC_ONLY, "-I" + inc]
                               + flags + [SELFTEST, MODULE, "-o", exe], capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-2000:]
    print("built with", flags or "no sanitizer (none available)")
    t0 = time.perf_counter()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    took = time.perf_counter() - t0
    assert r.returncode == 0 and "ctx_params selftest ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    assert took < 1.0, "the self-test is meant to run in under a second, took %.2f s" % took
