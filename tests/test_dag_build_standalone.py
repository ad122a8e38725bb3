"""The dependency analysis of the dataflow schedule stands alone: tests/integration/dag_build_selftest.cpp is compiled together
with csrc/dag_build.cpp and csrc/schedule.cpp ONLY (no engine, no libbce_amd.so, no HIP header) by the host compiler, with the
sanitizer flags and fallbacks of tests/test_schedule_dataflow_shared_standalone.py, and run as a program of its own:
hand-written task lists with the exact arrays the engine uploads, random lists against a brute-force model, every refusal of
bce_dag_create / bce_dag_create_pairs with its code and text, and the descriptor classifier (csrc/desc.hpp) over every op."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openfhe-boolean-circuit-evaluator_amd", "csrc")
SELFTEST = os.path.join(ROOT, "tests", "integration", "dag_build_selftest.cpp")
MODULES = [os.path.join(CSRC, "dag_build.cpp"), os.path.join(CSRC, "schedule.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the runtimes linked statically first: the program then also starts where the environment preloads some other library
ATTEMPTS = [SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []]


def test_dag_build_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dag_build_selftest")
    for flags in ATTEMPTS:   # a host compiler without sanitizer runtimes fails to link with them: then build without
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [SELFTEST] + MODULES + ["-o", exe],
                               capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-2000:]
    print("built with", flags or "no sanitizer (none available)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dag build selftest ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_the_modules_include_no_device_header():
    """dag_build and desc are host-only: nothing of HIP, and not kernels.hpp (the class count is an argument)"""
    for name in ("dag_build.hpp", "dag_build.cpp", "desc.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        includes = [line for line in text.splitlines() if line.startswith("#include")]
        assert includes and not [i for i in includes if "hip" in i or "kernels.hpp" in i or "devmem.hpp" in i], (name, includes)
