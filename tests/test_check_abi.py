"""ABI of device-side verify mode (bce_check_*, bce_plan_set_checks / _set_expected, bce_circuit_set_device_verify ...):
declared in the headers, exported by libbce_amd.so, bound by the package; the ctypes mirrors of the two structs have the
size the C compiler gives them; calls without a context are status codes.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

ENGINE = ["bce_check_slots", "bce_plan_set_checks", "bce_plan_set_expected", "bce_check_reset", "bce_check_get"]
CIRCUIT = ["bce_circuit_set_device_verify", "bce_circuit_device_verify_active", "bce_circuit_get_check_report"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(bce_[a-z0-9_]+)\s*\(", src))


def test_check_symbols_are_declared_exported_and_bound(bce):
    bce.build()
    L = bce.lib()
    assert set(ENGINE) <= _declared("bce_gpu.h")
    assert set(CIRCUIT) <= _declared("bce_circuit.h")
    for n in ENGINE + CIRCUIT:
        assert hasattr(L, n), "libbce_amd.so does not export %s" % n
    assert set(ENGINE) <= set(bce.ENGINE_SYMBOLS)
    assert set(CIRCUIT) <= set(bce.CIRCUIT_SYMBOLS)
    for m in ("setDeviceVerify", "deviceVerifyActive", "check_report"):
        assert hasattr(bce.Circuit, m)
    for m in ("check_slots", "plan_set_checks", "plan_set_expected", "check_reset", "check_get"):
        assert hasattr(bce.BinFHEContext, m)


def test_struct_sizes_match_the_c_compiler(bce, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bce_circuit.h"\n'
                     'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(bce_check_report), sizeof(bce_check_entry),\n'
                     '    offsetof(bce_check_report, max_abs_err), offsetof(bce_check_entry, err), offsetof(bce_check_entry, got),\n'
                     '    (int)BCE_CHECK_LOG_CAP); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(bce.CheckReport), C.sizeof(bce.CheckEntry), bce.CheckReport.max_abs_err.offset,
                   bce.CheckEntry.err.offset, bce.CheckEntry.got.offset, bce.CHECK_LOG_CAP]
    assert got[:2] == [48, 24]


def test_null_context_calls_are_argument_errors(bce):
    L = bce.lib()
    bce._bind_circuit()
    r, e = bce.CheckReport(), bce.CheckEntry()
    slots, bits = (C.c_uint32 * 1)(0), (C.c_uint8 * 1)(0)
    assert L.bce_check_slots(None, 1, slots, bits, 1, 0, 0, 0) == bce.ERR_ARG
    assert L.bce_plan_set_checks(None, None, slots, slots, 0) == bce.ERR_ARG
    assert L.bce_plan_set_expected(None, None, bits) == bce.ERR_ARG
    assert L.bce_check_reset(None) == bce.ERR_ARG
    assert L.bce_check_get(None, C.byref(r), C.byref(e), 1) == bce.ERR_ARG
    assert L.bce_circuit_set_device_verify(None, 1) == bce.ERR_ARG
    assert L.bce_circuit_device_verify_active(None) == 0
    assert L.bce_circuit_get_check_report(None, C.byref(r)) == bce.ERR_ARG


def test_device_verify_is_off_by_default_and_needs_an_engine(bce):
    """a plaintext-only circuit: the knob is remembered, the path is never active (no engine), the report is all zero"""
    c = bce.Circuit()
    c.ReadFile(os.path.join(ROOT, "tests", "golden", "circuits", "adder_2bit.out"))
    assert not c.deviceVerifyActive()
    c.setDeviceVerify(True)
    c.Reset()
    c.setPlaintext(True)
    assert not c.deviceVerifyActive()
    c.SetInput([[1, 0], [1, 1]])
    out = c.Clock()[0]
    assert out[0] + 2 * out[1] + 4 * out[2] == 4
    rep = c.check_report()
    assert rep["checked"] == 0 and rep["mismatches"] == 0
