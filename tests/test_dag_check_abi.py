"""ABI of verify mode on the dataflow schedule (bce_dag_set_checks / bce_dag_set_expected; report and log are the
context's bce_check_reset / bce_check_get): declared in bce_gpu.h, exported by libbce_amd.so, bound by the package; calls
without a context are status codes; the driver and the context have the methods the path is reached through.  No GPU
needed."""
import ctypes as C
import os
import re

from conftest import ROOT

ENGINE = ["bce_dag_set_checks", "bce_dag_set_expected"]
REPORT = ["bce_check_reset", "bce_check_get"]          # shared with the plan's checks


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(bce_[a-z0-9_]+)\s*\(", src))


def test_dag_check_symbols_are_declared_exported_and_bound(bce):
    bce.build()
    L = bce.lib()
    assert set(ENGINE + REPORT) <= _declared("bce_gpu.h")
    for n in ENGINE + REPORT:
        assert hasattr(L, n), "libbce_amd.so does not export %s" % n
    assert set(ENGINE + REPORT) <= set(bce.ENGINE_SYMBOLS)
    assert L.bce_dag_set_checks.argtypes is not None and len(L.bce_dag_set_checks.argtypes) == 5
    assert L.bce_dag_set_expected.argtypes is not None and len(L.bce_dag_set_expected.argtypes) == 4


def test_null_context_calls_are_argument_errors(bce):
    L = bce.lib()
    tasks, bits = (C.c_uint32 * 1)(0), (C.c_uint8 * 1)(0)
    assert L.bce_dag_set_checks(None, None, 1, tasks, 1) == bce.ERR_ARG
    assert L.bce_dag_set_checks(None, None, 0, None, 0) == bce.ERR_ARG
    assert L.bce_dag_set_expected(None, None, 1, bits) == bce.ERR_ARG


def test_the_driver_and_the_context_have_the_methods(bce):
    for m in ("dag_set_checks", "dag_set_expected", "dag_create", "dag_run", "check_reset", "check_get"):
        assert hasattr(bce.BinFHEContext, m), m
    for m in ("setDataflow", "setDeviceVerify", "setVerify", "dataflowActive", "deviceVerifyActive", "check_report"):
        assert hasattr(bce.Circuit, m), m


def test_the_three_opt_ins_need_an_engine(bce):
    """a plaintext-only circuit: the knobs are remembered, neither path is active without an engine"""
    c = bce.Circuit()
    c.ReadFile(os.path.join(ROOT, "tests", "golden", "circuits", "adder_2bit.out"))
    c.setDataflow(True)
    c.setDeviceVerify(True)
    c.Reset()
    c.setPlaintext(True)
    assert not c.dataflowActive() and not c.deviceVerifyActive()
    c.SetInput([[1, 0], [1, 1]])
    out = c.Clock()[0]
    assert out[0] + 2 * out[1] + 4 * out[2] == 4
    assert c.check_report()["checked"] == 0
