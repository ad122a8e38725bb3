"""Circuit.setDeviceVerify: verify mode (the reference's harnesses all run with setVerify(true): decrypt every gate output,
compare with the plaintext pass, "Bad <OP> fixing", replace -- src/gate.cpp:153-160) with the check on the device, between
the steps of the bootstrap-depth schedule, step by step and under setGraph.  Opt-in: setVerify alone keeps the host path."""
import os

import numpy as np
import pytest

import kat
import noise_model as nm
from kat import CIRCUITS

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED


@pytest.fixture(scope="module")
def toy_dv(bce):
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(SEED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std_dv(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    yield c
    c.close()


@pytest.mark.parametrize("graph", [False, True])
def test_injected_fault_is_repaired_on_the_bootstrap_depth_schedule(bce, toy_dv, graph, capfd):
    """the fault of test_verify_mode_repairs_an_injected_fault: input register R0 re-encrypted with the wrong bit"""
    c = bce.Circuit(toy_dv)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setDeviceVerify(True)
    c.setGraph(graph)
    c.Reset()
    assert not c.deviceVerifyActive()                      # verify is not on yet
    c.setVerify(True)
    assert c.deviceVerifyActive() and c.graphActive() == graph and not c.dataflowActive()
    c.SetInput([[1, 0], [1, 1]])                           # a = 1, b = 3
    toy_dv.Encrypt([0], [0], enc_index_base=123456)        # R0 (a bit 0) now encrypts 0 instead of 1
    for rep_no in range(2):                                # the second Clock() reuses the plan (and replays the graph)
        if rep_no:
            c.Rearm()
        capfd.readouterr()
        out = c.Clock()[0]
        err = capfd.readouterr().err
        assert out[0] + 2 * out[1] + 4 * out[2] == 4
        st, rep = c.stats(), c.check_report()
        assert st["verify_fixes"] == rep["mismatches"] >= 1 and rep["repaired"] == rep["mismatches"]
        assert err.count("Bad ") == rep["mismatches"] and "Bad OUTPUT fixing" not in err
        assert "Bad XOR fixing" in err and "Bad AND fixing" in err      # R4 = XOR(R0, R2) and R5 = AND(R0, R2)
        assert st["levels"] == len(c.relevel_steps()), "the run left the bootstrap-depth schedule"
        assert st["sublaunches"] == len(c.relevel_steps())                # one launch per step: no stage A / stage B rounds
        assert rep["checked"] == 7 and st["bootstraps"] == 13           # 3 XOR + 3 AND + 1 OR outputs; temporaries unchecked
    c.close()


def test_adder_64bit_without_fault_is_the_verify_off_run(bce, std_dv):
    """STD128_OPT, K = 2, seeded inputs: every register of both instances is the ciphertext the verify-off run leaves there
    (nothing was repaired, the checks perturb nothing), outputs equal, and the measured noise is the model's: every checked
    register is the output of a bootstrap of a tabulated set (noise_model.check_report: second moment in the band for this
    sample size, no error beyond 6.5 sigma)"""
    cc = std_dv
    path = os.path.join(CIRCUITS, "adder_64bit.txt")
    K = 2
    cases = [kat.adder_case(t, 64) for t in range(K)]
    snap, outs = {}, {}
    for mode in ("off", "device"):
        c = bce.Circuit(cc)
        c.ReadBristol(path)
        c.setInstances(K)
        c.setDeviceVerify(mode == "device")
        c.Reset()
        if mode == "device":
            c.setVerify(True)
        else:
            c.setEncrypted(True)
        assert c.deviceVerifyActive() == (mode == "device")
        info = c.info()
        W, stride = info["n_wires"], info["slot_stride"]
        cc.pool_reserve(K * stride)
        cc.lwe_write(np.arange(K * stride, dtype=np.uint32), np.zeros((K * stride, cc.n + 1), dtype=np.uint64))
        cc.set_encrypt_seed(SEED)
        for k, (ins, _) in enumerate(cases):
            c.SetInput(ins, instance=k)
        cc.set_encrypt_seed(None)
        c.Clock()
        outs[mode] = [c.Outputs(k) for k in range(K)]
        for k, (_, want) in enumerate(cases):
            assert outs[mode][k][0] == want, (mode, k)
        snap[mode] = np.concatenate([cc.lwe_read(np.arange(k * stride, k * stride + W, dtype=np.uint32)) for k in range(K)])
        if mode == "device":
            st, rep = c.stats(), c.check_report()
            assert rep["mismatches"] == 0 and rep["repaired"] == 0 and st["verify_fixes"] == 0
            assert rep["checked"] == K * (c.counts()["and"] + c.counts()["or"] + c.counts()["xor"]) > 0
            ratio = nm.check_report(rep, nm.model(cc.params, *cc.export_sk())["V_out"])
            print("adder_64bit K = %d: %d checked, noise_rms %.3f, measured / model %.3f, margin %d" % (K, rep["checked"], rep["noise_rms"], ratio, rep["margin"]))
            assert rep["margin"] > 0 and rep["checked"] >= 200
            assert st["levels"] == len(c.relevel_steps()) == 127
        c.close()
    assert outs["off"] == outs["device"]
    assert np.array_equal(snap["off"], snap["device"]), "device verify changed a ciphertext of a fault-free run"


def test_without_the_opt_in_verify_keeps_the_host_path(bce, toy_dv):
    c = bce.Circuit(toy_dv)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.Reset()
    c.setVerify(True)
    assert not c.deviceVerifyActive() and not c.graphActive()
    c.SetInput([[1, 0], [1, 1]])
    out = c.Clock()[0]
    assert out[0] + 2 * out[1] + 4 * out[2] == 4
    assert c.stats()["levels"] == c.info()["n_levels"]                               # the gate-level rounds ...
    assert c.stats()["sublaunches"] == c.info()["n_sublaunches"] > len(c.relevel_steps())   # ... with their two stages per level
    assert c.check_report()["checked"] == 0
    # the opt-in is also inactive where the host path is the only one: one Gate::Evaluate per gate, gate-level schedule
    for knob in ("batched", "relevel"):
        c.Reset()
        c.setDeviceVerify(True)
        c.setBatched(knob != "batched")
        c.setRelevel(knob != "relevel")
        c.setVerify(True)
        assert not c.deviceVerifyActive()
        c.SetInput([[1, 0], [1, 1]])
        out = c.Clock()[0]
        assert out[0] + 2 * out[1] + 4 * out[2] == 4 and c.stats()["levels"] == c.info()["n_levels"]
    c.close()
