"""Circuit.setDataflowShared on the device: setXorShared's lowering (a PAIR(OR, NAND) task and an AND per XOR, two blind
rotations instead of three) on the dataflow schedule (one persistent launch per Clock(), bce_dag_create_pairs).

Parity bar: every netlist gate register holds the ciphertext the step schedule of the same lowering leaves there on the same
seeded input ciphertexts (tests/test_gpu_xor_shared.py pins that one to an oracle replay), outputs equal the plaintext
evaluation / the reference's vectors, and the counters show the pairs as one bootstrap each."""
import os
import random

import numpy as np
import pytest

import kat
from kat import CIRCUITS
from test_random_circuits import random_netlist

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED


@pytest.fixture(scope="module")
def std(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    assert c.dag_supported()
    yield c
    c.close()


def _dag_launches(t):
    return sum(k["launches"] for k in t["by_kernel"] if "dag" in k["kernel"])


def _circuit(bce, cc, read, K, mode, verify=False):
    c = bce.Circuit(cc)
    read(c)
    c.setInstances(K)
    c.setXorShared(True)
    if mode == "dataflow":
        c.setDataflow(True)
        c.setDataflowShared(True)
    if verify:
        c.setDeviceVerify(True)
    c.Reset()
    if verify:
        c.setVerify(True)
    else:
        c.setEncrypted(True)
    return c


def test_adder_2bit_all_16_inputs_registers_equal_the_step_schedule(bce, std):
    cc = std
    K = 16
    read = lambda c: c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    regs = np.arange(4, 11, dtype=np.uint32)                       # R4..R10: the seven gate registers of the netlist
    snap = {}
    for mode, verify in (("steps", False), ("dataflow", False), ("dataflow", True)):
        c = _circuit(bce, cc, read, K, mode, verify)
        stride = c.info()["slot_stride"]
        assert c.xorSharedActive() and c.dataflowActive() == (mode == "dataflow") and c.deviceVerifyActive() == verify
        assert c.info()["n_bootstraps"] == 10
        if mode == "dataflow":
            tasks, _ = c.dataflow_plan()
            assert len(tasks) == 10 and sum(1 for t in tasks if t[0] >> 8) == 3
        cc.pool_reserve(K * stride)
        cc.set_encrypt_seed(SEED)                                  # every circuit draws the same input ciphertexts
        for k in range(K):
            a, b = k & 3, k >> 2
            c.SetInput([[a & 1, a >> 1], [b & 1, b >> 1]], instance=k)
        cc.set_encrypt_seed(None)
        where = np.concatenate([regs + k * stride for k in range(K)])
        cc.lwe_write(where, np.zeros((where.size, cc.n + 1), dtype=np.uint64))
        t0 = cc.timing()
        c.Clock()
        t1 = cc.timing()
        for k in range(K):
            o = c.Outputs(k)[0]
            assert o[0] + 2 * o[1] + 4 * o[2] == (k & 3) + (k >> 2), (mode, verify, k)
        st = c.stats()
        assert st["bootstraps"] == 10 * K and st["verify_fixes"] == 0, st
        if mode == "dataflow":
            assert _dag_launches(t1) - _dag_launches(t0) == 1 and t1["blind_rotate_launches"] - t0["blind_rotate_launches"] == 1
            assert st["sublaunches"] == 1 and cc.dag_last_run()["done"] == 10 * K
        if verify:
            rep = c.check_report()
            assert rep["checked"] == 7 * K and rep["mismatches"] == 0 and rep["repaired"] == 0, rep   # the AND tasks, not the pairs
        snap[(mode, verify)] = cc.lwe_read(where)
        c.close()
    assert snap[("steps", False)].any(axis=1).all()
    assert np.array_equal(snap[("steps", False)], snap[("dataflow", False)]), "dataflow + shared left other gate registers than steps + shared"
    assert np.array_equal(snap[("steps", False)], snap[("dataflow", True)]), "... under device verify"


@pytest.mark.parametrize("seed", range(4))
def test_random_netlists_dataflow_shared_equals_step_schedule_and_plaintext(bce, tmp_path, std, seed):
    """as test_random_netlists_dataflow_equals_step_schedule_and_plaintext: NOT chains, constants, MAND, wire copies; K = 3"""
    cc = std
    rnd = random.Random(9100 + seed)
    text, in_w, out_w, evaluate = random_netlist(rnd, rnd.randint(20, 70))
    path = tmp_path / "rand.txt"
    path.write_text(text)
    K = 3
    ins = [[[rnd.randint(0, 1) for _ in range(w)] for w in in_w] for _ in range(K)]
    snap = {}
    cc.set_encrypt_seed(SEED + seed)
    for mode in ("steps", "dataflow"):
        c = _circuit(bce, cc, lambda c: c.ReadBristol(str(path), new_flag=True), K, mode)
        info = c.info()
        W, stride = info["n_wires"], info["slot_stride"]
        assert c.xorSharedActive() and c.dataflowActive() == (mode == "dataflow")
        cc.pool_reserve(K * stride)
        cc.lwe_write(np.arange(K * stride, dtype=np.uint32), np.zeros((K * stride, cc.n + 1), dtype=np.uint64))
        for k in range(K):
            c.SetInput(ins[k], instance=k)
        c.Clock()
        for k in range(K):
            assert c.Outputs(k) == evaluate(ins[k]), "instance %d, %s" % (k, mode)
        assert c.stats()["bootstraps"] == info["n_bootstraps"] * K
        # all netlist registers of the K instances: registers nobody writes stayed zero under both schedules
        snap[mode] = np.concatenate([cc.lwe_read(np.arange(k * stride, k * stride + W, dtype=np.uint32)) for k in range(K)])
        c.close()
    cc.set_encrypt_seed(None)
    assert np.array_equal(snap["steps"], snap["dataflow"])


def test_aes_expanded_two_vectors(bce, std):
    cc = std
    path = os.path.join(CIRCUITS, "AES-expanded.txt")
    vecs = [v for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"][:2]
    K = len(vecs)
    lines = [l.split() for l in open(path) if l.strip()]
    n_in = int(lines[1][0]) + int(lines[1][1])
    boot = np.array([n_in + gi for gi, t in enumerate(lines[2:]) if t[-1] in ("AND", "XOR")], dtype=np.uint32)
    assert boot.size == 20325 + 5440
    snap = {}
    cc.set_encrypt_seed(SEED)
    for mode in ("steps", "dataflow"):
        c = _circuit(bce, cc, lambda c: c.ReadBristol(path), K, mode)
        stride = c.info()["slot_stride"]
        for k, v in enumerate(vecs):
            c.SetInput(kat.aes_case(v)[0], instance=k)
        assert c.xorSharedActive() and c.dataflowActive() == (mode == "dataflow")
        c.Clock()
        for k, v in enumerate(vecs):
            assert c.Outputs(k)[0] == kat.aes_case(v)[1], (mode, k)
        st = c.stats()
        assert st["bootstraps"] == 46090 * K and (st["sublaunches"] == 1 if mode == "dataflow" else st["levels"] == 416), (mode, st)
        snap[mode] = cc.lwe_read(np.concatenate([boot, boot + stride]))
        c.close()
    cc.set_encrypt_seed(None)
    assert np.array_equal(snap["steps"], snap["dataflow"]), "dataflow + shared AES gate registers differ from the step schedule's"
