"""Circuit.setXorShared on the device: XOR = AND(OR, NAND) with the OR and the NAND from one blind rotation (a PAIR descriptor
per XOR, tests/test_gpu_pairs.py pins those).  Circuits against their plaintext evaluation, the reference's vectors and an
oracle replay; stepped, as one graph and under device verify; and the noise of the two outputs of a pair, alone and as the
sum the consuming AND sees, against tests/noise_model.py."""
import math
import os

import numpy as np
import pytest

import kat
import noise_model as nm
import noise_run
import pair_model as pm
from kat import CIRCUITS

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED


@pytest.fixture(scope="module")
def toy_cc(bce):
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(SEED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std_cc(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    yield c
    c.close()


# ---- circuits ----------------------------------------------------------------------------------------------------------------------
def test_adder_2bit_toy_all_inputs_against_an_oracle_replay(bce, orc, toy_cc):
    """All 16 inputs.  The schedule's own descriptors (Circuit.relevel_plan: slots, temporaries and neg flags as Clock() hands
    them to the engine) are replayed on the oracle, pairs through pair_model.eval_desc, and run on the device one step at a time
    (a plan of the same descriptors), so that EVERY slot a step writes -- the XOR temporaries t, t + 1 before their bank is
    reused, and the netlist registers -- is compared word for word.  Then Clock() itself: outputs, counters, and every netlist
    register equal to the replay's."""
    o = orc.Oracle(orc.TOY, orc.GINX)
    o.keygen(SEED)
    assert np.array_equal(toy_cc.export_sk()[0], o.sk())
    c = bce.Circuit(toy_cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setXorShared(True)
    info = c.info()
    W, stride = info["n_wires"], info["slot_stride"]
    assert c.xorSharedActive() and info["n_bootstraps"] == 10 and len(c.relevel_steps()) == 4
    steps = c.relevel_plan()
    assert [len(st) for st in steps] == c.relevel_steps() and sum(len(st) for st in steps) == 10
    pairs = [d for st in steps for d in st if d[0] >> 8]
    assert len(pairs) == 3 and all(d[0] == bce.PAIR(bce.OR, bce.NAND) and d[3] >= W and d[3] + 1 < stride for d in pairs)
    written = lambda d: [d[3], d[3] + 1] if d[0] >> 8 else [d[3]]
    toy_cc.pool_reserve(stride)
    for a in range(4):
        for b in range(4):
            c.Reset()
            c.setEncrypted(True)
            c.SetInput([[a & 1, a >> 1], [b & 1, b >> 1]])
            what = "a = %d, b = %d" % (a, b)
            pool = dict(enumerate(toy_cc.lwe_read(np.arange(0, 4, dtype=np.uint32))))     # the input registers
            plan = toy_cc.plan_create(steps)
            for s, st in enumerate(steps):
                toy_cc.plan_run_step(plan, s)
                for d in st:
                    pm.eval_desc(o, pool, d)
                slots = [w for d in st for w in written(d)]
                got = toy_cc.lwe_read(np.array(slots, dtype=np.uint32))
                for w, ct in zip(slots, got):
                    assert np.array_equal(ct, pool[w]), "%s: step %d, slot %d differs from the oracle replay" % (what, s, w)
            toy_cc.plan_destroy(plan)
            regs = sorted(w for st in steps for d in st for w in written(d) if w < W)
            assert regs == list(range(4, 11))
            toy_cc.lwe_write(np.array(regs, dtype=np.uint32), np.zeros((len(regs), toy_cc.n + 1), dtype=np.uint64))
            out = c.Clock()[0]
            assert out[0] + 2 * out[1] + 4 * out[2] == a + b
            st = c.stats()
            assert st["bootstraps"] == 10 and st["levels"] == st["sublaunches"] == 4 and st["verify_fixes"] == 0
            got = toy_cc.lwe_read(np.array(regs, dtype=np.uint32))
            for w, ct in zip(regs, got):
                assert np.array_equal(ct, pool[w]), "%s: Clock() left another ciphertext in register R%d than the replay" % (what, w)
                assert o.decrypt(ct) == c_plain(a, b)[w], (what, w)
    c.close()


def c_plain(a, b):
    """plaintext values of the registers R0..R10 of adder_2bit.out (the netlist of test_gpu_circuit's oracle replay)"""
    R = [a & 1, a >> 1, b & 1, b >> 1]
    R += [R[0] ^ R[2], R[0] & R[2], R[1] ^ R[3], R[1] & R[3]]
    R += [R[5] ^ R[6], R[5] & R[6]]
    return R + [R[9] | R[7]]


def test_a_refused_switch_after_setinput_leaves_the_run_alone(bce, toy_cc):
    """Whether the lowering is active is fixed at SetInput (the pool is laid out for its schedule): a call that would switch
    it is refused, and Clock() runs the shared lowering on the encrypted inputs as if nothing had been asked."""
    c = bce.Circuit(toy_cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setXorShared(True)
    c.Reset()
    c.setEncrypted(True)
    c.SetInput([[1, 1], [0, 1]])             # 3 + 2
    for call in (lambda: c.setRelevel(False), lambda: c.setBatched(False), lambda: c.setVerify(True)):
        with pytest.raises(bce.BceError) as e:
            call()
        assert e.value.code == bce.ERR_STATE and c.xorSharedActive() and not c.getVerify()
    out = c.Clock()[0]
    assert out[0] + 2 * out[1] + 4 * out[2] == 5
    assert c.stats()["bootstraps"] == 10 and c.stats()["levels"] == 4
    c.close()


def test_adder_64bit_std128_device_verify(bce, std_cc):
    K = 4
    c = bce.Circuit(std_cc)
    c.ReadBristol(os.path.join(CIRCUITS, "adder_64bit.txt"))
    c.setInstances(K)
    c.setXorShared(True)
    c.setDeviceVerify(True)
    c.Reset()
    c.setVerify(True)
    assert c.deviceVerifyActive() and c.xorSharedActive()
    cases = [kat.adder_case(t, 64) for t in range(K)]
    for k, (ins, _) in enumerate(cases):
        c.SetInput(ins, instance=k)
    c.Clock()
    for k, (_, want) in enumerate(cases):
        assert c.Outputs(k)[0] == want, k
    st, rep, n = c.stats(), c.check_report(), c.counts()
    assert (n["and"], n["or"], n["xor"]) == (265, 0, 115)
    gates = 265 + 115
    assert rep["mismatches"] == 0 and rep["repaired"] == 0 and st["verify_fixes"] == 0
    assert rep["checked"] == gates * K                      # the same netlist wires as without the option; temporaries unchecked
    assert st["bootstraps"] == 495 * K and st["levels"] == len(c.relevel_steps()) == 127
    c.close()


def test_aes_expanded_std128_stepped_graph_and_dataflow_request(bce, std_cc):
    c = bce.Circuit(std_cc)
    c.ReadBristol(os.path.join(CIRCUITS, "AES-expanded.txt"))
    vecs = [v for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"][:2]
    K = len(vecs)
    assert K == 2
    c.setInstances(K)
    c.setXorShared(True)
    c.Reset()
    c.setEncrypted(True)
    for k, v in enumerate(vecs):
        c.SetInput(kat.aes_case(v)[0], instance=k)
    lines = [l.split() for l in open(os.path.join(CIRCUITS, "AES-expanded.txt")) if l.strip()]
    n_in = int(lines[1][0]) + int(lines[1][1])
    boot_regs = np.array([n_in + gi for gi, t in enumerate(lines[2:]) if t[-1] in ("AND", "XOR")], dtype=np.uint32)
    assert boot_regs.size == 20325 + 5440
    stride = c.info()["slot_stride"]
    regs = np.concatenate([boot_regs, boot_regs[::8] + stride])          # instance 0 whole, instance 1 sampled
    snaps = []
    for mode in ("stepped", "graph", "dataflow requested"):
        if mode != "stepped":
            c.Rearm()
        if mode == "graph":
            c.setGraph(True)
        if mode == "dataflow requested":
            c.setDataflow(True)
        assert c.xorSharedActive() and not c.dataflowActive() and c.graphActive() == (mode != "stepped")
        c.Clock()
        for k, v in enumerate(vecs):
            assert c.Outputs(k)[0] == kat.aes_case(v)[1], (mode, k)
        st = c.stats()
        assert st["bootstraps"] == 46090 * K and st["levels"] == 416, (mode, st)
        snaps.append(std_cc.lwe_read(regs))
    assert np.array_equal(snaps[0], snaps[1]), "graph replay left other ciphertexts than the stepped run"
    assert np.array_equal(snaps[0], snaps[2])
    c.close()


# ---- noise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["toy", "split", "STD128_OPT"])
def test_noise_of_both_outputs_and_of_their_sum(bce, orc, shape):
    """32,768 pairs (OR, NAND) on distinct random pairs of fresh inputs.  Each output's second moment within BAND of the
    model's V_out and no error beyond MAX_SIGMAS; the second moment of e1 + e2 -- what the consuming AND sees -- within BAND
    of 2 V_out (independent errors: the two tails share the accumulator's noise, rotated by X^e); then the ANDs: no wrong bit."""
    table = noise_run.shapes(orc.lib(), bce.TOY)
    paramset, custom, _ = table.get(shape, (bce.STD128_OPT, None, None))
    c = bce.BinFHEContext(paramset, bce.GINX) if custom is None else bce.BinFHEContext(method=bce.GINX, custom=custom)
    c.KeyGen(SEED)
    p = c.params
    s, z = c.export_sk()
    V = nm.model(p, s, z)["V_out"]
    M, n_in = 32768, 1024
    rng = np.random.default_rng(31)
    c.pool_reserve(n_in + 3 * M)
    bits = noise_run.fresh_inputs(c, rng, n_in)
    _, in0, in1 = nm.random_gates(rng, M, n_in)
    t = n_in + 2 * np.arange(M)
    op = np.full(M, bce.PAIR(bce.OR, bce.NAND))
    for o in range(0, M, noise_run.LAUNCH):
        sl = slice(o, o + noise_run.LAUNCH)
        c.EvalGates(noise_run.desc_array(bce.GateDesc, op[sl], in0[sl], in1[sl], t[sl]))
    a, b = bits[in0], bits[in1]
    e = []
    for second, want in ((0, a | b), (1, 1 - (a & b))):
        err = np.concatenate([nm.lwe_phase_error(c.lwe_read((t[o:o + 8192] + second).astype(np.uint32)), s, p["q"], want[o:o + 8192])
                              for o in range(0, M, 8192)]).astype(np.float64)
        e.append(err)
    m2 = [float(np.mean(x * x)) for x in e]
    m2_sum = float(np.mean((e[0] + e[1]) ** 2))
    corr = float(np.mean(e[0] * e[1]) / math.sqrt(m2[0] * m2[1]))
    worst = max(float(np.abs(x).max()) for x in e) / math.sqrt(V)
    print("%s: V_out %.3f; second moments %.3f, %.3f (ratios %.3f, %.3f); of the sum %.3f = %.3f x 2 V_out; correlation %+.4f; max |e| %.2f sigma"
          % (shape, V, m2[0], m2[1], m2[0] / V, m2[1] / V, m2_sum, m2_sum / (2 * V), corr, worst))
    for k in range(2):
        assert nm.BAND[0] <= m2[k] / V <= nm.BAND[1], (shape, k, m2[k] / V)
    assert worst <= nm.MAX_SIGMAS
    assert nm.BAND[0] <= m2_sum / (2 * V) <= nm.BAND[1], (shape, m2_sum / (2 * V))
    out = n_in + 2 * M + np.arange(M)
    for o in range(0, M, noise_run.LAUNCH):
        sl = slice(o, o + noise_run.LAUNCH)
        c.EvalGates(noise_run.desc_array(bce.GateDesc, np.full(len(t[sl]), bce.AND), t[sl], t[sl] + 1, out[sl]))
    got = np.asarray(c.Decrypt(out.astype(np.uint32)), dtype=np.int64)
    assert int((got != (a ^ b)).sum()) == 0
    c.close()
