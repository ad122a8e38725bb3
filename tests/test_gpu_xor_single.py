"""BCE_XOR (include/bce_gpu.h) on the device: XOR in one bootstrap of ct1 + ct2 with a three-level test polynomial, against the
reference of tests/xor_single_model.py (the blind rotation restated from the oracle's primitives, anchored to the oracle in
tests/test_xor_single_model.py), word for word at every stage, on every kernel family and both tails; in one call with plain
gates, a pair and a refresh, as a plan and as a dag; through the Circuit driver (setXorSingle) on the step, graph and dataflow
schedules with device verify; and its noise against the plain-gate prediction of tests/noise_model.py.  Shapes are the cheap
ones of noise_run.shapes (n = 32 / 16)."""
import hashlib
import math
import os

import numpy as np
import pytest

import kat
import noise_model as nm
import noise_run
import xor_single_model as xm
from kat import CIRCUITS
from test_circuit_xor_single import parity_vectors

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED


@pytest.fixture(scope="module")
def oracles(bce, orc):
    """one keyed oracle per (shape or tabulated set, method), made on first use"""
    table = noise_run.shapes(orc.lib(), None)
    made = {}

    def get(shape, method):
        if (shape, method) not in made:
            custom = table[shape][1] if shape in table else None
            o = orc.Oracle(method=getattr(orc, method), custom=custom) if custom else orc.Oracle(getattr(orc, shape), getattr(orc, method))
            o.keygen(SEED)
            made[(shape, method)] = (o, custom)
        return made[(shape, method)]

    return get


def _engine(bce, oracles, shape, method):
    o, custom = oracles(shape, method)
    c = bce.BinFHEContext(method=getattr(bce, method), custom=custom) if custom else bce.BinFHEContext(getattr(bce, shape), getattr(bce, method))
    assert c.params == o.params
    c.import_keys(o.sk(), o.z(), o.bsk(), o.ksk())
    return o, c


_CASES, _REF = {}, {}     # cases and their references are made once per oracle and shared by the tests that meet them again


def _cases(o):
    """the 16 cases (a, b, neg0, neg1, ca, cb): 4 inputs x 4 combinations of folded NOTs, fresh oracle encryptions"""
    if id(o) not in _CASES:
        _CASES[id(o)] = [(a, b, n0, n1, o.encrypt(a, 2000 + 2 * k), o.encrypt(b, 2001 + 2 * k))
                         for k, (a, b, n0, n1) in enumerate((a, b, n0, n1) for a in (0, 1) for b in (0, 1) for n0 in (0, 1) for n1 in (0, 1))]
    return _CASES[id(o)]


def _reference(o, case):
    a, b, n0, n1, ca, cb = case
    key = (id(o), n0, n1, ca.tobytes(), cb.tobytes())
    if key not in _REF:
        _REF[key] = xm.stages(o, ca, cb, n0, n1)
    return _REF[key]


def _load(c, cases, extra=0):
    """inputs of case i in slots 2i, 2i + 1; its output in slot 2 nb + i"""
    nb = len(cases)
    c.pool_reserve(3 * nb + extra)
    c.lwe_write(np.arange(2 * nb, dtype=np.uint32), np.concatenate([np.stack([x[4], x[5]]) for x in cases]))
    return [(xm.XOR, 2 * i, 2 * i + 1, 2 * nb + i, x[2], x[3]) for i, x in enumerate(cases)]


def _run(c, descs):
    nb = len(descs)
    t0 = c.timing()["bootstraps"]
    acc, lweN, ks = c.debug_eval_stages(descs)
    assert c.timing()["bootstraps"] - t0 == nb                       # one bootstrap each
    assert acc.shape[0] == lweN.shape[0] == ks.shape[0] == nb
    return acc, lweN, ks, c.lwe_read(np.arange(2 * nb, 3 * nb, dtype=np.uint32))


def _assert_reference(o, cases, acc, lweN, ks, out, what):
    for i, case in enumerate(cases):
        r = _reference(o, case)
        assert np.array_equal(acc[i], r["acc"]), "%s: accumulator, case %d" % (what, i)
        assert np.array_equal(lweN[i], r["lweN"]), "%s: extract + ModSwitch, case %d" % (what, i)
        assert np.array_equal(ks[i], r["ks"]), "%s: KeySwitch, case %d" % (what, i)
        assert np.array_equal(out[i], r["out"]), "%s: pool row, case %d" % (what, i)
        assert o.decrypt(out[i]) == (case[0] ^ case[2]) ^ (case[1] ^ case[3]), (what, i)


# ---- 1. every stage, word for word, on every kernel family (lone launches: the separate tail kernels) ------------------------------
@pytest.mark.parametrize("shape,method,env", [
    ("TOY", "GINX", {}), ("TOY", "AP", {}),
    ("split", "GINX", {"BCE_VARIANT": "1"}), ("split", "GINX", {"BCE_VARIANT": "2"}), ("split", "GINX", {"BCE_VARIANT": "3"}), ("split", "AP", {}),
    ("std256_like", "GINX", {}),
    ("std192_like", "AP", {"BCE_FP64": "1"}), ("std192_like", "GINX", {"BCE_FP64": "1"}),
    ("std192_like", "AP", {"BCE_FP64": "0"}), ("std192_like", "GINX", {"BCE_FP64": "0"}),
    ("int64_40", "GINX", {})],
    ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) or "default" if isinstance(v, dict) else v)
def test_every_stage_matches_the_model(bce, oracles, shape, method, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    o, c = _engine(bce, oracles, shape, method)
    cases = _cases(o)
    assert len(cases) == 16
    acc, lweN, ks, out = _run(c, _load(c, cases))
    _assert_reference(o, cases, acc, lweN, ks, out, "%s %s %s" % (shape, method, env))
    assert list(c.Decrypt(np.arange(32, 48, dtype=np.uint32))) == [(x[0] ^ x[2]) ^ (x[1] ^ x[3]) for x in cases]
    c.close()


# ---- 2. the fused tail: a saturated launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,method", [("split", "GINX"), ("std192_like", "AP")])
def test_saturated_launch_runs_the_fused_tail(bce, oracles, shape, method, monkeypatch):
    monkeypatch.setenv("BCE_FP64", "1")          # (std192_like: the fp64 AP build carries its tail)
    o, c = _engine(bce, oracles, shape, method)
    cases = _cases(o)
    nb = len(cases)
    lone, full = c.launch_capacity()
    big_n = full + 16 - full % 16 + 16            # larger than `full`, a multiple of the 16 cases
    assert big_n > full and big_n % nb == 0
    descs = _load(c, cases, extra=big_n)
    big = [(d[0], d[1], d[2], 3 * nb + i, d[4], d[5]) for i in range(big_n) for d in [descs[i % nb]]]
    t0 = c.timing()["fused_tail_launches"]
    acc, lweN, ks = c.debug_eval_stages(big)
    assert c.timing()["fused_tail_launches"] == t0 + 1, "a saturated launch runs the tail in the epilogue"
    out = c.lwe_read(np.arange(3 * nb, 3 * nb + big_n, dtype=np.uint32))
    _assert_reference(o, cases, acc[:nb], lweN[:nb], ks[:nb], out[:nb], "%s %s fused" % (shape, method))
    for i in range(nb, big_n):
        k = i % nb
        assert np.array_equal(acc[i], acc[k]) and np.array_equal(lweN[i], lweN[k]) and np.array_equal(ks[i], ks[k]) and np.array_equal(out[i], out[k]), "gate %d" % i
    c.close()


# ---- 3. XOR, plain gates, a pair and a refresh in one call, with instances; as a plan and as a dag -----------------------------------
def test_mixed_call_plan_and_dag(bce, oracles):
    o, c = _engine(bce, oracles, "split", "GINX")
    K, stride = 3, 16
    c.pool_reserve(3 * K * stride)
    ins = []
    for k in range(K):
        a, b = k & 1, 1 - (k >> 1)
        ins.append((a, b, o.encrypt(a, 3000 + 2 * k), o.encrypt(b, 3001 + 2 * k)))
        for copy in range(3):
            base = (copy * K + k) * stride
            c.lwe_write([base, base + 1], np.stack([ins[k][2], ins[k][3]]))
    first = [(bce.XOR, 0, 1, 5), (bce.PAIR(bce.OR, bce.NAND), 0, 1, 6), (bce.AND, 0, 1, 8, 1, 0), (bce.OP_REFRESH, 0, 0, 9), (bce.XOR, 1, 0, 12, 1, 0)]
    second = [(bce.XOR, 5, 8, 10, 0, 1), (bce.AND, 6, 7, 11), (bce.XOR, 9, 12, 13, 1, 1)]
    regs = [5, 6, 7, 8, 9, 10, 11, 12, 13]
    read = lambda copy: c.lwe_read([(copy * K + k) * stride + s for k in range(K) for s in regs])
    # (a) two frontier calls
    t0 = c.timing()["bootstraps"]
    c.EvalGates(first, instances=K, slot_stride=stride)
    c.EvalGates(second, instances=K, slot_stride=stride)
    assert c.timing()["bootstraps"] - t0 == 8 * K          # blind rotations: the pair counts 1, every XOR 1
    called = read(0)
    # (b) a resident plan, step by step on copy 1, then as one graph on copy 1 again
    plan = c.plan_create([first, second], instances=K, slot_stride=stride, slot_base=K * stride)
    c.plan_run_step(plan, 0)
    c.plan_run_step(plan, 1)
    stepped = read(1)
    c.lwe_write([(K + k) * stride + s for k in range(K) for s in regs], np.zeros_like(stepped))
    c.plan_run(plan)
    graphed = read(1)
    c.plan_destroy(plan)
    # (c) the dataflow kernel on copy 2
    assert c.dag_supported()
    dag = c.dag_create(first + second, pairs=True)
    c.dag_run(dag, instances=K, slot_stride=stride, slot_base=2 * K * stride)
    flowed = read(2)
    c.dag_destroy(dag)
    assert np.array_equal(called, stepped) and np.array_equal(called, graphed) and np.array_equal(called, flowed)
    for k, (a, b, ca, cb) in enumerate(ins):
        pool = {0: ca, 1: cb}
        for d in first + second:
            xm.eval_desc(o, pool, d)
        for j, s in enumerate(regs):
            assert np.array_equal(called[k * len(regs) + j], pool[s]), "instance %d register %d" % (k, s)
        x = a ^ b
        assert [o.decrypt(pool[s]) for s in regs] == [x, a | b, 1 - (a & b), (1 - a) & b, a, x ^ (1 - ((1 - a) & b)), (a | b) & (1 - (a & b)), 1 - x,
                                                      (1 - a) ^ x]
    c.close()


# ---- 4. circuits ------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("path", ["steps", "graph", "dataflow", "levels", "per_gate"])
def test_adder_2bit_toy_all_inputs(bce, toy_cc, path):
    c = bce.Circuit(toy_cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setXorSingle(True)
    c.setGraph(path == "graph")
    c.setDataflow(path == "dataflow")
    c.setRelevel(path not in ("levels", "per_gate"))
    c.setBatched(path != "per_gate")
    assert c.info()["n_bootstraps"] == 7
    for a in range(4):
        for b in range(4):
            c.Reset()
            c.setEncrypted(True)
            c.SetInput([[a & 1, a >> 1], [b & 1, b >> 1]])
            assert c.dataflowActive() == (path == "dataflow" and toy_cc.dag_supported()) and c.graphActive() == (path == "graph")
            o = c.Clock()[0]
            assert o[0] + 2 * o[1] + 4 * o[2] == a + b, (path, a, b)
            st = c.stats()
            assert st["bootstraps"] == 7 and st["verify_fixes"] == 0
    c.close()


@pytest.mark.parametrize("verify", ["off", "host", "device", "device_dataflow"])
def test_parity_sixteen_vectors_in_lock_step(bce, toy_cc, verify):
    """parity.out has NOT gates in front of its XORs (the descriptors' flags) and one that feeds an OUTPUT; with verify every
    gate output -- the XORs' included: they are netlist wires -- is decrypted and compared, on the host or on the device"""
    vecs = parity_vectors(16)
    c = bce.Circuit(toy_cc)
    c.ReadFile(os.path.join(CIRCUITS, "parity.out"))
    c.setInstances(len(vecs))
    c.setXorSingle(True)
    c.setDeviceVerify(verify.startswith("device"))
    c.setDataflow(verify == "device_dataflow")
    c.Reset()
    if verify == "off":
        c.setEncrypted(True)
    else:
        c.setVerify(True)
    for k, (ins, _) in enumerate(vecs):
        c.SetInput(ins, instance=k)
    assert c.deviceVerifyActive() == verify.startswith("device") and c.dataflowActive() == (verify == "device_dataflow" and toy_cc.dag_supported())
    c.Clock()
    for k, (_, want) in enumerate(vecs):
        assert c.Outputs(k)[0] == want, (verify, k)
    n = c.counts()
    st = c.stats()
    assert st["verify_fixes"] == 0 and st["bootstraps"] == len(vecs) * (n["and"] + n["or"] + n["xor"])
    if verify.startswith("device"):
        rep = c.check_report()
        assert rep["checked"] == len(vecs) * (n["and"] + n["or"] + n["xor"]) and rep["mismatches"] == 0 and rep["repaired"] == 0
        assert 0 < rep["max_abs_err"] < toy_cc.params["q"] // 8
    c.close()


def test_aes_expanded_std128_two_blocks_on_both_schedules(bce, std_cc):
    """the headline workload in 25,765 bootstraps per block: both reference vectors in lock-step against the golden outputs
    and the plaintext pass, on the step schedule and on the dataflow schedule, the same ciphertext in every register"""
    vecs = [v for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"][:2]
    K = len(vecs)
    assert K == 2
    plain = bce.Circuit()                                    # the plaintext pass
    plain.ReadBristol(os.path.join(CIRCUITS, "AES-expanded.txt"))
    plain.setXorSingle(True)
    want = []
    for v in vecs:
        plain.Reset()
        plain.setPlaintext(True)
        plain.setEncrypted(False)
        plain.SetInput(kat.aes_case(v)[0])
        want.append(plain.Clock()[0])
        assert want[-1] == kat.aes_case(v)[1]
    plain.close()
    snap = {}
    std_cc.set_encrypt_seed(SEED)                            # both circuits draw the same input ciphertexts
    for mode in ("steps", "dataflow"):
        c = bce.Circuit(std_cc)
        c.ReadBristol(os.path.join(CIRCUITS, "AES-expanded.txt"))
        c.setInstances(K)
        c.setXorSingle(True)
        c.setDataflow(mode == "dataflow")
        c.Reset()
        c.setEncrypted(True)
        info = c.info()
        W, stride = info["n_wires"], info["slot_stride"]
        assert info["n_bootstraps"] == 25765 and stride >= W
        for k, v in enumerate(vecs):
            c.SetInput(kat.aes_case(v)[0], instance=k)
        assert c.dataflowActive() == (mode == "dataflow")
        t0 = std_cc.timing()["bootstraps"]
        c.Clock()
        assert std_cc.timing()["bootstraps"] - t0 == 25765 * K == c.stats()["bootstraps"]
        for k, v in enumerate(vecs):
            assert c.Outputs(k)[0] == want[k], "%s: AES vector %d" % (mode, k)
        # the whole register file of both instances (NOT wires are folded into their consumers: no run writes their registers)
        snap[mode] = [hashlib.sha256(std_cc.lwe_read(np.arange(k * stride + lo, k * stride + min(lo + 8192, W), dtype=np.uint32)).tobytes()).hexdigest()
                      for k in range(K) for lo in range(0, W, 8192)]
        c.close()
    std_cc.set_encrypt_seed(None)
    assert len(snap["steps"]) == 2 * 4 and snap["steps"] == snap["dataflow"]


# ---- 5. noise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["STD128_OPT", "toy"])
def test_output_noise_is_a_plain_gates(bce, orc, shape):
    """8,192 BCE_XOR bootstraps on distinct random pairs of 1,024 refreshed inputs, with random folded NOTs: zero wrong
    decryptions, the output's second moment within the band tests/test_gpu_noise.py holds plain gates to (noise_model.BAND
    around the model's plain-gate prediction for this key), mean and largest error under the same bars; and the phase error of
    every input SUM -- the prepared ciphertext (ct1' + ct2') mod q, formed on the host from the pool rows exactly as the
    prologue forms it -- stays below q/8, the margin every level has on both sides."""
    c = bce.BinFHEContext(getattr(bce, "TOY" if shape == "toy" else shape), bce.GINX)
    c.KeyGen(None if shape == "toy" else SEED)
    p = c.params
    q = p["q"]
    s, z = c.export_sk()
    V = nm.model(p, s, z)
    rng = np.random.default_rng(24)
    n_in, M = 1024, 8192
    c.pool_reserve(n_in + M)
    bits = rng.integers(0, 2, n_in).astype(np.uint8)
    c.Encrypt(bits, np.arange(n_in, dtype=np.uint32), mode=1)                 # BOOTSTRAPPED: every input is a refreshed ciphertext
    bits = bits.astype(np.int64)
    _, in0, in1 = nm.random_gates(rng, M, n_in)
    neg = rng.integers(0, 2, (M, 2))
    descs = np.zeros((M, 6), dtype=np.uint32)
    descs[:, 0], descs[:, 1], descs[:, 2], descs[:, 3], descs[:, 4], descs[:, 5] = bce.XOR, in0, in1, n_in + np.arange(M), neg[:, 0], neg[:, 1]
    c.EvalGates((bce.GateDesc * M).from_buffer(descs))
    a, b = bits[in0] ^ neg[:, 0], bits[in1] ^ neg[:, 1]
    want = a ^ b
    out = np.arange(n_in, n_in + M, dtype=np.uint32)
    c.check_reset()
    c.check_slots(out, want.astype(np.uint8))
    rep = c.check_get()[0]
    ratio, mean, bar, mx = nm.report_stats(rep, V["V_out"], V["B_out"])
    # the input sums, with EvalNOT (-a, q/4 - b) folded in as the prologue does
    rows = c.lwe_read(np.arange(n_in, dtype=np.uint32)).astype(np.int64)
    nots = (-rows) % q
    nots[:, -1] = (q // 4 - rows[:, -1]) % q
    sums = (np.where(neg[:, :1] == 1, nots[in0], rows[in0]) + np.where(neg[:, 1:] == 1, nots[in1], rows[in1])) % q
    sum_err = nm.lwe_phase_error(sums, s, q, a + b)
    worst = int(np.abs(sum_err).max())
    print("%s: %d XOR bootstraps, rms %.3f (model %.3f), ratio %.3f, mean %+.3f (bar %.3f), max |e| %d = %.2f sigma; input sums: rms %.2f, max |e| %d of q/8 = %d" % (
        shape, rep["checked"], rep["noise_rms"], math.sqrt(V["V_out"]), ratio, mean, bar, rep["max_abs_err"], mx, float(np.sqrt((sum_err.astype(np.float64) ** 2).mean())), worst, q // 8))
    assert rep["checked"] == M and rep["mismatches"] == 0
    assert list(c.Decrypt(out[:64])) == list(want[:64])
    assert nm.BAND[0] <= ratio <= nm.BAND[1], "measured / model = %.3f outside [%.2f, %.2f]" % (ratio, nm.BAND[0], nm.BAND[1])
    assert abs(mean) <= bar, (mean, bar)
    assert mx <= nm.MAX_SIGMAS, mx
    assert worst < q // 8, (worst, q // 8)
    c.close()


# ---- 6. argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_checks(bce, oracles):
    o, c = _engine(bce, oracles, "split", "GINX")
    c.pool_reserve(8)
    c.Encrypt(np.array([0, 1], dtype=np.uint8), np.arange(2, dtype=np.uint32))
    calls = (lambda d: c.EvalGates(d), lambda d: c.plan_create([d]), lambda d: c.debug_eval_stages(d), lambda d: c.dag_create(d),
             lambda d: c.dag_create(d, pairs=True))
    bad = [bce.PAIR(bce.XOR, g) for g in (bce.OR, bce.AND, bce.NOR, bce.NAND)] + [bce.PAIR(g, bce.XOR) for g in (bce.OR, bce.AND, bce.NOR, bce.NAND)]
    bad += [bce.PAIR(bce.XOR, bce.XOR), 7, 8, 15]
    bad += [6, 0x10000, 0x10000 | bce.AND, 0x10007, 0x20006, bce.XOR | (1 << 31)]     # BCE_XOR is the word 0x10006 and nothing else
    for op in bad:
        for call in calls:
            with pytest.raises(bce.BceError) as e:
                call([(op, 0, 1, 2)])
            assert e.value.code == bce.ERR_ARG, hex(op)
    for op in (bce.XOR, bce.AND):                                     # pool bounds as for AND
        c.EvalGates([(op, 0, 1, 7)])                                  # the last slot
        for d in ((op, 0, 1, 8), (op, 8, 1, 2), (op, 0, 8, 2)):
            for call in calls[:3]:
                with pytest.raises(bce.BceError) as e:
                    call([d])
                assert e.value.code == bce.ERR_POOL, d
        with pytest.raises(bce.BceError) as e:
            c.EvalGates([(op, 0, 1, 2)], instances=2, slot_stride=6)  # 2 + 6 = 8
        assert e.value.code == bce.ERR_POOL
    assert list(c.Decrypt(np.array([7], dtype=np.uint32))) == [0]   # AND(0, 1) was the last write
    c.EvalGates([(bce.XOR, 0, 1, 7)])
    assert list(c.Decrypt(np.array([7], dtype=np.uint32))) == [1]
    c.close()
