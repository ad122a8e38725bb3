"""Verify mode on the dataflow schedule: the persistent kernel decrypts, compares and repairs a task's output between its
bootstrap and the release of its consumers (bce_dag_set_checks / bce_dag_set_expected; Circuit: setDataflow +
setDeviceVerify + setVerify) -- where the reference's Gate::Evaluate does it (src/gate.cpp:153-160).

Parity bar: the checks of a resident step plan (bce_plan_set_checks) on the same slots and the same ciphertexts.  The
counters are integer sums over identical ciphertexts, so every report field must be EQUAL, not close.

Engine level: the six-task DAG of test_gpu_plan_checks.py,
    t0: r6 = AND(r0, r1)    t1: r9  = OR(r4, r5)
    t2: r7 = OR(r6, r2)     t3: r10 = AND(r4, r5)
    t4: r8 = NAND(r7, r3)   t5: r11 = NOR(r4, r5)
with the registers laid out so that every checked output is the direct neighbour of one of its own inputs (pool rows are
n + 1 words apart: neighbours share cache lines) and r6 -> r7 -> r8 sit in a row."""
import os
import random

import numpy as np
import pytest

import kat
import noise_model as nm
from kat import CIRCUITS
from test_random_circuits import random_netlist

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED
STRIDE, K, BASE = 16, 2, 16
#      register: r0 r1 r2 r3 r4 r5  r6 r7 r8 r9 r10 r11
SLOT = dict(zip(range(12), [0, 5, 6, 4, 8, 11, 1, 2, 3, 7, 10, 9]))
BITS = [[0, 1, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1]]      # instance 1: AND = 1, OR with 0, NAND with 1: a wrong r0 travels
OUT_REGS = [6, 9, 7, 10, 8, 11]                      # in task order = in the plan's step-major check order
TASK_TO_STEP = {0: (0, 0), 1: (0, 1), 2: (1, 0), 3: (1, 1), 4: (2, 0), 5: (2, 1)}
REPORT_FIELDS = ("checked", "mismatches", "repaired", "sum_err", "sum_sq_err", "max_abs_err")


def _gates(bce):
    return [(bce.AND, 0, 1, 6), (bce.OR, 4, 5, 9), (bce.OR, 6, 2, 7), (bce.AND, 4, 5, 10), (bce.NAND, 7, 3, 8), (bce.NOR, 4, 5, 11)]


def _tasks(bce):
    return [(op, SLOT[a], SLOT[b], SLOT[o]) for op, a, b, o in _gates(bce)]


def _steps(bce):
    t = _tasks(bce)
    return [[t[0], t[1]], [t[2], t[3]], [t[4], t[5]]]


CHECK_SLOTS = [[SLOT[6], SLOT[9]], [SLOT[7], SLOT[10]], [SLOT[8], SLOT[11]]]
OUT_SLOTS = np.array([BASE + k * STRIDE + SLOT[r] for k in range(K) for r in OUT_REGS], dtype=np.uint32)


def test_layout_puts_every_checked_output_next_to_one_of_its_inputs(bce):
    for op, a, b, o in _gates(bce):
        assert min(abs(SLOT[o] - SLOT[a]), abs(SLOT[o] - SLOT[b])) == 1, (a, b, o)
    assert SLOT[7] - SLOT[6] == 1 and SLOT[8] - SLOT[7] == 1
    assert sorted(SLOT.values()) == list(range(12))


def _simulate(bce, inputs, truth_inputs, repair):
    """plaintext run on `inputs` against the expected bits of `truth_inputs`, a check (and repair) at every task's completion:
    (expected [K][6] in task order, {(task, instance)} that mismatch, final bits of OUT_REGS per instance)"""
    fn = {bce.AND: lambda a, b: a & b, bce.OR: lambda a, b: a | b, bce.NAND: lambda a, b: 1 - (a & b), bce.NOR: lambda a, b: 1 - (a | b)}
    expect, bad, final = [], set(), []
    for k in range(K):
        good, val = dict(enumerate(truth_inputs[k])), dict(enumerate(inputs[k]))
        for t, (op, a, b, out) in enumerate(_gates(bce)):
            good[out] = fn[op](good[a], good[b])
            val[out] = fn[op](val[a], val[b])
            if val[out] != good[out]:
                bad.add((t, k))
                if repair:
                    val[out] = good[out]
        expect.append([good[r] for r in OUT_REGS])
        final.append([val[r] for r in OUT_REGS])
    return np.array(expect, dtype=np.uint8), bad, final


@pytest.fixture(scope="module")
def std(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    assert c.dag_supported()
    yield c
    c.close()


def _load_inputs(c, inputs):
    c.pool_reserve(BASE + K * STRIDE)
    c.set_encrypt_seed(SEED)
    for k in range(K):
        c.Encrypt(inputs[k], np.array([BASE + k * STRIDE + SLOT[r] for r in range(6)], dtype=np.uint32), enc_index_base=500 + 8 * k)
    c.set_encrypt_seed(None)


def _prefill(c, expect):
    """the output registers hold VALID encryptions of the complement of the expected bits: a check that reads one stale
    word of a row finds a wrong bit or a wild error, not zeros that happen to decrypt to 0"""
    c.set_encrypt_seed(SEED + 1)
    c.Encrypt((1 - expect).reshape(-1), OUT_SLOTS, enc_index_base=9000)
    c.set_encrypt_seed(None)


def _key(x):
    return (x["tag"], x["index"], x["instance"], x["slot"], x["err"], x["got"], x["expect"])


@pytest.mark.parametrize("case", ["fault_free", "fault_repair", "fault_no_repair"])
def test_engine_checks_inside_the_kernel_equal_the_plan_s_checks(bce, std, case):
    c = std
    repair = case != "fault_no_repair"
    inputs = [list(b) for b in BITS]
    if case != "fault_free":
        inputs[1][0] ^= 1
    _load_inputs(c, inputs)
    expect, bad, final = _simulate(bce, inputs, BITS, repair)
    assert bad == {"fault_free": set(), "fault_repair": {(0, 1)}, "fault_no_repair": {(0, 1), (2, 1), (4, 1)}}[case]
    # the plan on the same slots, walked step by step
    plan = c.plan_create(_steps(bce), K, STRIDE, BASE)
    c.plan_set_checks(plan, CHECK_SLOTS, repair=repair)
    c.plan_set_expected(plan, expect)
    _prefill(c, expect)
    c.check_reset()
    for s in range(3):
        c.plan_run_step(plan, s)
    rep_p, log_p = c.check_get()
    regs_p = c.lwe_read(OUT_SLOTS)
    c.plan_destroy(plan)
    assert {(x["tag"], x["index"], x["instance"]) for x in log_p} == {TASK_TO_STEP[t] + (k,) for t, k in bad}
    # the DAG, twice on the same object (the second run re-arms the queues)
    dag = c.dag_create(_tasks(bce))
    c.dag_set_checks(dag, list(range(6)), repair=repair)
    c.dag_set_expected(dag, expect)
    for run in range(2):
        _prefill(c, expect)
        c.check_reset()
        c.dag_run(dag, K, STRIDE, BASE)
        rep_d, log_d = c.check_get()
        last = c.dag_last_run()
        assert last["done"] == 6 * K and last["abort"] == 0
        for f in REPORT_FIELDS:
            print("%-16s run %d %-12s plan %d dag %d" % (case, run, f, rep_p[f], rep_d[f]))
        for f in REPORT_FIELDS:
            assert rep_d[f] == rep_p[f], (f, run)
        assert rep_d["checked"] == 6 * K and rep_d["mismatches"] == len(bad) and rep_d["repaired"] == (len(bad) if repair else 0)
        assert {(x["tag"], x["instance"]) for x in log_d} == bad, "a mismatch at a consumer: its producer was released before the repair"
        for x in log_d:
            assert x["index"] == x["tag"] and x["slot"] == BASE + x["instance"] * STRIDE + SLOT[OUT_REGS[x["tag"]]]
        mapped = [dict(x, tag=TASK_TO_STEP[x["tag"]][0], index=TASK_TO_STEP[x["tag"]][1]) for x in log_d]
        assert sorted(map(_key, mapped)) == sorted(map(_key, log_p))
        assert np.array_equal(c.lwe_read(OUT_SLOTS), regs_p), "registers differ from the plan's (run %d)" % run
        assert list(c.Decrypt(OUT_SLOTS)) == [b for k in range(K) for b in final[k]]
        if case == "fault_free":   # 12 bootstrap outputs of STD128_OPT: no error beyond 6.5 sigma of the model (too few for a band)
            nm.check_report(rep_d, nm.model(c.params, *c.export_sk())["V_out"])
            assert rep_d["margin"] > 0
        if case == "fault_repair":     # the repaired register is the trivial ciphertext of the right bit
            row = np.zeros(c.n + 1, dtype=np.uint64)
            row[c.n] = int(expect[1][0]) * (c.params["q"] // 4)
            assert np.array_equal(c.lwe_read([BASE + STRIDE + SLOT[6]])[0], row)
    c.dag_destroy(dag)


def test_engine_state_and_argument_errors_and_detaching(bce, std):
    c = std
    inputs = [list(b) for b in BITS]
    inputs[1][0] ^= 1
    _load_inputs(c, inputs)
    expect = _simulate(bce, inputs, BITS, True)[0]
    # a run that never had checks: the registers to compare the detached run with
    ref = c.dag_create(_tasks(bce))
    _prefill(c, expect)
    c.dag_run(ref, K, STRIDE, BASE)
    c.synchronize()
    regs_ref = c.lwe_read(OUT_SLOTS)
    c.dag_destroy(ref)

    dag = c.dag_create(_tasks(bce))

    def fails(code, call):
        with pytest.raises(bce.BceError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))

    fails(bce.ERR_ARG, lambda: c.dag_set_checks(dag, [0, 6]))                 # task index out of range
    fails(bce.ERR_ARG, lambda: c.dag_set_checks(dag, [0, 2, 0]))              # duplicate
    fails(bce.ERR_STATE, lambda: c.dag_set_expected(dag, expect))             # no checks attached (the failed calls attached none)
    c.dag_set_checks(dag, list(range(6)), repair=True)
    fails(bce.ERR_STATE, lambda: c.dag_run(dag, K, STRIDE, BASE))             # checks, no expected bits
    fails(bce.ERR_ARG, lambda: c.dag_set_expected(dag, np.full((K, 6), 4, dtype=np.uint8)))
    fails(bce.ERR_ARG, lambda: c._ck(c._L.bce_dag_set_expected(c.h, dag, K, None)))
    fails(bce.ERR_ARG, lambda: c._ck(c._L.bce_dag_set_checks(c.h, dag, 2, None, 0)))
    fails(bce.ERR_STATE, lambda: c.dag_run(dag, K, STRIDE, BASE))             # the rejected bits were not taken
    c.dag_set_expected(dag, expect[:1])
    fails(bce.ERR_STATE, lambda: c.dag_run(dag, K, STRIDE, BASE))             # expected bits of 1 instance, run of 2
    c.dag_set_expected(dag, expect)
    _prefill(c, expect)
    c.check_reset()
    c.dag_run(dag, K, STRIDE, BASE)
    rep, _ = c.check_get()
    assert (rep["checked"], rep["mismatches"], rep["repaired"]) == (6 * K, 1, 1)
    c.dag_set_checks(dag, [])                                                 # detached
    _prefill(c, expect)
    c.check_reset()
    c.dag_run(dag, K, STRIDE, BASE)
    rep, log = c.check_get()
    assert rep["checked"] == 0 and log == []
    assert np.array_equal(c.lwe_read(OUT_SLOTS), regs_ref), "a detached run differs from a run that never had checks"
    c.dag_destroy(dag)


def _adder2_fault(bce, cc, dataflow, capfd):
    """adder_2bit.out, a = 1, b = 3, input register R0 re-encrypted with the wrong bit; two Clock()s; returns the reports"""
    c = bce.Circuit(cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setDataflow(dataflow)
    c.setDeviceVerify(True)
    c.Reset()
    assert not c.deviceVerifyActive() and c.dataflowActive() == dataflow           # verify is not on yet
    c.setVerify(True)
    assert c.deviceVerifyActive() and c.dataflowActive() == dataflow
    cc.set_encrypt_seed(SEED)
    c.SetInput([[1, 0], [1, 1]])
    cc.Encrypt([0], [0], enc_index_base=123456)              # R0 (a bit 0) now encrypts 0 instead of 1
    cc.set_encrypt_seed(None)
    reports = []
    for rep_no in range(2):
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
        assert rep["checked"] == 7 and st["bootstraps"] == 13           # 3 XOR + 3 AND + 1 OR outputs; temporaries unchecked
        if dataflow:
            assert st["sublaunches"] == 1 and st["levels"] == 1
        else:
            assert st["sublaunches"] == st["levels"] == len(c.relevel_steps())
        reports.append({f: rep[f] for f in REPORT_FIELDS})
    c.close()
    return reports


def test_driver_injected_fault_is_repaired_inside_the_persistent_kernel(bce, std, capfd):
    flow = _adder2_fault(bce, std, True, capfd)
    steps = _adder2_fault(bce, std, False, capfd)
    print("dataflow", flow, "steps", steps)
    assert flow[0] == flow[1] == steps[0] == steps[1]


def _run_circuit(bce, cc, path, new_flag, K, ins, mode, fault=None, capfd=None):
    """mode: 'flow' (verify off, dataflow), 'steps_verify', 'flow_verify'; fault = (instance, wire): that input register is
    re-encrypted with the complement of its bit.  Returns registers of all wires, outputs, report, stats, stderr."""
    c = bce.Circuit(cc)
    c.ReadBristol(path, new_flag=new_flag)
    c.setInstances(K)
    c.setDataflow(mode != "steps_verify")
    c.setDeviceVerify(mode != "flow")
    c.Reset()
    if mode == "flow":
        c.setEncrypted(True)
    else:
        c.setVerify(True)
    assert c.dataflowActive() == (mode != "steps_verify") and c.deviceVerifyActive() == (mode != "flow")
    info = c.info()
    W, stride = info["n_wires"], info["slot_stride"]
    cc.pool_reserve(K * stride)
    cc.lwe_write(np.arange(K * stride, dtype=np.uint32), np.zeros((K * stride, cc.n + 1), dtype=np.uint64))
    cc.set_encrypt_seed(SEED)
    for k in range(K):
        c.SetInput(ins[k], instance=k)
    if fault is not None:
        slot = fault[0] * stride + fault[1]
        bit = int(cc.Decrypt([slot])[0])
        cc.Encrypt([1 - bit], [slot], enc_index_base=424242)
    cc.set_encrypt_seed(None)
    if capfd is not None:
        capfd.readouterr()
    c.Clock()
    err = capfd.readouterr().err if capfd is not None else ""
    outs = [c.Outputs(k) for k in range(K)]
    regs = np.concatenate([cc.lwe_read(np.arange(k * stride, k * stride + W, dtype=np.uint32)) for k in range(K)])
    st, rep, counts = c.stats(), c.check_report(), c.counts()
    c.close()
    return regs, outs, rep, st, err, counts


def test_driver_fault_free_adder_64bit_is_the_verify_off_run_and_the_step_schedule_s_report(bce, std):
    cc = std
    path = os.path.join(CIRCUITS, "adder_64bit.txt")
    Kc = 2
    cases = [kat.adder_case(t, 64) for t in range(Kc)]
    ins = [x[0] for x in cases]
    res = {m: _run_circuit(bce, cc, path, False, Kc, ins, m) for m in ("flow", "steps_verify", "flow_verify")}
    for m, (regs, outs, rep, st, _, counts) in res.items():
        for k in range(Kc):
            assert outs[k][0] == cases[k][1], (m, k)
        if m != "flow":
            assert rep["mismatches"] == 0 and rep["repaired"] == 0 and st["verify_fixes"] == 0
            assert rep["checked"] == Kc * (counts["and"] + counts["or"] + counts["xor"]) >= 200
            # every checked register is a bootstrap output of STD128_OPT: second moment in the model's band for this sample size
            ratio = nm.check_report(rep, nm.model(cc.params, *cc.export_sk())["V_out"])
            print("%-12s %d checked, noise_rms %.3f, measured / model %.3f" % (m, rep["checked"], rep["noise_rms"], ratio))
            assert rep["margin"] > 0
    assert res["flow_verify"][3]["levels"] == 1          # one persistent launch (plus the launch of the output NOTs, as with verify off)
    assert res["flow_verify"][3]["sublaunches"] == res["flow"][3]["sublaunches"] <= 2
    assert np.array_equal(res["flow_verify"][0], res["flow"][0]), "the checks changed a ciphertext of a fault-free run"
    assert np.array_equal(res["flow_verify"][0], res["steps_verify"][0])
    for f in REPORT_FIELDS:
        print("%-12s steps %d dataflow %d" % (f, res["steps_verify"][2][f], res["flow_verify"][2][f]))
    for f in REPORT_FIELDS:
        assert res["flow_verify"][2][f] == res["steps_verify"][2][f], f


@pytest.mark.parametrize("seed", range(2))
def test_driver_random_netlists_with_a_fault_equal_the_step_schedule(bce, std, tmp_path, capfd, seed):
    cc = std
    rnd = random.Random(9100 + seed)
    text, in_w, out_w, evaluate = random_netlist(rnd, rnd.randint(20, 70))
    path = tmp_path / "rand.txt"
    path.write_text(text)
    Kc = 3
    ins = [[[rnd.randint(0, 1) for _ in range(w)] for w in in_w] for _ in range(Kc)]
    fault = (rnd.randrange(Kc), rnd.randrange(sum(in_w)))
    a = _run_circuit(bce, cc, str(path), True, Kc, ins, "steps_verify", fault, capfd)
    b = _run_circuit(bce, cc, str(path), True, Kc, ins, "flow_verify", fault, capfd)
    assert np.array_equal(a[0], b[0]), "wire registers differ"
    assert a[1] == b[1]
    for k in range(Kc):
        if k != fault[0]:
            assert b[1][k] == evaluate(ins[k]), k
    for f in REPORT_FIELDS:
        print("%-12s steps %d dataflow %d" % (f, a[2][f], b[2][f]))
    for f in REPORT_FIELDS:
        assert a[2][f] == b[2][f], f
    assert a[3]["verify_fixes"] == b[3]["verify_fixes"]
    assert a[4].count("Bad ") == b[4].count("Bad ")
    assert b[3]["levels"] == 1


def test_config5_class_runs_the_checks_in_the_fp64_kernel(bce, capfd):
    """STD192 / AP: k_bootstrap_dag64 through the same worker"""
    cc = bce.BinFHEContext(bce.STD192, bce.AP)
    try:
        cc.KeyGen(2718)
        assert cc.dag_supported()
        flow = _adder2_fault(bce, cc, True, capfd)
        steps = _adder2_fault(bce, cc, False, capfd)
        assert flow[0] == flow[1] == steps[0] == steps[1]
    finally:
        cc.close()


def test_without_the_device_opt_in_dataflow_and_verify_keep_the_host_path(bce, std):
    c = bce.Circuit(std)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setDataflow(True)
    c.Reset()
    c.setVerify(True)
    assert not c.dataflowActive() and not c.deviceVerifyActive()
    c.SetInput([[1, 0], [1, 1]])
    out = c.Clock()[0]
    assert out[0] + 2 * out[1] + 4 * out[2] == 4
    assert c.stats()["levels"] == c.info()["n_levels"]                     # the gate-level rounds of the host path ...
    assert c.stats()["sublaunches"] == c.info()["n_sublaunches"] > 1       # ... with their two stages per level
    assert c.check_report()["checked"] == 0
    c.close()
