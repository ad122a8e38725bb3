"""Checks attached to a resident plan (bce_plan_set_checks / bce_plan_set_expected): after the kernels of step s the
engine decrypts the listed registers on the device, compares them with the expected bits and, with repair on, replaces a
wrong one -- walked step by step (bce_plan_run_step) and inside the captured hipGraph (bce_plan_run) alike.

TOY, K = 2, three dependent steps plus one independent gate per step:
    step 0: r6 = AND(r0, r1)     r9  = OR(r4, r5)
    step 1: r7 = OR(r6, r2)      r10 = AND(r4, r5)
    step 2: r8 = NAND(r7, r3)    r11 = NOR(r4, r5)
A fault = input r0 of instance 1 overwritten with an encryption of the wrong bit; a host simulation of the plan predicts
which checks fail, with and without repair."""
import numpy as np
import pytest

import noise_model as nm

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED
STRIDE, K, BASE = 16, 2, 16        # the plan's instances sit one slot_base above slot 0
BITS = [[0, 1, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1]]       # instance 1: AND = 1, then OR with 0, then NAND with 1: a wrong r0 travels
REGS = np.array([BASE + k * STRIDE + r for k in range(K) for r in range(6, 12)], dtype=np.uint32)


def _steps(bce):
    return [[(bce.AND, 0, 1, 6), (bce.OR, 4, 5, 9)], [(bce.OR, 6, 2, 7), (bce.AND, 4, 5, 10)], [(bce.NAND, 7, 3, 8), (bce.NOR, 4, 5, 11)]]


CHECKS = [[6, 9], [7, 10], [8, 11]]


def _simulate(bce, inputs, truth_inputs, repair):
    """plaintext run of the plan on `inputs` with the expected bits of `truth_inputs`: (expected [K][6], mismatches, final registers)"""
    fn = {bce.AND: lambda a, b: a & b, bce.OR: lambda a, b: a | b, bce.NAND: lambda a, b: 1 - (a & b), bce.NOR: lambda a, b: 1 - (a | b)}
    expect, bad, final = [], set(), []
    for k in range(K):
        good = dict(enumerate(truth_inputs[k]))
        for st in _steps(bce):
            for op, a, b, out in st:
                good[out] = fn[op](good[a], good[b])
        expect.append([good[w] for st in CHECKS for w in st])
        val = dict(enumerate(inputs[k]))
        for s, st in enumerate(_steps(bce)):
            for op, a, b, out in st:
                val[out] = fn[op](val[a], val[b])
            for i, w in enumerate(CHECKS[s]):
                if val[w] != good[w]:
                    bad.add((s, i, k))
                    if repair:
                        val[w] = good[w]
        final.append([val[r] for r in range(6, 12)])
    return np.array(expect, dtype=np.uint8), bad, final


@pytest.fixture(scope="module")
def toy(bce, orc):
    o = orc.Oracle(orc.TOY, orc.GINX)
    o.keygen(SEED)
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(SEED)
    c.pool_reserve(BASE + K * STRIDE)
    yield o, c
    o.close()
    c.close()


def _load(c, inputs):
    c.set_encrypt_seed(SEED)
    for k in range(K):
        c.Encrypt(inputs[k], np.arange(6) + BASE + k * STRIDE, enc_index_base=500 + 8 * k)
    c.set_encrypt_seed(None)
    c.lwe_write(REGS, np.zeros((len(REGS), c.n + 1), dtype=np.uint64))


def _walk(c, plan):
    for s in range(3):
        c.plan_run_step(plan, s)


def test_checks_do_not_perturb_a_correct_run_and_join_a_captured_graph(bce, toy):
    _, c = toy
    _load(c, BITS)
    plan = c.plan_create(_steps(bce), K, STRIDE, BASE)
    _walk(c, plan)
    plain_regs = c.lwe_read(REGS)
    c.plan_run(plan)                                   # captured WITHOUT checks
    assert np.array_equal(c.lwe_read(REGS), plain_regs)
    expect, bad, final = _simulate(bce, BITS, BITS, True)
    assert not bad
    assert list(c.Decrypt(REGS)) == [b for k in range(K) for b in final[k]]
    c.plan_set_checks(plan, CHECKS, repair=True)
    for run in (lambda: _walk(c, plan), lambda: c.plan_run(plan)):     # the second: captured again, now with the checks
        c.lwe_write(REGS, np.zeros((len(REGS), c.n + 1), dtype=np.uint64))
        c.plan_set_expected(plan, expect)
        c.check_reset()
        run()
        rep, log = c.check_get()
        assert (rep["checked"], rep["mismatches"], rep["repaired"], log) == (6 * K, 0, 0, [])
        # every checked register is a bootstrap output of TOY: no error beyond 6.5 sigma of the model (12 samples carry no band)
        nm.check_report(rep, nm.model(c.params, *c.export_sk())["V_out"])
        assert rep["margin"] > 0
        assert np.array_equal(c.lwe_read(REGS), plain_regs), "checks changed a register of a correct run"
    c.plan_set_checks(plan, [[], [], []])                # detached again: runs without expected bits, checks nothing
    c.check_reset()
    c.plan_run(plan)
    assert c.check_get()[0]["checked"] == 0
    c.plan_destroy(plan)


@pytest.mark.parametrize("repair", [True, False])
def test_an_injected_fault_is_found_where_the_simulation_says(bce, toy, repair):
    _, c = toy
    faulty = [list(b) for b in BITS]
    faulty[1][0] ^= 1
    _load(c, faulty)
    expect, bad, final = _simulate(bce, faulty, BITS, repair)
    assert bad == ({(0, 0, 1)} if repair else {(0, 0, 1), (1, 0, 1), (2, 0, 1)})
    truth = _simulate(bce, BITS, BITS, True)[2]
    assert (final == truth) == repair
    plan = c.plan_create(_steps(bce), K, STRIDE, BASE)
    c.plan_set_checks(plan, CHECKS, repair=repair)
    seen = []
    for run in (lambda: _walk(c, plan), lambda: c.plan_run(plan)):
        c.lwe_write(REGS, np.zeros((len(REGS), c.n + 1), dtype=np.uint64))
        c.plan_set_expected(plan, expect)
        c.check_reset()
        run()
        rep, log = c.check_get()
        assert {(x["tag"], x["index"], x["instance"]) for x in log} == bad
        for x in log:
            assert x["slot"] == BASE + x["instance"] * STRIDE + CHECKS[x["tag"]][x["index"]] and x["got"] == 1 - x["expect"]
        assert (rep["checked"], rep["mismatches"], rep["repaired"]) == (6 * K, len(bad), len(bad) if repair else 0)
        assert list(c.Decrypt(REGS)) == [b for k in range(K) for b in final[k]]
        seen.append((rep, sorted(log, key=lambda x: (x["tag"], x["index"], x["instance"])), c.lwe_read(REGS)))
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1], "walked and captured runs report differently"
    assert np.array_equal(seen[0][2], seen[1][2]), "walked and captured runs leave different registers"
    if repair:   # the repaired register is the trivial ciphertext of the right bit
        row = np.zeros(c.n + 1, dtype=np.uint64)
        row[c.n] = int(expect[1][0]) * (c.params["q"] // 4)
        assert np.array_equal(c.lwe_read([BASE + STRIDE + 6])[0], row)
    c.plan_destroy(plan)


def test_a_plan_with_checks_needs_its_expected_bits(bce, toy):
    _, c = toy
    _load(c, BITS)
    plan = c.plan_create(_steps(bce), K, STRIDE, BASE)
    c.plan_set_checks(plan, CHECKS)
    for call in (lambda: c.plan_run_step(plan, 0), lambda: c.plan_run(plan)):
        with pytest.raises(bce.BceError) as e:
            call()
        assert e.value.code == bce.ERR_STATE
    with pytest.raises(bce.BceError) as e:
        c.plan_set_expected(plan, np.full((K, 6), 4, dtype=np.uint8))
    assert e.value.code == bce.ERR_ARG
    with pytest.raises(bce.BceError) as e:
        c.plan_set_checks(plan, [[6], [BASE + K * STRIDE], []])       # a slot outside the pool (slot_base and stride added)
    assert e.value.code == bce.ERR_POOL
    c.plan_destroy(plan)
