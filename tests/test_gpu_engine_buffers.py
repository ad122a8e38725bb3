"""The engine's grow-on-demand buffers and staged uploads (csrc/devmem.hpp in csrc/engine.cpp) along the paths on which they
are reallocated while work is in flight or a captured graph points at their neighbours: the descriptor ring past its
1,024-entry floor and wrapped while busy, the check stage past 64 KiB, the pool under a captured plan with checks, the
expected bits of a DAG for 1 -> 4 -> 1 instances, and the debug calls after an error return.  Everything is exact: bits
against truth tables, report counters against the oracle's decrypt / noise, registers word for word.  TOY (n = 64, N = 512)
wherever the kernel class allows; the DAG needs STD128_OPT (TOY has no persistent kernel).  Nothing here measures device
memory: what is released when is the business of tests/test_devmem_standalone.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED
REPORT_FIELDS = ("checked", "mismatches", "repaired", "sum_err", "sum_sq_err", "max_abs_err")
TRUTH = [lambda a, b: a | b, lambda a, b: a & b, lambda a, b: 1 - (a | b), lambda a, b: 1 - (a & b), lambda a, b: a ^ b,
         lambda a, b: 1 - (a ^ b)]      # OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST = ops 0..5


@pytest.fixture(scope="module")
def toy(bce, orc):
    """same-seed keys on both sides; slots 0, 1 = encryptions of 0, 1 and slots 2, 3 = other encryptions of 0, 1"""
    o = orc.Oracle(orc.TOY, orc.GINX)
    o.keygen(SEED)
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(SEED)
    assert np.array_equal(c.export_sk()[0], o.sk())
    c.pool_reserve(64)
    c.set_encrypt_seed(SEED)
    c.Encrypt([0, 1, 0, 1], [0, 1, 2, 3], enc_index_base=100)
    c.set_encrypt_seed(None)
    yield o, c
    o.close()
    c.close()


def _gates(count, out0):
    """count gates over the four input slots, every (op, a, b) in turn: (descriptors, expected bits)"""
    descs, want = [], []
    for i in range(count):
        op, a, b = i % 6, (i // 6) % 2, (i // 12) % 2
        descs.append((op, a, 2 + b, out0 + i))
        want.append(TRUTH[op](a, b))
    return descs, want


def test_descriptor_ring_grows_shrinks_and_wraps_while_busy(bce, toy):
    _, c = toy
    assert (bce.OR, bce.AND, bce.NOR, bce.NAND, bce.XOR_FAST, bce.XNOR_FAST) == (0, 1, 2, 3, 4, 5)
    c.pool_reserve(4 + 1500)
    for count in (1, 1500, 1):                  # 1,500 is past the ring slots' floor of 1,024 descriptors
        descs, want = _gates(count, 4)
        c.lwe_write(np.arange(4, 4 + count), np.zeros((count, c.n + 1), dtype=np.uint64))
        c.EvalGates(descs)
        assert list(c.Decrypt(np.arange(4, 4 + count))) == want, count
    # scattered reads gather through a ring slot into a staging pair that grows past its floor of 64 rows
    dense = c.lwe_read(np.arange(4, 1504))
    for picks in ([4, 1503], np.arange(4, 1504, 20), [1000, 5]):
        assert np.array_equal(c.lwe_read(picks), dense[np.asarray(picks) - 4]), len(picks)
    # five launches with nothing between them that waits: the fifth takes the first one's ring slot
    c.lwe_write(np.arange(4, 4 + 5 * 24), np.zeros((5 * 24, c.n + 1), dtype=np.uint64))
    wants = []
    for call in range(5):
        descs, want = _gates(24, 4 + 24 * call)
        descs, want = descs[call:] + descs[:call], want[call:] + want[:call]      # a different list in every slot
        descs = [(op, a, b, 4 + 24 * call + i) for i, (op, a, b, _) in enumerate(descs)]
        c.EvalGates(descs)
        wants += want
    assert list(c.Decrypt(np.arange(4, 4 + 5 * 24))) == wants


def _report_of(o, cts, expect):
    got = [o.decrypt(ct) for ct in cts]
    err = [o.noise(ct, int(e)) for ct, e in zip(cts, expect)]
    return {"checked": len(got), "mismatches": sum(int(g != e) for g, e in zip(got, expect)), "repaired": 0,
            "sum_err": sum(err), "sum_sq_err": sum(e * e for e in err), "max_abs_err": max(abs(e) for e in err)}


def test_check_stage_grows_past_64_kib_and_serves_small_lists_again(bce, toy):
    o, c = toy
    q, big, base = c.params["q"], 20000, 8
    c.pool_reserve(base + big)
    # the big list: trivial ciphertexts (0, b), b through all of Z_q, against expected bits that are right for some only;
    # the oracle's verdict on each of the q * 4 (ciphertext, expected bit) pairs, once
    cts = np.zeros((big, c.n + 1), dtype=np.uint64)
    cts[:, c.n] = np.arange(big) % q
    c.lwe_write(np.arange(base, base + big), cts)
    expect_big = ((np.arange(big) // q + np.arange(big) * 4 // q) % 4).astype(np.uint8)
    verdict = {(b, e): (o.decrypt(cts[b]), o.noise(cts[b], e)) for b in range(q) for e in range(4)}
    pairs = [verdict[(i % q, int(expect_big[i]))] for i in range(big)]
    want_big = {"checked": big, "mismatches": sum(int(g != e) for (g, _), e in zip(pairs, expect_big)), "repaired": 0,
                "sum_err": sum(e for _, e in pairs), "sum_sq_err": sum(e * e for _, e in pairs), "max_abs_err": max(abs(e) for _, e in pairs)}
    assert 0 < want_big["mismatches"] < big
    assert 4 * big + big > (1 << 16)            # slot words + expected bytes exceed the stage's floor
    # the small list: the four fresh inputs and four trivial rows, two expectations wrong
    small = np.array([0, 1, 2, 3, base + 5, base + 200, base + 300, base + 511], dtype=np.uint32)
    small_cts = c.lwe_read(small)
    expect_small = np.array([o.decrypt(ct) for ct in small_cts], dtype=np.uint8)
    expect_small[[1, 6]] = (expect_small[[1, 6]] + 1) % 4
    want_small = _report_of(o, small_cts, expect_small)
    assert want_small["mismatches"] == 2
    for slots, expect, want in ((small, expect_small, want_small), (np.arange(base, base + big), expect_big, want_big),
                                (small, expect_small, want_small)):
        c.check_reset()
        c.check_slots(slots, expect, tag=3)
        rep, log = c.check_get()
        assert {f: rep[f] for f in REPORT_FIELDS} == want, len(slots)
        assert all(x["tag"] == 3 and x["got"] != x["expect"] for x in log) and 0 < len(log) <= want["mismatches"]
    assert np.array_equal(c.lwe_read(np.arange(base, base + big)), cts), "repair = 0 changed the pool"


# ---- a captured plan with checks survives a growing pool and new check lists ------------------------------------------------
STRIDE, K, BASE = 16, 2, 16
BITS = [[0, 1, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1]]
PLAN_REGS = np.array([BASE + k * STRIDE + r for k in range(K) for r in range(6, 12)], dtype=np.uint32)


def _plan_steps(bce):
    return [[(bce.AND, 0, 1, 6), (bce.OR, 4, 5, 9)], [(bce.OR, 6, 2, 7), (bce.AND, 4, 5, 10)], [(bce.NAND, 7, 3, 8), (bce.NOR, 4, 5, 11)]]


def _plan_values(bce):
    """plaintext value of every register of every instance"""
    vals = []
    for k in range(K):
        v = dict(enumerate(BITS[k]))
        for st in _plan_steps(bce):
            for op, a, b, out in st:
                v[out] = TRUTH[op](v[a], v[b])
        vals.append(v)
    return vals


def test_pool_growth_and_new_check_lists_under_a_captured_plan(bce, toy):
    _, c = toy
    vals = _plan_values(bce)
    c.set_encrypt_seed(SEED)
    for k in range(K):
        c.Encrypt(BITS[k], np.arange(6) + BASE + k * STRIDE, enc_index_base=500 + 8 * k)
    c.set_encrypt_seed(None)
    plan = c.plan_create(_plan_steps(bce), K, STRIDE, BASE)

    def run(checks, flip):
        """one captured run with the expected bits of `checks`, the one at `flip` = (instance, check) wrong: (report, log, registers)"""
        flat = [r for st in checks for r in st]
        expect = np.array([[vals[k][r] for r in flat] for k in range(K)], dtype=np.uint8)
        expect[flip] ^= 1
        c.plan_set_expected(plan, expect)
        c.lwe_write(PLAN_REGS, np.zeros((len(PLAN_REGS), c.n + 1), dtype=np.uint64))
        c.check_reset()
        c.plan_run(plan)
        rep, log = c.check_get()
        assert (rep["checked"], rep["mismatches"], rep["repaired"]) == (len(flat) * K, 1, 0)
        assert [(x["instance"], x["slot"], x["got"], x["expect"]) for x in log] == \
               [(flip[0], BASE + flip[0] * STRIDE + flat[flip[1]], vals[flip[0]][flat[flip[1]]], 1 - vals[flip[0]][flat[flip[1]]])]
        regs = c.lwe_read(PLAN_REGS)
        assert list(c.Decrypt(PLAN_REGS)) == [vals[k][r] for k in range(K) for r in range(6, 12)]
        return {f: rep[f] for f in REPORT_FIELDS}, log, regs

    checks = [[6, 9], [7, 10], [8, 11]]
    c.plan_set_checks(plan, checks)
    rep0, log0, regs0 = run(checks, (1, 2))
    before = c._L.bce_pool_slots(c.h)
    c.pool_reserve(before + 4096)               # the pool moves: the capture is stale and is taken again, the contents stay
    assert c._L.bce_pool_slots(c.h) == before + 4096
    rep1, log1, regs1 = run(checks, (1, 2))
    assert rep1 == rep0 and log1 == log0 and np.array_equal(regs1, regs0), "the run after the pool grew differs"
    other = [[9], [], [11, 8, 6]]               # another list, another size; slot 6 is checked two steps after it was written
    c.plan_set_checks(plan, other)
    with pytest.raises(bce.BceError) as e:
        c.plan_run(plan)                        # new lists need their own expected bits
    assert e.value.code == bce.ERR_STATE
    rep2, log2, regs2 = run(other, (0, 3))
    assert rep2["checked"] == 4 * K and log2[0]["tag"] == 2 and log2[0]["index"] == 2
    assert np.array_equal(regs2, regs0), "the bootstraps are deterministic: other checks, same registers"
    c.plan_destroy(plan)


# ---- the expected bits of a DAG for 1, 4 and 1 instances, against the plan path -----------------------------------------------
def _dag_tasks(bce):
    A, O, NA, NO = bce.AND, bce.OR, bce.NAND, bce.NOR
    return [(A, 0, 1, 6), (O, 2, 3, 7), (NA, 4, 5, 8), (NO, 0, 2, 9), (O, 6, 7, 10), (A, 8, 9, 11), (NA, 10, 11, 12), (O, 6, 8, 13),
            (A, 12, 13, 14), (NO, 14, 7, 15), (O, 15, 9, 16), (NA, 16, 12, 17)]


def test_dag_expected_bits_for_one_four_and_one_instances_equal_the_plan_path(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    assert c.dag_supported()
    tasks, stride, kmax = _dag_tasks(bce), 32, 4
    level = {}
    for op, a, b, out in tasks:
        level[out] = 1 + max(level.get(a, 0), level.get(b, 0))
    steps = [[i for i, t in enumerate(tasks) if level[t[3]] == lv] for lv in range(1, max(level.values()) + 1)]
    order = [i for st in steps for i in st]     # the DAG's checks in the plan's step-major order: one layout of expected bits
    assert sorted(order) == list(range(12)) and len(steps) == 7
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, (kmax, 6))
    c.pool_reserve(kmax * stride)
    c.set_encrypt_seed(SEED)
    for k in range(kmax):
        c.Encrypt(bits[k], np.arange(6) + k * stride, enc_index_base=700 + 8 * k)
    c.set_encrypt_seed(None)
    vals = []
    for k in range(kmax):
        v = dict(enumerate(int(x) for x in bits[k]))
        for op, a, b, out in tasks:
            v[out] = TRUTH[op](v[a], v[b])
        vals.append(v)
    dag = c.dag_create(tasks)
    c.dag_set_checks(dag, order)
    key = lambda x: (x["instance"], x["slot"], x["err"], x["got"], x["expect"])
    for inst in (1, 4, 1):
        regs = np.array([k * stride + r for k in range(inst) for r in range(6, 18)], dtype=np.uint32)
        expect = np.array([[vals[k][tasks[i][3]] for i in order] for k in range(inst)], dtype=np.uint8)
        expect[inst - 1, 5] ^= 1                # one wrong expectation in the last instance: a log entry to compare
        plan = c.plan_create([[tasks[i] for i in st] for st in steps], inst, stride, 0)
        c.plan_set_checks(plan, [[tasks[i][3] for i in st] for st in steps])
        c.plan_set_expected(plan, expect)
        c.lwe_write(regs, np.zeros((len(regs), c.n + 1), dtype=np.uint64))
        c.check_reset()
        for s in range(len(steps)):
            c.plan_run_step(plan, s)
        rep_p, log_p = c.check_get()
        regs_p = c.lwe_read(regs)
        c.plan_destroy(plan)
        assert (rep_p["checked"], rep_p["mismatches"]) == (12 * inst, 1)
        c.dag_set_expected(dag, expect)
        c.lwe_write(regs, np.zeros((len(regs), c.n + 1), dtype=np.uint64))
        c.check_reset()
        c.dag_run(dag, inst, stride, 0)
        rep_d, log_d = c.check_get()
        last = c.dag_last_run()
        assert last["done"] == 12 * inst and last["abort"] == 0
        for f in REPORT_FIELDS:
            assert rep_d[f] == rep_p[f], (f, inst)
        assert sorted(map(key, log_d)) == sorted(map(key, log_p)) and len(log_d) == 1
        assert np.array_equal(c.lwe_read(regs), regs_p), "registers differ from the plan's (%d instances)" % inst
        assert list(c.Decrypt(regs)) == [vals[k][r] for k in range(inst) for r in range(6, 18)]
    c.dag_destroy(dag)
    c.close()


def test_debug_calls_work_after_their_error_returns(bce, toy):
    _, c = toy
    Q, n_slots = c.params["Q"], c._L.bce_pool_slots(c.h)
    descs, _ = _gates(6, 4)
    acc, lweN, ks = c.debug_eval_stages(descs)
    out = c.lwe_read(np.arange(4, 10))
    with pytest.raises(bce.BceError) as e:
        c.debug_tail(acc, [4, 5, n_slots, 7, 8, 9])
    assert e.value.code == bce.ERR_POOL
    bad = np.zeros((2, c.N), dtype=np.uint64)
    bad[1, 7] = Q
    with pytest.raises(bce.BceError) as e:
        c.debug_ntt(bad)
    assert e.value.code == bce.ERR_ARG
    c.lwe_write(np.arange(4, 10), np.zeros((6, c.n + 1), dtype=np.uint64))
    lweN2, ks2 = c.debug_tail(acc, np.arange(4, 10))
    assert np.array_equal(lweN2, lweN) and np.array_equal(ks2, ks)
    assert np.array_equal(c.lwe_read(np.arange(4, 10)), out), "the tail alone gives other ciphertexts than the gates did"
    ok = np.zeros((2, c.N), dtype=np.uint64)
    ok[1, 7] = Q - 1
    assert np.array_equal(c.debug_ntt(c.debug_ntt(ok), inverse=True), ok)
