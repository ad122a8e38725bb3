"""Pair tasks in the persistent kernel (bce_dag_create_pairs): a BCE_PAIR descriptor is ONE task of the dependency-driven
evaluation with the two outputs `out` and `out + 1`, both published by the task's one release.

Parity bar: every register a DAG run writes holds, word for word, what the same descriptors leave through bce_eval_gates
called level by level on the same context and the same seeded input ciphertexts -- the path tests/test_gpu_pairs.py pins to
the oracle stage by stage -- and decrypts to the truth tables.  All through the C ABI."""
import numpy as np
import pytest

import pair_model as pm

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED
N_IN = 4
#                instance 0     instance 1     instance 2
INPUT_BITS = [[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 1, 0]]
COMBOS = [(0, 2), (0, 3), (1, 2), (1, 3)]          # instance 0: (0, 0), (0, 1), (1, 0), (1, 1)
K = len(INPUT_BITS)


@pytest.fixture(scope="module", params=["GINX", "AP"])
def std(request, bce):
    c = bce.BinFHEContext(bce.STD128_OPT, getattr(bce, request.param))
    c.KeyGen(SEED)
    assert c.dag_supported()
    yield c
    c.close()


def _writes(t):
    return [t[3], t[3] + 1] if t[0] >> 8 else [t[3]]


def _levels(tasks):
    lvl, out = {}, []
    for t in tasks:
        l = 1 + max(lvl.get(t[1], 0), lvl.get(t[2], 0))
        for o in _writes(t):
            lvl[o] = l
        while len(out) < l:
            out.append([])
        out[l - 1].append(t)
    return out


def _plain(tasks, bits):
    val = dict(enumerate(bits))
    for t in tasks:
        op, a, b, out, n0, n1 = (tuple(t) + (0, 0))[:6]
        x, y = val[a] ^ n0, val[b] ^ n1
        val[out] = pm.truth(op & 0xFF, x, y)
        if op >> 8:
            val[out + 1] = pm.truth((op >> 8) - 1, x, y)
    return val


def _every_pair_dag(bce):
    """all 12 ordered pairs; pair i on input combination i % 4, every third with a NOT folded into an input; behind each pair a
    consumer of both outputs, one of `out` alone and one of `out + 1` alone"""
    tasks = []
    for i, (op, op2) in enumerate(pm.ORDERED_PAIRS):
        a, b = COMBOS[i % 4]
        t = N_IN + 5 * i
        tasks.append((bce.PAIR(op, op2), a, b, t, 1 if i % 3 == 1 else 0, 1 if i % 6 == 4 else 0))
        tasks.append((bce.AND, t, t + 1, t + 2, 0, 0))
        tasks.append((bce.NAND, t, a, t + 3, 0, 1 if i % 2 else 0))
        tasks.append((bce.OR, b, t + 1, t + 4, 1 if i % 4 == 2 else 0, 0))
    return tasks, N_IN + 5 * len(pm.ORDERED_PAIRS)


def _chain_dag(bce, depth=8):
    """every link reads ONLY the second output of the pair before it (and an input): a DAG that ignored the second output's
    writer would start every link at once, on registers that hold nothing yet"""
    ops = [(pm.OR, pm.NAND), (pm.AND, pm.NOR), (pm.NOR, pm.OR), (pm.NAND, pm.AND)]
    tasks, prev = [], 1
    for j in range(depth):
        op, op2 = ops[j % 4]
        out = N_IN + 2 * j
        tasks.append((bce.PAIR(op, op2), prev, j % N_IN, out, j & 1, 0))
        prev = out + 1
    return tasks, N_IN + 2 * depth


def _load_inputs(c, stride, base, bits=INPUT_BITS, seed=SEED):
    """the same input ciphertexts in the two copies of the K instances: slots k * stride + i and base + k * stride + i"""
    c.pool_reserve(base + len(bits) * stride)
    flat = np.array([b for row in bits for b in row], dtype=np.uint8)
    slots = np.array([k * stride + i for k in range(len(bits)) for i in range(N_IN)], dtype=np.uint32)
    c.set_encrypt_seed(seed)
    c.Encrypt(flat, slots, enc_index_base=700)
    c.Encrypt(flat, slots + base, enc_index_base=700)
    c.set_encrypt_seed(None)
    assert np.array_equal(c.lwe_read(slots), c.lwe_read(slots + base))


def _reference(c, name, tasks, stride, bits=INPUT_BITS):
    """bce_eval_gates level by level on instances at slot 0; returns (written slots of all instances, their ciphertexts)"""
    Kb = len(bits)
    written = np.array([k * stride + o for k in range(Kb) for t in tasks for o in _writes(t)], dtype=np.uint32)
    cache = c.__dict__.setdefault("_level_by_level", {})     # computed once per context and DAG, shared by the tests, read-only
    if name not in cache:
        for level in _levels(tasks):
            c.EvalGates(level, instances=Kb, slot_stride=stride)
        want = c.lwe_read(written)
        got_bits = list(c.Decrypt(written))
        plain = [_plain(tasks, b) for b in bits]
        assert got_bits == [plain[k][o] for k in range(Kb) for t in tasks for o in _writes(t)], "the reference path's own bits"
        want.setflags(write=False)
        cache[name] = want
    return written, cache[name]


def _run_and_compare(c, name, tasks, n_slots, wgs=(1, 2), bits=INPUT_BITS):
    Kb = len(bits)
    stride = n_slots + 3                       # a stride with room to spare
    base = Kb * stride
    _load_inputs(c, stride, base, bits)
    written, want = _reference(c, name, tasks, stride, bits)
    plain = [_plain(tasks, b) for b in bits]
    want_bits = [plain[k][o] for k in range(Kb) for t in tasks for o in _writes(t)]
    zeros = np.zeros((written.size, c.n + 1), dtype=np.uint64)
    for wg in wgs:
        c.dag_set_limits(workgroups_per_cu=wg)
        dag = c.dag_create(tasks, prio=[i % 4 for i in range(len(tasks))], pairs=True)
        c.lwe_write(written + base, zeros)
        t0 = c.timing()["bootstraps"]
        c.dag_run(dag, Kb, stride, base)
        c.synchronize()
        last = c.dag_last_run()
        assert last["done"] == len(tasks) * Kb and last["abort"] == 0, last
        assert c.timing()["bootstraps"] - t0 == len(tasks) * Kb, "a pair counts as one bootstrap"
        got = c.lwe_read(written + base)
        for r in np.nonzero((got != want).any(axis=1))[0]:
            raise AssertionError("%s, %d workgroup(s) per CU: slot %d differs from the level-by-level path" % (name, wg, written[r]))
        assert list(c.Decrypt(written + base)) == want_bits
        c.dag_destroy(dag)
    c.dag_set_limits()


# ---- 1. every pair, both residencies ---------------------------------------------------------------------------------------------------
def test_every_ordered_pair_with_all_three_kinds_of_consumer(bce, std):
    tasks, n_slots = _every_pair_dag(bce)
    assert len(tasks) == 48 and sum(1 for t in tasks if t[0] >> 8) == 12
    assert any(t[4] for t in tasks if t[0] >> 8) and any(t[5] for t in tasks if t[0] >> 8)
    seen = {tuple(b[x] ^ n for x, n in ((t[1], t[4]), (t[2], t[5]))) for b in INPUT_BITS for t in tasks if t[0] >> 8}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    _run_and_compare(std, "pairs", tasks, n_slots)


# ---- 2. a chain that hangs on second outputs only ----------------------------------------------------------------------------------------
def test_a_chain_through_second_outputs_only(bce, std):
    tasks, n_slots = _chain_dag(bce)
    assert len(_levels(tasks)) == 8 and all(t[1] == u[3] + 1 for u, t in zip(tasks, tasks[1:]))
    _run_and_compare(std, "chain", tasks, n_slots)


# ---- 3. the config-5 class: k_bootstrap_dag64 -----------------------------------------------------------------------------------------
def test_config5_pair_dag(bce):
    c = bce.BinFHEContext(bce.STD192, bce.AP)
    c.KeyGen(2718)
    assert c.dag_supported() and c.params["N"] == 2048
    t = N_IN
    tasks = [(bce.PAIR(bce.OR, bce.NAND), 0, 1, t, 0, 0), (bce.AND, t, t + 1, t + 2, 0, 0),
             (bce.PAIR(bce.NOR, bce.AND), 2, 3, t + 3, 1, 0), (bce.OR, t + 4, 0, t + 5, 0, 1),
             (bce.PAIR(bce.AND, bce.OR), t + 2, t + 5, t + 6, 0, 0), (bce.NAND, t + 6, 3, t + 8, 0, 0),
             (bce.PAIR(bce.NAND, bce.NOR), t + 7, t + 3, t + 9, 0, 1), (bce.NOR, t + 10, t + 9, t + 11, 0, 0)]
    _run_and_compare(c, "config5", tasks, t + 12, wgs=(0,), bits=INPUT_BITS[:2])
    c.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------
def test_what_bce_dag_create_pairs_refuses(bce, std):
    c = std
    c.pool_reserve(16)
    ok = bce.PAIR(bce.OR, bce.NAND)

    def refused(tasks, code=bce.ERR_ARG):
        with pytest.raises(bce.BceError) as e:
            c.dag_create(tasks, pairs=True)
        assert e.value.code == code, (tasks, str(e.value))

    refused([(ok, 0, 1, 4), (bce.AND, 0, 1, 5)])                   # writes another pair's out + 1
    refused([(bce.AND, 0, 1, 5), (ok, 0, 1, 4)])                   # out + 1 already written
    refused([(bce.AND, 5, 1, 6), (ok, 0, 1, 4)])                   # reads the pair's out + 1 before the pair
    refused([(bce.AND, 0, 1, 8), (bce.OR, 8, 5, 9), (ok, 2, 3, 4)])   # ... so the pair's out + 1 is read by an earlier task
    refused([(ok, 5, 1, 4)])                                       # reads its own second output
    for op in (bce.PAIR(bce.OR, bce.OR), bce.PAIR(bce.XOR_FAST, bce.AND), bce.PAIR(bce.AND, bce.XNOR_FAST), bce.PAIR(bce.OP_REFRESH, bce.AND),
               bce.PAIR(bce.OR, bce.NAND) | (1 << 16), bce.AND | (200 << 8)):
        refused([(op, 0, 1, 4)])
        with pytest.raises(bce.BceError) as e:                     # the status bce_eval_gates gives for the same word
            c.EvalGates([(op, 0, 1, 4)])
        assert e.value.code == bce.ERR_ARG
    with pytest.raises(bce.BceError) as e:                         # without the new entry pairs stay refused
        c.dag_create([(ok, 0, 1, 4)])
    assert e.value.code == bce.ERR_UNSUPPORTED
    dag = c.dag_create([(ok, 0, 1, 4), (bce.AND, 4, 5, 6)], pairs=True)
    with pytest.raises(bce.BceError) as e:                         # the stride must cover out + 1 of the last task too
        c.dag_run(dag, 2, 6, 0)
    assert e.value.code == bce.ERR_ARG
    c.dag_destroy(dag)
    dag = c.dag_create([(ok, 0, 1, 4)], pairs=True)                # max slot = out + 1 = 5
    with pytest.raises(bce.BceError) as e:
        c.dag_run(dag, 2, 5, 0)                                    # stride 5 covers out, not out + 1
    assert e.value.code == bce.ERR_ARG
    with pytest.raises(bce.BceError) as e:
        c.dag_run(dag, 1, 0, (1 << 31))                            # far outside any pool
    assert e.value.code == bce.ERR_POOL
    c.dag_destroy(dag)


def test_out_plus_one_beyond_the_pool(bce):
    """a context of its own, so that the pool has exactly 8 slots: out = 6 fits, out = 7 leaves out + 1 outside"""
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    c.pool_reserve(8)
    c.Encrypt(np.array([0, 1], dtype=np.uint8), np.arange(2, dtype=np.uint32))
    ok = bce.PAIR(bce.OR, bce.NAND)
    dag = c.dag_create([(ok, 0, 1, 6)], pairs=True)
    c.dag_run(dag, 1, 0, 0)
    c.synchronize()
    assert list(c.Decrypt(np.array([6, 7], dtype=np.uint32))) == [1, 1]
    c.dag_destroy(dag)
    dag = c.dag_create([(ok, 0, 1, 7)], pairs=True)
    with pytest.raises(bce.BceError) as e:
        c.dag_run(dag, 1, 0, 0)
    assert e.value.code == bce.ERR_POOL
    c.dag_destroy(dag)
    dag = c.dag_create([(ok, 0, 1, 2)], pairs=True)
    with pytest.raises(bce.BceError) as e:
        c.dag_run(dag, 2, 5, 0)                                    # 2 + 1 + 5 = 8
    assert e.value.code == bce.ERR_POOL
    c.dag_destroy(dag)
    c.close()


# ---- 5. checks -----------------------------------------------------------------------------------------------------------------------------
def test_checks_on_and_consumers_and_on_a_pair_task(bce, std):
    c = std
    tasks, n_slots = _every_pair_dag(bce)
    stride = n_slots + 3
    base = K * stride
    _load_inputs(c, stride, base)
    plain = [_plain(tasks, b) for b in INPUT_BITS]
    ands = [i for i, t in enumerate(tasks) if t[0] == bce.AND]
    checked = ands + [0]                                           # the 12 AND consumers and the first pair task
    assert len(ands) == 12 and tasks[0][0] >> 8
    expect = np.array([[plain[k][tasks[i][3]] for i in checked] for k in range(K)], dtype=np.uint8)   # a pair: its FIRST output
    dag = c.dag_create(tasks, pairs=True)
    c.dag_set_checks(dag, checked, repair=False)
    c.dag_set_expected(dag, expect)
    c.check_reset()
    c.dag_run(dag, K, stride, base)
    rep, log = c.check_get()
    assert rep["checked"] == len(checked) * K and rep["mismatches"] == 0 and rep["repaired"] == 0 and not log
    assert c.dag_last_run()["done"] == len(tasks) * K
    # one expected bit flipped, with repair: that register ends as the trivial ciphertext of the expected bit
    flip_check, flip_k = 3, 1
    expect[flip_k, flip_check] ^= 1
    c.dag_set_checks(dag, checked, repair=True)
    c.dag_set_expected(dag, expect)
    c.check_reset()
    c.dag_run(dag, K, stride, base)
    rep, log = c.check_get()
    assert rep["checked"] == len(checked) * K and rep["mismatches"] == 1 and rep["repaired"] == 1
    slot = base + flip_k * stride + tasks[checked[flip_check]][3]
    assert len(log) == 1 and (log[0]["tag"], log[0]["index"], log[0]["instance"], log[0]["slot"]) == (checked[flip_check], flip_check, flip_k, slot)
    row = c.lwe_read(np.array([slot], dtype=np.uint32))[0]
    trivial = np.zeros(c.n + 1, dtype=np.uint64)
    trivial[-1] = int(expect[flip_k, flip_check]) * (c.params["q"] // 4)
    assert np.array_equal(row, trivial)
    c.dag_destroy(dag)
