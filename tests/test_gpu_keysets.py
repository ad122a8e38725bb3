"""Key sets (include/bce_gpu.h, "key sets"): gates under several clients' keys in one launch.

Set k of a context gets KeyGen(SEEDS[k]) under its selection; the reference is always the oracle keyed with the same seed
(test_gpu_engine.test_keygen_matches_oracle_keygen pins that the two agree), never a keyed call.  BCE_XOR and BCE_PAIR are no
gates of the oracle's batched eval_gates: for them the reference is tests/xor_single_model.py / tests/pair_model.py, the
restatements from the oracle's own primitives that the existing XOR and pair tests use.  Where the oracle would take too long
(600 STD128_OPT bootstraps) the reference is a fresh single-set context running the unkeyed call.  Every comparison is word
for word on the final ciphertexts."""
import numpy as np
import pytest

import noise_run
import xor_single_model as xm
from test_gpu_engine import _custom_narrow

pytestmark = pytest.mark.gpu

SEEDS = [0x0FE5EED, 0x0FE5EED + 1, 0x0FE5EED + 2]
MAP4 = [2, 0, 2, 1]          # a repeat, out of order, set 0 in the middle


def _keyed(bce, orc, nsets, paramset=None, method="GINX", custom=None, oracles=None):
    """a context with `nsets` key sets, set k from KeyGen(SEEDS[k]) under its selection, and the oracles of the same seeds"""
    mk = dict(method=getattr(bce, method), custom=custom) if custom else dict(paramset=getattr(bce, paramset), method=getattr(bce, method))
    c = bce.BinFHEContext(**mk)
    if oracles is None:
        oracles = _oracles(orc, nsets, paramset, method, custom)
    assert c.keyset_count() == 1 and c.keyset_selected() == 0
    for k in range(nsets):
        if k:
            assert c.keyset_add() == k
            c.keyset_select(k)
        c.KeyGen(SEEDS[k])
    c.keyset_select(0)
    assert c.keyset_count() == nsets and c.keyset_selected() == 0
    assert c.params == oracles[0].params
    return c, oracles


def _oracles(orc, nsets, paramset=None, method="GINX", custom=None):
    out = []
    for k in range(nsets):
        o = orc.Oracle(method=getattr(orc, method), custom=custom) if custom else orc.Oracle(getattr(orc, paramset), getattr(orc, method))
        o.keygen(SEEDS[k])
        out.append(o)
    return out


@pytest.fixture(scope="module")
def toy3(bce, orc):
    c, os_ = _keyed(bce, orc, 3, "TOY")
    yield c, os_
    c.close()


@pytest.fixture(scope="module")
def std_oracles(orc):
    return _oracles(orc, 2, "STD128_OPT")


@pytest.fixture(scope="module")
def std2(bce, orc, std_oracles):
    c, os_ = _keyed(bce, orc, 2, "STD128_OPT", oracles=std_oracles)
    yield c, os_
    c.close()


def _replay(o, ins, descs):
    """the registers the descriptors leave, from the input registers {slot: ciphertext}, under oracle o (model for XOR / PAIR)"""
    pool = dict(ins)
    for d in descs:
        xm.eval_desc(o, pool, d)
    return pool


def _written(bce, descs):
    regs = []
    for d in descs:
        regs.append(d[3])
        if (d[0] >> 8) & 0xFF:
            regs.append(d[3] + 1)
    return regs


# ---- 1. one frontier with every kind of descriptor, against the oracle -----------------------------------------------------------
def test_frontier_of_every_descriptor_kind_under_three_sets(toy3, bce):
    c, os_ = toy3
    K, stride = 4, 16
    c.pool_reserve(K * stride)
    frontier = [(bce.OR, 0, 1, 4), (bce.AND, 0, 1, 5), (bce.NOR, 0, 1, 6), (bce.NAND, 0, 1, 7), (bce.XOR_FAST, 0, 1, 8), (bce.XNOR_FAST, 0, 1, 9),
                (bce.XOR, 0, 1, 10), (bce.OP_REFRESH, 0, 0, 11), (bce.AND, 0, 1, 12, 1, 0), (bce.OR, 0, 1, 13, 0, 1), (bce.PAIR(bce.OR, bce.NAND), 0, 1, 14)]
    regs = _written(bce, frontier)
    assert regs == list(range(4, 16))
    ins = []
    for k in range(K):
        o = os_[MAP4[k]]
        a, b = k & 1, k >> 1
        ins.append({0: o.encrypt(a, 100 + 2 * k), 1: o.encrypt(b, 101 + 2 * k)})
        c.lwe_write([k * stride, k * stride + 1], np.stack([ins[k][0], ins[k][1]]))
    c.EvalGates(frontier, instances=K, slot_stride=stride, keysets=MAP4)
    got = c.lwe_read([k * stride + s for k in range(K) for s in regs]).reshape(K, len(regs), -1)
    told_apart = False
    for k in range(K):
        want = _replay(os_[MAP4[k]], ins[k], frontier)
        for j, s in enumerate(regs):
            assert np.array_equal(got[k, j], want[s]), "instance %d (set %d) register %d" % (k, MAP4[k], s)
        a, b = k & 1, k >> 1
        assert [os_[MAP4[k]].decrypt(got[k, j]) for j in range(len(regs))] == \
            [a | b, a & b, 1 - (a | b), 1 - (a & b), a ^ b, 1 - (a ^ b), a ^ b, a, (1 - a) & b, a | (1 - b), a | b, 1 - (a & b)]
        if MAP4[k] != 0 and not told_apart:      # the same inputs under set 0's keys give other words: the test can tell keys apart
            other = _replay(os_[0], ins[k], frontier)
            assert all(not np.array_equal(got[k, j], other[s]) for j, s in enumerate(regs))
            told_apart = True
    assert told_apart


# ---- 2. every kernel family, small launches, against the oracle -----------------------------------------
GATES4 = lambda bce: [(bce.AND, 0, 1, 2), (bce.NOR, 0, 1, 3), (bce.XOR_FAST, 0, 1, 4), (bce.OR, 0, 1, 5, 1, 0)]


def _family(bce, c, os_, kmap, descs, base, fused=None):
    """K = len(kmap) instances of `descs` (inputs in slots 0, 1; plain gates) keyed by kmap against oracle eval_gates.
    fused: launches with the tail in the blind rotation's epilogue that the call must count, where the test knows it"""
    K, stride = len(kmap), 8
    n1 = c.n + 1
    c.pool_reserve(K * stride)
    ref = np.zeros((K, stride, n1), dtype=np.uint64)
    for k in range(K):
        o = os_[kmap[k]]
        ref[k, 0], ref[k, 1] = o.encrypt(k & 1, base + 2 * k), o.encrypt(1 - (k >> 1 & 1), base + 2 * k + 1)
        c.lwe_write([k * stride, k * stride + 1], ref[k, :2])
    t0 = c.timing()["fused_tail_launches"]
    c.EvalGates(descs, instances=K, slot_stride=stride, keysets=kmap)
    outs = [d[3] for d in descs]
    got = c.lwe_read([k * stride + s for k in range(K) for s in outs]).reshape(K, len(outs), n1)
    assert fused is None or c.timing()["fused_tail_launches"] == t0 + fused
    full = [tuple(d) + (0,) * (6 - len(d)) for d in descs]
    for k in range(K):
        pool = np.ascontiguousarray(ref[k])
        os_[kmap[k]].eval_gates(pool, full)
        assert np.array_equal(got[k], pool[outs]), "instance %d (set %d)" % (k, kmap[k])
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_std128_opt_every_blind_rotation_kernel(bce, orc, std_oracles, variant, monkeypatch):
    monkeypatch.setenv("BCE_VARIANT", str(variant))
    c, os_ = _keyed(bce, orc, 2, "STD128_OPT", oracles=std_oracles)
    # 12 workgroups: a small launch with the separate tail kernels, unless the two-per-CU build is forced (it carries its tail)
    _family(bce, c, os_, [1, 0, 1], GATES4(bce), 200 + 10 * variant, fused=1 if variant == 3 else 0)
    c.close()


def test_toy_ap(bce, orc):
    c, os_ = _keyed(bce, orc, 2, "TOY", method="AP")
    _family(bce, c, os_, [1, 0, 1], GATES4(bce), 300)
    c.close()


@pytest.fixture(scope="module")
def std192_oracles(orc):
    return _oracles(orc, 2, "STD192")


@pytest.mark.parametrize("fp64", ["default", "0"])
def test_std192_fp64_and_integer_bodies(bce, orc, std192_oracles, fp64, monkeypatch):
    if fp64 == "0":
        monkeypatch.setenv("BCE_FP64", "0")
    c, os_ = _keyed(bce, orc, 2, "STD192", oracles=std192_oracles)
    _family(bce, c, os_, [1, 0], GATES4(bce)[:2], 400)
    c.close()


@pytest.mark.parametrize("method", ["GINX", "AP"])
def test_four_digit_29_bit_modulus_narrow_kernel(bce, orc, method):
    c, os_ = _keyed(bce, orc, 2, method=method, custom=_custom_narrow(orc, 2048))
    _family(bce, c, os_, [1, 0], GATES4(bce)[:2], 500)
    c.close()


# ---- 3. saturated launches, STD128_OPT / GINX, default variant ----------------------------------------------------------------------
NB = 100
MAP6 = [1, 0, 1, 1, 0, 0]
_SAT = {}


def _saturated_inputs(bce, os_):
    """100 descriptors (every plain operation, folded NOTs, refreshes) and the inputs of six instances, instance k encrypted
    by oracle MAP6[k]; made once for both tests"""
    if not _SAT:
        rng = np.random.default_rng(4242)
        ops = [bce.OR, bce.AND, bce.NOR, bce.NAND, bce.XOR_FAST, bce.XNOR_FAST, bce.OP_REFRESH]
        descs = []
        for i in range(NB):
            op = ops[int(rng.integers(0, len(ops)))]
            descs.append((op, 2 * i, 2 * i + 1, 2 * NB + i, int(rng.integers(0, 2)), int(rng.integers(0, 2)) if op != bce.OP_REFRESH else 0))
        bits = rng.integers(0, 2, size=(6, 2 * NB))
        cts = np.stack([np.stack([os_[MAP6[k]].encrypt(int(bits[k, i]), 9000 + 1000 * k + i) for i in range(2 * NB)]) for k in range(6)])
        _SAT.update(descs=descs, cts=cts)
    return _SAT["descs"], _SAT["cts"]


def test_saturated_launch_with_the_fused_tail(std2, bce):
    """300 workgroups: more than the device's compute units, so the two-per-CU build with the tail in its epilogue"""
    c, os_ = std2
    descs, cts = _saturated_inputs(bce, os_)
    K, stride = 3, 3 * NB
    c.pool_reserve(6 * stride)
    for k in range(K):
        c.lwe_write(np.arange(k * stride, k * stride + 2 * NB, dtype=np.uint32), cts[k])
    t0 = c.timing()["fused_tail_launches"]
    c.EvalGates(descs, instances=K, slot_stride=stride, keysets=MAP6[:K])
    got = c.lwe_read([k * stride + 2 * NB + i for k in range(K) for i in range(NB)]).reshape(K, NB, -1)
    assert c.timing()["fused_tail_launches"] == t0 + 1
    for k in range(K):
        pool = np.zeros((stride, c.n + 1), dtype=np.uint64)
        pool[:2 * NB] = cts[k]
        os_[MAP6[k]].eval_gates(pool, descs)
        assert np.array_equal(got[k], pool[2 * NB:]), "instance %d (set %d)" % (k, MAP6[k])


def test_multi_round_launch_behind_the_xcd_start_gate(std2, bce):
    """600 workgroups: more than two per compute unit, so a second round of workgroups behind the per-XCD start gate.  The
    reference: per set, a fresh single-set context running the same descriptors unkeyed on that set's instances."""
    c, os_ = std2
    descs, cts = _saturated_inputs(bce, os_)
    K, stride = 6, 3 * NB
    c.pool_reserve(K * stride)
    for k in range(K):
        c.lwe_write(np.arange(k * stride, k * stride + 2 * NB, dtype=np.uint32), cts[k])
    c.EvalGates(descs, instances=K, slot_stride=stride, keysets=MAP6)
    got = c.lwe_read([k * stride + 2 * NB + i for k in range(K) for i in range(NB)]).reshape(K, NB, -1)
    for s in (0, 1):
        mine = [k for k in range(K) if MAP6[k] == s]
        ref = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
        ref.KeyGen(SEEDS[s])
        ref.pool_reserve(len(mine) * stride)
        for j, k in enumerate(mine):
            ref.lwe_write(np.arange(j * stride, j * stride + 2 * NB, dtype=np.uint32), cts[k])
        ref.EvalGates(descs, instances=len(mine), slot_stride=stride)
        want = ref.lwe_read([j * stride + 2 * NB + i for j in range(len(mine)) for i in range(NB)]).reshape(len(mine), NB, -1)
        ref.close()
        for j, k in enumerate(mine):
            assert np.array_equal(got[k], want[j]), "instance %d (set %d)" % (k, s)
    assert not np.array_equal(got[0], got[1])


# ---- 4. plans -------------------------------------------------------------------------------------------------------------------
def test_keyed_plan_step_by_step_and_as_a_graph(toy3, bce):
    c, os_ = toy3
    K, stride = 4, 16
    c.pool_reserve(3 * K * stride)
    steps = [[(bce.AND, 0, 1, 4), (bce.XOR, 0, 1, 5), (bce.PAIR(bce.OR, bce.NAND), 0, 1, 6)],
             [(bce.OR, 4, 5, 8), (bce.NAND, 6, 7, 9, 1, 0)],
             [(bce.XOR_FAST, 8, 9, 10), (bce.OP_REFRESH, 9, 9, 11)]]
    flat = [d for st in steps for d in st]
    regs = _written(bce, flat)
    ins = []
    for k in range(K):
        o = os_[MAP4[k]]
        ins.append({0: o.encrypt(k & 1, 600 + 2 * k), 1: o.encrypt(1 - (k >> 1), 601 + 2 * k)})
        for copy in range(3):
            base = (copy * K + k) * stride
            c.lwe_write([base, base + 1], np.stack([ins[k][0], ins[k][1]]))
    read = lambda copy: c.lwe_read([(copy * K + k) * stride + s for k in range(K) for s in regs])
    for st in steps:                                                    # copy 0: keyed calls, frontier by frontier
        c.EvalGates(st, instances=K, slot_stride=stride, keysets=MAP4)
    called = read(0)
    plan = c.plan_create(steps, instances=K, slot_stride=stride, slot_base=K * stride, keysets=MAP4)
    for s in range(len(steps)):
        c.plan_run_step(plan, s)
    stepped = read(1)
    plan2 = c.plan_create(steps, instances=K, slot_stride=stride, slot_base=2 * K * stride, keysets=MAP4)
    c.keyset_select(1)                                                  # a keyed plan does not follow the selection
    c.plan_run(plan2)
    c.keyset_select(0)
    c.plan_run(plan2)                                                   # replay of the same graph (idempotent: inputs are not overwritten)
    graphed = read(2)
    c.plan_destroy(plan)
    c.plan_destroy(plan2)
    assert np.array_equal(called, stepped) and np.array_equal(called, graphed)
    called = called.reshape(K, len(regs), -1)
    for k in range(K):
        want = _replay(os_[MAP4[k]], ins[k], flat)
        for j, s in enumerate(regs):
            assert np.array_equal(called[k, j], want[s]), "instance %d (set %d) register %d" % (k, MAP4[k], s)


# ---- 5. the selection rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["TOY", "split"])
def test_a_call_without_a_map_acts_on_the_selected_set(bce, orc, shape, toy3):
    """TOY has no persistent kernel (bce_dag_supported is 0 there), so the dag_run part runs on the smallest shape that has one,
    the `split` shape of the noise tests (n = 32, N = 1024, four digits), which repeats every other check as well."""
    if shape == "TOY":
        c, os_ = toy3
        assert not c.dag_supported()
    else:
        c, os_ = _keyed(bce, orc, 2, custom=noise_run.shapes(orc.lib(), None)["split"][1])
        assert c.dag_supported()
    c.pool_reserve(16)
    dag = c.dag_create([(bce.NAND, 0, 1, 6), (bce.OR, 6, 0, 7, 0, 1)]) if c.dag_supported() else None
    for sel in (1, 0):
        o = os_[sel]
        c.keyset_select(sel)
        assert c.keyset_selected() == sel
        s, z = c.export_sk()
        assert np.array_equal(s, o.sk()) and np.array_equal(z, o.z())
        assert np.array_equal(c.export_bsk(), o.bsk()) and np.array_equal(c.export_ksk(), o.ksk())
        c.set_encrypt_seed(SEEDS[sel])
        c.Encrypt([0, 1], [0, 1], enc_index_base=40)
        c.Encrypt([1, 0], [2, 3], enc_index_base=50, mode=bce.BOOTSTRAPPED)
        got = c.lwe_read([0, 1, 2, 3])
        ca, cb = o.encrypt(0, 40), o.encrypt(1, 41)
        assert np.array_equal(got[0], ca) and np.array_equal(got[1], cb)
        assert np.array_equal(got[2], o.bootstrap(o.encrypt(1, 50))) and np.array_equal(got[3], o.bootstrap(o.encrypt(0, 51)))
        assert list(c.Decrypt([0, 1, 2, 3])) == [0, 1, 1, 0]
        c.EvalGates([(bce.AND, 0, 1, 4), (bce.OR, 0, 1, 5, 1, 0)])
        out = c.lwe_read([4, 5])
        assert np.array_equal(out[0], o.eval_bingate(bce.AND, ca, cb)) and np.array_equal(out[1], o.eval_bingate(bce.OR, o.eval_not(ca), cb))
        if dag is not None:
            c.dag_run(dag)
            out = c.lwe_read([6, 7])
            t = o.eval_bingate(bce.NAND, ca, cb)
            assert np.array_equal(out[0], t) and np.array_equal(out[1], o.eval_bingate(bce.OR, t, o.eval_not(ca)))
        c.set_encrypt_seed(None)
    assert c.keyset_selected() == 0
    if dag is not None:
        c.dag_destroy(dag)
        c.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def _code(bce, call):
    with pytest.raises(bce.BceError) as e:
        call()
    return e.value.code


def test_errors(bce, orc):
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(SEEDS[0])
    assert c.keyset_add() == 1
    c.keyset_select(1)
    c.KeyGen(SEEDS[1])
    c.keyset_select(0)
    c.pool_reserve(32)
    c.Encrypt([1, 0, 1, 1], [0, 1, 16, 17])
    g = [(bce.AND, 0, 1, 2)]
    c.EvalGates(g, instances=2, slot_stride=16, keysets=[1, 0])
    assert _code(bce, lambda: c.EvalGates(g, instances=2, slot_stride=16, keysets=[0, 7])) == bce.ERR_ARG       # no such set
    assert _code(bce, lambda: c.EvalGates(g, instances=2, slot_stride=16, keysets=[0, 256])) == bce.ERR_ARG
    assert _code(bce, lambda: c.keyset_select(7)) == bce.ERR_ARG
    assert c.keyset_add() == 2                                                                                    # a set without keys
    assert _code(bce, lambda: c.EvalGates(g, instances=2, slot_stride=16, keysets=[0, 2])) == bce.ERR_NO_KEYS
    assert _code(bce, lambda: c.plan_create([g], instances=2, slot_stride=16, keysets=[2, 0])) == bce.ERR_NO_KEYS
    c.keyset_select(2)
    assert _code(bce, lambda: c.EvalGates(g)) == bce.ERR_NO_KEYS
    assert _code(bce, lambda: c.Decrypt([0])) == bce.ERR_NO_KEYS
    assert _code(bce, lambda: c.keyset_drop(2)) == bce.ERR_ARG                                                    # the selected set
    c.keyset_select(0)
    assert _code(bce, lambda: c.keyset_drop(0)) == bce.ERR_ARG                                                    # set 0
    assert _code(bce, lambda: c.keyset_drop(9)) == bce.ERR_ARG
    plan = c.plan_create([g], instances=2, slot_stride=16, keysets=[1, 0])
    assert _code(bce, lambda: c.keyset_drop(1)) == bce.ERR_STATE                                                  # named by a live plan
    assert _code(bce, lambda: c.plan_set_checks(plan, [[2]])) == bce.ERR_UNSUPPORTED
    c.plan_run(plan)
    c.plan_destroy(plan)
    c.keyset_drop(1)
    assert c.keyset_count() == 2
    assert _code(bce, lambda: c.EvalGates(g, instances=2, slot_stride=16, keysets=[1, 0])) == bce.ERR_ARG       # dropped
    assert c.keyset_add() == 1                                                                                    # the lowest free id again
    ids = [c.keyset_add() for _ in range(253)]
    assert ids == list(range(3, 256)) and c.keyset_count() == 256
    assert _code(bce, c.keyset_add) == bce.ERR_ARG                                                                # the 257th set
    assert c.keyset_count() == 256
    c.EvalGates(g)                                                                                                # set 0 still works
    assert list(c.Decrypt([2])) == [0]
    c.close()


# ---- 7. the circuit runtime: one key set per instance ------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["steps", "graph"])
def test_circuit_instances_under_their_own_key_sets(toy3, bce, graph):
    """adder_2bit at TOY, K = 4 instances under sets [2, 0, 2, 1], another plaintext input each: Outputs(k), and every
    bootstrapped register of instance k against the oracle MAP4[k] replay of relevel_plan() from that instance's input registers."""
    import os
    from kat import CIRCUITS
    cc, os_ = toy3
    c = bce.Circuit(cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    K = 4
    c.setInstances(K)
    c.setInstanceKeys(MAP4)
    c.setGraph(graph)
    c.Reset()
    c.setEncrypted(True)
    steps = c.relevel_plan()
    flat = [d for st in steps for d in st]
    stride = c.info()["slot_stride"]
    ab = [(3, 2), (1, 3), (2, 2), (0, 1)]
    for k, (a, b) in enumerate(ab):
        c.SetInput([[a & 1, a >> 1], [b & 1, b >> 1]], instance=k)
    assert cc.keyset_selected() == 0                                   # the selection is restored after every SetInput
    ins = [dict(enumerate(cc.lwe_read(np.arange(k * stride, k * stride + 4, dtype=np.uint32)))) for k in range(K)]
    for k in range(K):                                                 # the inputs are ciphertexts of their own set
        assert [os_[MAP4[k]].decrypt(ins[k][w]) for w in range(4)] == [ab[k][0] & 1, ab[k][0] >> 1, ab[k][1] & 1, ab[k][1] >> 1]
    c.Clock()
    assert c.graphActive() == graph and cc.keyset_selected() == 0
    regs = _written(bce, flat)
    for k, (a, b) in enumerate(ab):
        out = c.Outputs(k)[0]
        assert out[0] + 2 * out[1] + 4 * out[2] == a + b, "instance %d" % k
        want = _replay(os_[MAP4[k]], ins[k], flat)
        got = cc.lwe_read([k * stride + s for s in regs])
        for j, s in enumerate(regs):
            assert np.array_equal(got[j], want[s]), "instance %d (set %d) register %d" % (k, MAP4[k], s)
    c.close()


def test_circuit_refuses_what_per_instance_keys_do_not_run(toy3, bce):
    import os
    from kat import CIRCUITS
    cc, _ = toy3
    path = os.path.join(CIRCUITS, "adder_2bit.out")

    def circuit():
        c = bce.Circuit(cc)
        c.ReadFile(path)
        c.setInstances(4)
        return c

    for setter in ("setDataflow", "setVerify", "setDeviceVerify"):
        c = circuit()                                                  # keys first, then the option
        c.setInstanceKeys(MAP4)
        assert _code(bce, lambda: getattr(c, setter)(True)) == bce.ERR_UNSUPPORTED, setter
        c.close()
        c = circuit()                                                  # the option first, then the keys
        getattr(c, setter)(True)
        assert _code(bce, lambda: c.setInstanceKeys(MAP4)) == bce.ERR_UNSUPPORTED, setter
        c.close()
    shard = lambda c: c.set_exchange(0, 2, 1, lambda nbytes, on_dev: 0, None, None, None, None, 0)   # gate sharding over two ranks
    c = circuit()
    c.setInstanceKeys(MAP4)
    assert _code(bce, lambda: shard(c)) == bce.ERR_UNSUPPORTED
    c.close()
    c = circuit()
    shard(c)
    assert _code(bce, lambda: c.setInstanceKeys(MAP4)) == bce.ERR_UNSUPPORTED
    c.close()
    c = circuit()
    assert _code(bce, lambda: c.setInstanceKeys([0, 1])) == bce.ERR_ARG     # one id per instance
    c.setInstanceKeys(MAP4)
    c.Reset()
    c.setEncrypted(True)
    c.SetInput([[1, 1], [0, 1]])
    assert _code(bce, lambda: c.setInstanceKeys(MAP4)) == bce.ERR_STATE     # before SetInput
    c.close()
