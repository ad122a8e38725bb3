"""Pair descriptors (BCE_PAIR, include/bce_gpu.h) on the device: two gates from one blind rotation, against the reference of
tests/pair_model.py (the oracle's own stages on the rotated accumulator), word for word at every stage, on every path a
launch can take: separate tail kernels (lone launches, all four kernel families) and the fused epilogue (saturated launches
of the split-transform kernel, the fp64 AP kernel).  Shapes are the cheap ones of noise_run.shapes (n = 32 / 16)."""
import numpy as np
import pytest

import noise_run
import pair_model as pm

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


def _cases(o, pairs, base, inputs=((0, 0), (0, 1), (1, 0), (1, 1)), k0=0):
    """(op, op2, a, b, neg0, neg1, ca, cb) with fresh oracle encryptions; every third case folds a NOT into an input"""
    cases, idx = [], base
    for op, op2 in pairs:
        for a, b in inputs:
            k = k0 + len(cases)
            cases.append((op, op2, a, b, 1 if k % 3 == 1 else 0, 1 if k % 6 == 4 else 0, o.encrypt(a, idx), o.encrypt(b, idx + 1)))
            idx += 2
    return cases


def _load(c, cases, extra=0):
    """inputs of case i in slots 2i, 2i + 1; outputs of case i in slots 2 nb + 2i, 2 nb + 2i + 1"""
    nb = len(cases)
    c.pool_reserve(4 * nb + extra)
    c.lwe_write(np.arange(2 * nb, dtype=np.uint32), np.concatenate([np.stack([x[6], x[7]]) for x in cases]))
    return [(pm.PAIR(x[0], x[1]), 2 * i, 2 * i + 1, 2 * nb + 2 * i, x[4], x[5]) for i, x in enumerate(cases)]


_REF = {}     # the reference of a case is computed once and shared by the tests that meet the case again


def _reference(o, op, op2, ca, cb, n0, n1):
    key = (id(o), op, op2, n0, n1, ca.tobytes(), cb.tobytes())
    if key not in _REF:
        _REF[key] = pm.stages(o, op, op2, ca, cb, n0, n1)
    return _REF[key]


def _assert_reference(o, c, cases, acc, lweN, ks, out, what):
    nb = len(cases)
    for i, (op, op2, a, b, n0, n1, ca, cb) in enumerate(cases):
        r = _reference(o, op, op2, ca, cb, n0, n1)
        assert np.array_equal(acc[i], r["acc"]), "%s: accumulator, case %d" % (what, i)
        for second, row in ((0, i), (1, nb + i)):
            assert np.array_equal(lweN[row], r["lweN"][second]), "%s: extract + ModSwitch, case %d output %d" % (what, i, second)
            assert np.array_equal(ks[row], r["ks"][second]), "%s: KeySwitch, case %d output %d" % (what, i, second)
            assert np.array_equal(out[2 * i + second], r["out"][second]), "%s: pool row, case %d output %d" % (what, i, second)
        assert o.decrypt(out[2 * i]) == pm.truth(op, a ^ n0, b ^ n1), (what, i)
        assert o.decrypt(out[2 * i + 1]) == pm.truth(op2, a ^ n0, b ^ n1), (what, i)


def _run(c, descs):
    nb = len(descs)
    acc, lweN, ks = c.debug_eval_stages(descs)
    assert acc.shape[0] == nb and lweN.shape[0] == 2 * nb and ks.shape[0] == 2 * nb
    return acc, lweN, ks, c.lwe_read(np.arange(2 * nb, 4 * nb, dtype=np.uint32))


# ---- 1. the one-wave-per-transform family ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GINX", "AP"])
def test_toy_every_ordered_pair_every_stage(bce, oracles, method):
    o, c = _engine(bce, oracles, "TOY", method)
    cases = _cases(o, pm.ORDERED_PAIRS, 100)
    assert len(cases) == 48 and any(x[4] for x in cases) and any(x[5] for x in cases)
    t0 = c.timing()
    acc, lweN, ks, out = _run(c, _load(c, cases))
    t1 = c.timing()
    assert t1["bootstraps"] - t0["bootstraps"] == 48          # blind rotations: a pair counts 1
    _assert_reference(o, c, cases, acc, lweN, ks, out, "TOY " + method)
    bits = c.Decrypt(np.arange(2 * 48, 4 * 48, dtype=np.uint32))
    for i, (op, op2, a, b, n0, n1, _, _) in enumerate(cases):
        assert (bits[2 * i], bits[2 * i + 1]) == (pm.truth(op, a ^ n0, b ^ n1), pm.truth(op2, a ^ n0, b ^ n1))
    c.close()


# ---- 2. the split-transform family: separate tail kernels and the fused epilogue ------------------------------------------------------
def _six(o, base):
    inputs = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 0), (0, 1)]
    return [x for k, pr in enumerate(pm.DISTINCT_PAIRS) for x in _cases(o, [pr], base + 2 * k, inputs=[inputs[k]], k0=k)]


@pytest.mark.parametrize("shape", ["split", "STD128_OPT"])
def test_split_family_lone_and_saturated_launch(bce, oracles, shape):
    o, c = _engine(bce, oracles, shape, "GINX")
    cases = _six(o, 300)
    nb, big_n = len(cases), 300
    assert nb == 6
    lone = _load(c, cases, extra=2 * big_n)
    t0 = c.timing()["fused_tail_launches"]
    acc, lweN, ks, out = _run(c, lone)
    assert c.timing()["fused_tail_launches"] == t0, "a lone launch keeps the separate tail kernels"
    _assert_reference(o, c, cases, acc, lweN, ks, out, shape + " lone")
    big = [(lone[i % nb][0], lone[i % nb][1], lone[i % nb][2], 4 * nb + 2 * i, lone[i % nb][4], lone[i % nb][5]) for i in range(big_n)]
    acc_b, lweN_b, ks_b = c.debug_eval_stages(big)
    assert c.timing()["fused_tail_launches"] == t0 + 1, "a saturated launch runs the tail in the epilogue"
    out_b = c.lwe_read(np.arange(4 * nb, 4 * nb + 2 * big_n, dtype=np.uint32))
    for i in range(big_n):
        k = i % nb
        assert np.array_equal(acc_b[i], acc[k]), "accumulator, gate %d" % i
        for second, row_b, row in ((0, i, k), (1, big_n + i, nb + k)):
            assert np.array_equal(lweN_b[row_b], lweN[row]), "extract + ModSwitch, gate %d output %d" % (i, second)
            assert np.array_equal(ks_b[row_b], ks[row]), "KeySwitch, gate %d output %d" % (i, second)
            assert np.array_equal(out_b[2 * i + second], out[2 * k + second]), "pool row, gate %d output %d" % (i, second)
    c.close()


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("shape", ["split", "STD128_OPT"])
def test_split_family_lone_launch_under_every_kernel(bce, oracles, shape, variant, monkeypatch):
    monkeypatch.setenv("BCE_VARIANT", str(variant))
    o, c = _engine(bce, oracles, shape, "GINX")
    cases = _six(o, 300)
    acc, lweN, ks, out = _run(c, _load(c, cases))
    _assert_reference(o, c, cases, acc, lweN, ks, out, "%s BCE_VARIANT=%d" % (shape, variant))
    c.close()


# ---- 3. the 64-bit families --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,method,fp64", [("std192_like", "AP", "1"), ("std192_like", "GINX", "1"), ("std192_like", "AP", "0"),
                                               ("std192_like", "GINX", "0"), ("int64_40", "GINX", "1")])
def test_word64_families(bce, oracles, shape, method, fp64, monkeypatch):
    monkeypatch.setenv("BCE_FP64", fp64)
    o, c = _engine(bce, oracles, shape, method)
    pairs = [(pm.OR, pm.NAND), (pm.AND, pm.NOR), (pm.NAND, pm.OR), (pm.NOR, pm.AND)]
    cases = [x for k, pr in enumerate(pairs) for x in _cases(o, [pr], 700 + 2 * k, inputs=[((k >> 1) & 1, k & 1)], k0=k)]
    descs = _load(c, cases)
    t0 = c.timing()["fused_tail_launches"]
    acc, lweN, ks, out = _run(c, descs)
    fused = c.timing()["fused_tail_launches"] - t0
    _assert_reference(o, c, cases, acc, lweN, ks, out, "%s %s BCE_FP64=%s" % (shape, method, fp64))
    # the fp64 AP build with the folded key carries its tail, at any launch size; no other build of these families does
    assert fused == (1 if method == "AP" and c.fp64() and c.forward_transforms_per_step() == 2 * o.params["dG"] - 2 else 0)
    assert fused or (shape, method, fp64) != ("std192_like", "AP", "1")
    if fused:
        # the same launch through the separate tail kernels, on the device
        monkeypatch.setenv("BCE_FUSE_TAIL", "0")
        _, c2 = _engine(bce, oracles, shape, method)
        _load(c2, cases)
        t0 = c2.timing()["fused_tail_launches"]
        acc2, lweN2, ks2, out2 = _run(c2, descs)
        assert c2.timing()["fused_tail_launches"] == t0
        assert np.array_equal(acc2, acc) and np.array_equal(lweN2, lweN) and np.array_equal(ks2, ks) and np.array_equal(out2, out)
        c2.close()
    c.close()


# ---- 4. plain and pair descriptors in one call, instances --------------------------------------------------------------------------
def test_mixed_call_with_instances_and_a_plan(bce, oracles):
    o, c = _engine(bce, oracles, "TOY", "GINX")
    K, stride = 3, 16
    c.pool_reserve(2 * K * stride)
    ins = []
    for k in range(K):
        ca, cb = o.encrypt(k & 1, 900 + 2 * k), o.encrypt(1 - (k >> 1), 901 + 2 * k)
        ins.append((k & 1, 1 - (k >> 1), ca, cb))
        c.lwe_write([k * stride, k * stride + 1], np.stack([ca, cb]))
        c.lwe_write([(K + k) * stride, (K + k) * stride + 1], np.stack([ca, cb]))
    plain = [(bce.NAND, 0, 1, 2), (bce.OR, 1, 0, 3, 1, 0), (bce.OP_REFRESH, 0, 0, 4)]
    mixed = [plain[0], (bce.PAIR(bce.OR, bce.NAND), 0, 1, 8), plain[1], (bce.PAIR(bce.AND, bce.NOR), 0, 1, 10, 0, 1), plain[2]]
    t0 = c.timing()["bootstraps"]
    c.EvalGates(mixed, instances=K, slot_stride=stride)
    assert c.timing()["bootstraps"] - t0 == 5 * K
    base2 = K * stride          # the same plain descriptors alone, on a second copy of the inputs
    c.EvalGates([(d[0], d[1] + base2, d[2] + base2, d[3] + base2) + tuple(d[4:]) for d in plain], instances=K, slot_stride=stride)
    for k, (a, b, ca, cb) in enumerate(ins):
        got = c.lwe_read([k * stride + s for s in (2, 3, 4, 8, 9, 10, 11)])
        alone = c.lwe_read([base2 + k * stride + s for s in (2, 3, 4)])
        assert np.array_equal(got[:3], alone), "plain descriptors next to pairs, instance %d" % k
        assert np.array_equal(got[0], o.eval_bingate(bce.NAND, ca, cb))
        r = pm.stages(o, pm.OR, pm.NAND, ca, cb)
        assert np.array_equal(got[3], r["out"][0]) and np.array_equal(got[4], r["out"][1]), "pair at out, out + 1, instance %d" % k
        r = pm.stages(o, pm.AND, pm.NOR, ca, cb, 0, 1)
        assert np.array_equal(got[5], r["out"][0]) and np.array_equal(got[6], r["out"][1])
        assert [o.decrypt(x) for x in got[3:]] == [a | b, 1 - (a & b), a & (1 - b), 1 - (a | (1 - b))]
    # the same frontier, then AND(t, t + 1) = XOR, as a resident plan: stepped and as one graph
    steps = [[(bce.PAIR(bce.OR, bce.NAND), 0, 1, 5), plain[0]], [(bce.AND, 5, 6, 7)]]
    plan = c.plan_create(steps, instances=K, slot_stride=stride)
    t0 = c.timing()["bootstraps"]
    c.plan_run_step(plan, 0)
    c.plan_run_step(plan, 1)
    assert c.timing()["bootstraps"] - t0 == 3 * K
    stepped = c.lwe_read([k * stride + s for k in range(K) for s in (5, 6, 7)])
    c.lwe_write([k * stride + s for k in range(K) for s in (5, 6, 7)], np.zeros_like(stepped))
    c.plan_run(plan)
    graphed = c.lwe_read([k * stride + s for k in range(K) for s in (5, 6, 7)])
    assert np.array_equal(stepped, graphed)
    for k, (a, b, ca, cb) in enumerate(ins):
        assert np.array_equal(stepped[3 * k + 2], pm.xor_shared(o, ca, cb))
        assert o.decrypt(stepped[3 * k + 2]) == a ^ b
    c.plan_destroy(plan)
    c.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_illegal_pairs_pool_bound_and_the_dataflow_kernel(bce, oracles):
    o, c = _engine(bce, oracles, "split", "GINX")
    c.pool_reserve(8)
    c.Encrypt(np.array([0, 1], dtype=np.uint8), np.arange(2, dtype=np.uint32))
    bad = [bce.PAIR(bce.OR, bce.OR), bce.PAIR(bce.XOR_FAST, bce.AND), bce.PAIR(bce.AND, bce.XNOR_FAST), bce.PAIR(bce.OP_REFRESH, bce.AND),
           bce.PAIR(bce.AND, bce.OP_NOT), bce.PAIR(bce.OP_COPY, bce.OR), bce.PAIR(bce.OR, bce.NAND) | (1 << 16), bce.AND | (200 << 8)]
    for op in bad:
        for call in (lambda d: c.EvalGates(d), lambda d: c.plan_create([d]), lambda d: c.debug_eval_stages(d)):
            with pytest.raises(bce.BceError) as e:
                call([(op, 0, 1, 2)])
            assert e.value.code == bce.ERR_ARG, hex(op)
    ok = bce.PAIR(bce.OR, bce.NAND)
    c.EvalGates([(ok, 0, 1, 6)])                                   # out + 1 = 7: the last slot
    assert list(c.Decrypt(np.array([6, 7], dtype=np.uint32))) == [1, 1]
    for call in (lambda d: c.EvalGates(d), lambda d: c.plan_create([d]), lambda d: c.EvalGates(d, instances=2, slot_stride=0)):
        with pytest.raises(bce.BceError) as e:
            call([(ok, 0, 1, 7)])                                  # out is inside the pool, out + 1 is not
        assert e.value.code == bce.ERR_POOL
    with pytest.raises(bce.BceError) as e:
        c.EvalGates([(ok, 0, 1, 2)], instances=2, slot_stride=5)   # 2 + 1 + 5 = 8
    assert e.value.code == bce.ERR_POOL
    assert c.dag_supported()
    with pytest.raises(bce.BceError) as e:
        c.dag_create([(bce.AND, 0, 1, 2), (ok, 0, 2, 4)])
    assert e.value.code == bce.ERR_UNSUPPORTED and "pair" in str(e.value)
    c.close()
