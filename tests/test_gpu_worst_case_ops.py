"""Worst-case operands for the descriptors with two real inputs: BCE_XOR, BCE_PAIR, the LWE preparation and the persistent kernel.

tests/test_gpu_worst_case.py feeds every gate the all-zero second input with neg0 = neg1 = 0 and knows only the plain gates'
test polynomial.  This file takes its row table (every kernel class, selector and largest modulus), its key families and
its steering, and runs, through bce_debug_eval_stages and bit for bit at all four stages (a pair: the shared accumulator and
both outputs' three later stages, second outputs after the first in descriptor order):

  edges      worst_case.two_operand_cases -- a chosen prepared word vector split into two non-trivial operands under all four
             negation combinations, sums that wrap mod q; BCE_XOR's three-level polynomial on both sides of its four window
             boundaries under every a pattern; all 12 ordered pairs on the window edges of both gates and on the unrotated
             polynomial (a = 0); the four plain gates as a check of the preparation alone -- under the key families of the
             existing suite;
  steered    BCE_XOR and pairs steered (first-step key solved for their own polynomial) to every target of target_polys;
             BCE_XOR to the RoundqQ boundary accumulators of its own tail (no Q/8 + 1 added: the only way to hand that tail a
             chosen accumulator); pairs to X^(2N - e) A2, so that the SECOND tail reads the boundary accumulator A2 -- with 0
             and Q - 1 at the wrap index and at negated positions -- through the rotation, e = N/2, N, 3N/2 in turn;
  saturated  the same descriptors replicated into one launch with the fused tail (also with qKS = 2^26 and 2^29);
  dataflow   the edge descriptors as one k_bootstrap_dag run of two instances under crafted keys: pool rows equal the step
             path's (stages do not leave the persistent kernel).

References import nothing of the engine: xor_single_model.stages (BCE_XOR), pair_model.stages (pairs), the oracle's stages
(plain gates).  Nothing is decrypted: crafted keys encrypt nothing.  The CPU half (not marked gpu) asserts on the oracle and
the models alone that the operands are what they claim: case counts, boundaries, pairs, negations, targets reached.
"""
import numpy as np
import pytest

import pair_model as pm
import test_gpu_worst_case as base
import worst_case as wc
import xor_single_model as xm
from test_gpu_worst_case import CPU_ROWS, FUSED_PARAMS, ROW_PARAMS, ROWS, Row

gpu = pytest.mark.gpu
XOR_POLY = lambda o, op, b: xm.xor_poly(o.params, b)                       # polynomial makers for wc.steered_keys
FIRST_GATE_POLY = lambda o, op, b: wc.test_vector(o, op & 0xFF, b)
PAIR_WORDS = tuple(wc.pair_word(a, b) for a, b in wc.ORDERED_PAIRS)
LATER = base.STAGES[1:]


# ---- keys, references, layout ------------------------------------------------------------------------------------------------
def _install(o, c, bsk, ksk):
    """the same caller-made key words on both sides (c None: the oracle alone); the model's key cache belongs to the old key"""
    s, z = wc.zero_secret(o)
    o.import_keys_eval(s, z, bsk, ksk)
    o._xor_single_keys = None
    if c is not None:
        c.import_keys_eval(s, z, bsk.reshape(-1), ksk.reshape(-1))


def _reference(o, case):
    """(accumulator, [(lweN, ks, pool row) per output]) of a case (name, op, ct1, ct2, neg0, neg1, prep)"""
    _, op, ct1, ct2, n0, n1, prep = case
    if op == wc.XOR:
        r = xm.stages(o, ct1, ct2, n0, n1)
        return r["acc"], [(r["lweN"], r["ks"], r["out"])]
    if wc.is_pair(op):
        r = pm.stages(o, op & 0xFF, (op >> 8) - 1, ct1, ct2, n0, n1)
        return r["acc"], [(r["lweN"][s], r["ks"][s], r["out"][s]) for s in (0, 1)]
    a, b = (o.eval_not(ct1) if n0 else ct1), (o.eval_not(ct2) if n1 else ct2)
    acc, lweN, ks, out = base._oracle_stages(o, op, o.gate_prep(op, a, b))
    return acc, [(lweN, ks, out)]


def _load(c, cases, extra=0, copies=1):
    """inputs of case i in slots 2i, 2i + 1, its outputs in 2 nb + 2i (and + 1: a pair's second); `copies` such blocks of 4 nb
    slots back to back, `extra` slots behind them.  Returns the descriptors of block 0."""
    nb = len(cases)
    c.pool_reserve(4 * nb * copies + extra)
    ins = np.concatenate([np.stack([x[2], x[3]]) for x in cases])
    for k in range(copies):
        c.lwe_write(np.arange(4 * nb * k, 4 * nb * k + 2 * nb, dtype=np.uint32), ins)
    return [(x[1], 2 * i, 2 * i + 1, 2 * nb + 2 * i, x[4], x[5]) for i, x in enumerate(cases)]


def _engine_stages(c, descs, out_base):
    """[(accumulator, [(lweN, ks, pool row) per output])] per descriptor, outputs of descriptor i at out_base + 2i (+ 1)"""
    nb = len(descs)
    acc, lweN, ks = c.debug_eval_stages(descs)
    assert acc.shape[0] == nb and lweN.shape[0] == ks.shape[0] == nb + sum(1 for d in descs if wc.is_pair(d[0]))
    out = c.lwe_read(np.arange(out_base, out_base + 2 * nb, dtype=np.uint32))
    res, second = [], nb
    for i, d in enumerate(descs):
        outs = [(lweN[i], ks[i], out[2 * i])]
        if wc.is_pair(d[0]):
            outs.append((lweN[second], ks[second], out[2 * i + 1]))
            second += 1
        res.append((np.array(acc[i]), outs))
    return res


def _first_difference(got, want):
    """None, or (stage name, index, engine word, reference word) of the first stage that differs"""
    if not np.array_equal(got[0], want[0]):
        k = int(np.flatnonzero(got[0] != want[0])[0])
        return base.STAGES[0], k, int(got[0][k]), int(want[0][k])
    assert len(got[1]) == len(want[1])
    for s, (g3, w3) in enumerate(zip(got[1], want[1])):
        for stage, g, w in zip(LATER, g3, w3):
            if not np.array_equal(g, w):
                k = int(np.flatnonzero(g != w)[0])
                return stage + (" (second output)" if s else ""), k, int(g[k]), int(w[k])
    return None


def _run_and_compare(o, c, cases, what):
    """small launch of every case, every stage against the reference; returns (failures, engine results)"""
    nb = len(cases)
    got = _engine_stages(c, _load(c, cases), 2 * nb)
    bad = []
    for i, case in enumerate(cases):
        d = _first_difference(got[i], _reference(o, case))
        if d:
            bad.append("%s | %s | %s: first difference at %d: engine %d, reference %d" % ((what, case[0]) + d))
    return bad, got


def _finish(o, c, bad):
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- steering ------------------------------------------------------------------------------------------------------------
def _as_cases(o, steered):
    """steered_keys' (name, op, prepared, first-step-only prepared, target) as two-operand cases: the prepared words split
    into two real operands, negations in turn; the first-step-only ciphertexts follow the two-step ones"""
    q = o.params["q"]
    two, one = [], []
    for i, (name, op, prep, first, _) in enumerate(steered):
        for k, (lst, p, suffix) in enumerate(((two, prep, ""), (one, first, " (first step only)"))):
            n0, n1 = wc.NEGATIONS[(i + k) % 4]
            ct1, ct2 = wc.split_operands(q, p, n0, n1)
            lst.append(("%s %s neg=%d%d%s" % (name, wc.op_name(op), n0, n1, suffix), op, ct1, ct2, n0, n1, p))
    return two + one


def _chunks(o, targets, seconds, rng, what, gates, poly):
    """key sets of at most n/2 targets each: [(what, bsk, steered cases)]; gates: one word per target, or a cycle for all"""
    per = o.n // 2
    out = []
    for second in seconds:
        for lo in range(0, len(targets), per):
            g = gates[lo:lo + per] if len(gates) == len(targets) else gates
            bsk, steered = wc.steered_keys(o, targets[lo:lo + per], second, rng, gates=tuple(g), poly=poly)
            out.append(("%s, second key %s" % (what, second), bsk, steered))
    return out


def _xor_boundary_targets(o, rng):
    return [("coeff RoundqQ boundaries of the offset-free tail %d" % k, "coeff", a) for k, a in enumerate(base._tail_accumulators(o, rng, off=0))]


def _pair_boundary_targets(o, rng):
    """([(name, form, target)], [pair word], [A2])"""
    rot = base._rotated_tail_targets(o, rng, base.EXPONENT_PAIRS)
    return ([("coeff rotated RoundqQ boundaries %d" % k, "coeff", t) for k, (_, t, _) in enumerate(rot)], [w for w, _, _ in rot],
            [a for _, _, a in rot])


def _steered_op_sets(o, rng, polys=True, seconds=("Q-1", "uniform"), boundary_seconds=("Q-1", "uniform")):
    """[(what, bsk, steered cases)]: BCE_XOR and pairs to target_polys (second-step key all Q - 1 and uniform) and to their
    tails' boundary accumulators"""
    out = []
    if polys:
        out += _chunks(o, wc.target_polys(o, rng), seconds, rng, "XOR steered", (wc.XOR,), XOR_POLY)
        out += _chunks(o, wc.target_polys(o, rng), seconds, rng, "pairs steered", PAIR_WORDS, FIRST_GATE_POLY)
    out += _chunks(o, _xor_boundary_targets(o, rng), boundary_seconds, rng, "XOR steered to its tail's boundaries", (wc.XOR,), XOR_POLY)
    targets, words, _ = _pair_boundary_targets(o, rng)
    out += _chunks(o, targets, boundary_seconds, rng, "pairs steered to the second tail's boundaries", words, FIRST_GATE_POLY)
    return out


KEY_FAMILIES = base.KEY_FAMILIES


# ---- GPU: two-operand edge cases under extreme keys ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_xor_and_pair_edges_under_extreme_keys(bce, orc, monkeypatch, row):
    """family `edges`: all two-operand cases under keys of all Q - 1 / qKS - 1 and uniform with forced ends, the cases without
    the per-boundary b sweeps under all 1, all 0 and alternating rows; every stage equals the reference's.  Trimmed, in those
    three subset families only (the numpy reference of BCE_XOR is what an id's time goes to): BCE_XOR keeps one b per a
    pattern -- still all ten b values -- and a pair its a = 0 case and the first edge under a=cycle.  After the trim an id still
    takes about 1.2 times test_edge_ciphertexts_under_extreme_keys of the same row (slowest on MI355X: 3.58 s against 3.14 s,
    narrow64_N2048-default-AP), because the two full families alone cost more than that id: 30 (AP: 38) numpy blind rotations
    each, 20 - 40 ms apiece at N = 2048, where the existing test's reference is the oracle's C."""
    o, c = base._pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3911)
    cases = wc.two_operand_cases(o)
    bad = []
    for bpat, kpat, subset in KEY_FAMILIES:
        _install(o, c, wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng))
        bad += _run_and_compare(o, c, wc.operand_subset(cases) if subset else cases, "bsk %s, ksk %s" % (bpat, kpat))[0]
    _finish(o, c, bad)


# ---- GPU: steered accumulators -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_xor_and_pair_steered_accumulator(bce, orc, monkeypatch, row):
    """family `steered`: after the first executed step the accumulator is the chosen pair (asserted on the engine through the
    ciphertext that stops there: the operand reached the tail); the second step and the tails work on it."""
    o, c = base._pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3912)
    bad = []
    for what, bsk, steered in _steered_op_sets(o, rng):
        _install(o, c, bsk, wc.extreme_ksk(o, "uniform", rng))
        b, got = _run_and_compare(o, c, _as_cases(o, steered), what)
        bad += b
        for i, (name, _, _, _, want) in enumerate(steered):
            if not np.array_equal(got[len(steered) + i][0], want):
                bad.append("%s | %s: the engine's accumulator after the first step is not the target" % (what, name))
    _finish(o, c, bad)


# ---- GPU: the same descriptors in one saturated launch (fused tail) ------------------------------------------------------------
def _saturated(o, c, cases, replicas, what, small_is_separate):
    nb = len(cases)
    descs = _load(c, cases, extra=2 * replicas)
    t0 = c.timing()["fused_tail_launches"]
    small = _engine_stages(c, descs, 2 * nb)
    t1 = c.timing()["fused_tail_launches"]
    if small_is_separate:
        assert t1 == t0, "the small launch was expected to run the separate tail kernels"
    big = [descs[i % nb][:3] + (4 * nb + 2 * i,) + descs[i % nb][4:] for i in range(replicas)]      # a pair writes out, out + 1
    got = _engine_stages(c, big, 4 * nb)
    assert c.timing()["fused_tail_launches"] == t1 + 1, "the saturated launch did not run the tail in its epilogue"
    bad = []
    for i in range(replicas):
        d = _first_difference(got[i], small[i % nb])
        if d:
            bad.append("%s | replica %d of %s | %s differs from the small launch" % (what, i, cases[i % nb][0], d[0]))
    for i, case in enumerate(cases):
        d = _first_difference(small[i], _reference(o, case))
        if d:
            bad.append("%s | %s | %s: first difference at %d: small launch %d, reference %d" % ((what, case[0]) + d))
    return bad


def _large_qks_rows():
    rows = []
    for log_qks in (26, 29):
        rows.append(Row("split", "qKS_2^%d" % log_qks, wc.GINX, lambda L, b, o, lg=log_qks: base._split_params(L, qKS=1 << lg), {}, 300))
        rows.append(Row("fp64", "N2048_base14_16waves_qKS_2^%d" % log_qks, wc.AP,
                        lambda L, b, o, lg=log_qks: base._custom(16, 2048, 1024, base._prime_below(L, 1 << 39, 2048), 1 << 14, qKS=1 << lg),
                        {"BCE_VARIANT": "3"}, 300, {"forward_transforms_per_step": 4}))
    return rows


LARGE_QKS = _large_qks_rows()
SATURATED_PARAMS = FUSED_PARAMS + [pytest.param(r, id=r.id) for r in LARGE_QKS]


@gpu
@pytest.mark.parametrize("row", SATURATED_PARAMS)
def test_xor_and_pair_saturated_launch(bce, orc, monkeypatch, row):
    """family `saturated`: the descriptors of the two tests above in one launch of row.fused bootstraps: fused_tail_launches
    goes up by one, every replica equals the small launch, the small launch the reference, at every stage.  Edge cases under
    uniform+forced / qKS-1 and Q-1 / uniform; the steered sets with both second-step keys for target_polys and the uniform
    one for the boundary sets.  The rows with qKS = 2^26 and 2^29 run the steered boundary sets only."""
    o, c = base._pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3913)
    separate = row.cls.startswith("split") and row.env.get("BCE_VARIANT") != "3"
    large = row in LARGE_QKS
    bad = []
    if not large:
        cases = wc.two_operand_cases(o)
        for bpat, kpat in (("uniform+forced", "qKS-1"), ("Q-1", "uniform")):
            _install(o, c, wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng))
            bad += _saturated(o, c, cases, row.fused, "bsk %s, ksk %s" % (bpat, kpat), separate)
    for k, (what, bsk, steered) in enumerate(_steered_op_sets(o, rng, polys=not large, boundary_seconds=("uniform",))):
        _install(o, c, bsk, wc.extreme_ksk(o, wc.KSK_PATTERNS[k % 3], rng))
        bad += _saturated(o, c, _as_cases(o, steered), row.fused, what, separate)
    _finish(o, c, bad)


# ---- GPU: the persistent kernel under crafted keys -----------------------------------------------------------------------------
DAG_ROWS = [(r, 1) for r in ROWS if r.selector == "default" and r.cls in ("split", "split_lazy_edge")]
DAG_ROWS += [(r, 1) for r in ROWS if (r.cls, r.selector, r.method) == ("fp64", "N2048_base14_16waves", wc.AP)]
DAG_ROWS += [(r, 0) for r in ROWS if r.selector in ("N2048_base14_16waves_separate_tail", "N2048_base14_8waves") and r.cls == "fp64" and r.method == wc.AP]


@gpu
@pytest.mark.parametrize("row,supported", [pytest.param(r, s, id=r.id) for r, s in DAG_ROWS])
def test_dataflow_kernel_under_extreme_keys(bce, orc, monkeypatch, row, supported):
    """family `dataflow`: every two-operand edge descriptor (plain gates, BCE_XOR and pairs mixed, inputs only, distinct
    outputs) as ONE run of the persistent kernel with two instances, under keys of all Q - 1 / qKS - 1 and uniform with forced
    ends: every output pool row of both instances -- out and out + 1 of pairs -- is the row the step path wrote for the same
    descriptor (which test_xor_and_pair_edges_under_extreme_keys holds to the reference).  Rows without the persistent kernel
    only assert that dag_supported() says so."""
    o, c = base._pair(bce, orc, row, monkeypatch)
    assert int(c.dag_supported()) == supported, "dag_supported() = %d on %s" % (c.dag_supported(), row.id)
    bad = []
    if supported:
        rng = np.random.default_rng(3914)
        cases = wc.two_operand_cases(o)
        nb, K = len(cases), 2
        stride = 4 * nb
        outs = np.array([b * stride + 2 * nb + j for b in range(2 * K) for j in range(2 * nb)], dtype=np.uint32).reshape(2, K * 2 * nb)
        written = np.array([[1, int(wc.is_pair(x[1]))] for x in cases], dtype=bool).reshape(-1)
        for bpat, kpat in (("Q-1", "qKS-1"), ("uniform+forced", "uniform")):
            _install(o, c, wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng))
            descs = _load(c, cases, copies=2 * K)
            c.lwe_write(outs.reshape(-1), np.zeros((outs.size, o.n + 1), dtype=np.uint64))
            c.EvalGates(descs, instances=K, slot_stride=stride)                                   # blocks 0, 1: the step path
            dag = c.dag_create(descs, pairs=True)
            c.dag_run(dag, instances=K, slot_stride=stride, slot_base=K * stride)                 # blocks 2, 3
            c.synchronize()
            last = c.dag_last_run()
            assert last["done"] == K * nb and last["abort"] == 0, last
            stepped, flowed = c.lwe_read(outs[0]), c.lwe_read(outs[1])
            c.dag_destroy(dag)
            for k in range(K):
                for j in np.flatnonzero(written):
                    g, w = flowed[k * 2 * nb + j], stepped[k * 2 * nb + j]
                    if not np.array_equal(g, w):
                        bad.append("bsk %s, ksk %s | %s | pool row of output %d, instance %d: first difference at %d"
                                   % (bpat, kpat, cases[j // 2][0], j % 2, k, int(np.flatnonzero(g != w)[0])))
                assert stepped[k * 2 * nb:(k + 1) * 2 * nb][written].any(), "the step path wrote nothing"
            assert np.array_equal(stepped[:2 * nb], stepped[2 * nb:]), "the step path's instances differ"
    _finish(o, c, bad)


# ---- CPU: the operands are what they claim to be (oracle and models alone) -------------------------------------------------------
ANCHOR_KEYS = (("Q-1", "qKS-1"), ("uniform+forced", "uniform"))


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_model_blind_rotation_equals_the_oracles_under_crafted_keys(orc, row):
    """the reference of BCE_XOR is anchored where it is used: after import_keys_eval of the all-Q - 1 and the uniform-with-
    forced-ends keys the numpy blind rotation with a plain gate's polynomial is bo_blind_rotate word for word, on prepared edge
    ciphertexts of the row (every a pattern, gates in turn; the plain gates' window-edge cases), at the row's modulus"""
    o = base._oracle(orc, row)
    q, n = o.params["q"], o.n
    rng = np.random.default_rng(3915)
    preps = [(wc.PLAIN[(k // 2) % 4], np.array(list(a) + [wc.b_patterns(q, wc.PLAIN[(k // 2) % 4])[(k + 2) % 6]], dtype=np.uint64))
             for k, (_, a, _) in enumerate(wc.a_patterns(o))]
    preps += [(x[1], x[6]) for x in wc.two_operand_cases(o) if x[1] in wc.PLAIN][::3]
    assert len(preps) >= 15 and set(g for g, _ in preps) == set(wc.PLAIN)
    for k, (bpat, kpat) in enumerate(ANCHOR_KEYS):
        _install(o, None, wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng))
        for gate, prep in preps[k::2]:             # half of the ciphertexts per key
            m = xm.plain_poly(o.params, gate, int(prep[n]))
            assert np.array_equal(m, wc.test_vector(o, gate, int(prep[n])))
            assert np.array_equal(xm.blind_rotate(o, m, prep), o.blind_rotate(gate, prep)), (bpat, wc.GATE_NAMES[gate], prep)
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_two_operand_cases_are_what_they_claim(orc, row):
    """every case prepares to its claimed word vector through the oracle's EvalNOT and gate_prep (BCE_XOR: AND's sum); both
    operands are non-trivial; the counts the coverage claim rests on.  ct2 is the fixed cycle, whose one zero in eight words
    stays (the preparation's own edge): every other word of it is non-zero.  A prepared word q - 1 has no pair of reduced
    operands whose sum wraps, so the share of wrapping sums is asserted over the cases of a row: at least a third, and
    at least one in every case whose prepared words are not all q - 1."""
    o = base._oracle(orc, row)
    q, n = o.params["q"], o.n
    cases = wc.two_operand_cases(o)
    names = [x[0] for x in cases]
    assert len(set(names)) == len(names)
    pats = wc.a_patterns(o)
    n_pat = len(pats)
    assert n_pat == (14 if o.params["method"] == wc.AP else 10)
    xor = [x for x in cases if x[1] == wc.XOR]
    pairs = [x for x in cases if wc.is_pair(x[1])]
    plain = [x for x in cases if x[1] in wc.PLAIN]
    assert len(xor) + len(pairs) + len(plain) == len(cases)
    wraps = 0
    ct2_fixed = wc.second_operand(q, n)
    assert int(ct2_fixed[n]) >= q // 2 and set(int(v) for v in ct2_fixed) == {0, 1, q // 4, q // 2 - 1, q // 2, q // 2 + 1, 3 * q // 4, q - 1}
    for name, op, ct1, ct2, n0, n1, prep in cases:
        assert int(ct1.max()) < q and int(ct2.max()) < q and int(prep.max()) < q, name
        a, b = (o.eval_not(ct1) if n0 else ct1), (o.eval_not(ct2) if n1 else ct2)
        assert np.array_equal(o.gate_prep(wc.AND if op == wc.XOR else op & 0xFF, a, b), prep), name
        assert np.array_equal(wc.lwe_not(q, ct1), o.eval_not(ct1))
        assert np.array_equal(ct2, ct2_fixed) and np.count_nonzero(ct2) == n + 1 - (n + 1) // 8, name
        assert np.count_nonzero(ct1) >= (n + 1) // 2, name
        w = wc.wrapped_sums(q, ct1, ct2, n0, n1)
        assert w == int(((a + b) >= q).sum())
        assert w >= 1 or (prep == q - 1).all() or (prep[:n] == q - 1).all(), name
        wraps += w
    assert 3 * wraps >= len(cases) * (n + 1), "only %d of %d sums wrap" % (wraps, len(cases) * (n + 1))
    print("%s: %d cases (%d XOR, %d pair, %d plain), %d of %d sums wrap" % (row.id, len(cases), len(xor), len(pairs), len(plain), wraps, len(cases) * (n + 1)))
    for group in (xor, pairs, plain, wc.operand_subset(cases)):
        assert set((x[4], x[5]) for x in group) == set(wc.NEGATIONS)
    # BCE_XOR: every a pattern, all ten b values, all ten under a=cycle
    assert len(xor) == 2 * n_pat + 10
    ten = set(wc.xor_b_values(q))
    e = q // 8
    assert ten == {0, q - 1, e - 1, e, 3 * e - 1, 3 * e, 5 * e - 1, 5 * e, 7 * e - 1, 7 * e} and len(ten) == 10
    for pname, a, _ in pats:
        assert sum(1 for x in xor if list(x[6][:n]) == list(a)) >= 2, pname
    cyc = dict((nm, a) for nm, a, _ in pats)["a=cycle"]
    assert [int(x[6][n]) for x in xor[2 * n_pat:]] == wc.xor_b_values(q)
    assert all(list(x[6][:n]) == list(cyc) and x[0].startswith(wc.SWEEP) for x in xor[2 * n_pat:])
    sub = wc.operand_subset(xor)                      # every a pattern once, and still all ten b values
    assert len(sub) == n_pat and [list(x[6][:n]) for x in sub] == [list(a) for _, a, _ in pats]
    assert set(int(x[6][n]) for x in sub) == ten
    # pairs: all 12 ordered pairs, on every window edge of both gates under a=cycle, and once with a = 0
    assert wc.ORDERED_PAIRS == pm.ORDERED_PAIRS and [wc.pair_word(*p) for p in wc.ORDERED_PAIRS] == [pm.PAIR(*p) for p in pm.ORDERED_PAIRS]
    assert set(x[1] for x in pairs) == set(PAIR_WORDS) and len(PAIR_WORDS) == 12
    total = 0
    for op, op2 in wc.ORDERED_PAIRS:
        mine = [x for x in pairs if x[1] == wc.pair_word(op, op2)]
        edges = set(wc.gate_window(q, op) + wc.gate_window(q, op2))
        assert len(edges) == (2 if (op - op2) % 4 == 2 else 4)           # a gate and its complement share their edges
        assert set(int(x[6][n]) for x in mine if list(x[6][:n]) == list(cyc)) == edges
        zero = [x for x in mine if not x[6][:n].any()]
        assert len(zero) == 1 and (int(zero[0][6][n]) + 1) % q in edges and wc.executed_steps(o, zero[0][6]) == 0
        assert len(mine) == len(edges) + 1
        total += len(mine)
    assert total == len(pairs) == 4 * 3 + 8 * 5
    assert len(wc.operand_subset(pairs)) == 24
    # plain gates: every gate under every negation combination, b on a window edge or next to it
    assert len(plain) == 16
    for gate in wc.PLAIN:
        assert set((x[4], x[5]) for x in plain if x[1] == gate) == set(wc.NEGATIONS)
        assert all(int(x[6][n]) in wc.b_patterns(q, gate)[2:] for x in plain if x[1] == gate)
    assert len(cases) == 2 * n_pat + 10 + 52 + 16
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_xor_window_boundaries_move_exactly_the_coefficients_they_should(orc, row):
    """for b on each of the four boundaries k q/8 (k = 1, 3, 5, 7), xor_poly(b) and xor_poly(b - 1) differ in exactly the
    coefficients j (2N/q), j < q/2, at which t = b - j is on a boundary: there the level moves between 0 and +-2(Q/8 + 1) as
    the definition says; and the model's accumulators of the two b differ (under a uniform key with forced ends)."""
    o = base._oracle(orc, row)
    p = o.params
    q, Q, N, n = p["q"], p["Q"], o.N, o.n
    f, e, one = 2 * N // q, q // 8, 2 * (Q // 8 + 1) % Q
    rng = np.random.default_rng(3916)
    _install(o, None, wc.extreme_bsk(o, "uniform+forced", rng), wc.extreme_ksk(o, "0", rng))

    def level(t):
        return one if e <= t < 3 * e else Q - one if 5 * e <= t < 7 * e else 0

    cyc = dict((nm, a) for nm, a, _ in wc.a_patterns(o))["a=cycle"]
    for k in (1, 3, 5, 7):
        b = k * e
        m, m1 = xm.xor_poly(p, b), xm.xor_poly(p, b - 1)
        assert set(int(v) for v in m) <= {0, one, Q - one} and not np.delete(m, np.arange(0, N, f)).any()
        js = sorted(j for j in range(q // 2) if (b - j) % q in (e, 3 * e, 5 * e, 7 * e))
        assert len(js) == 2                                   # the four boundaries are q/4 apart, j runs over half of Z_q
        assert list(np.flatnonzero(m != m1)) == [j * f for j in js], (k, js)
        for j in js:
            assert int(m[j * f]) == level((b - j) % q) and int(m1[j * f]) == level((b - 1 - j) % q) and int(m[j * f]) != int(m1[j * f])
        accs = [xm.blind_rotate(o, xm.xor_poly(p, bb), np.array(list(cyc) + [bb], dtype=np.uint64)) for bb in (b, b - 1)]
        assert not np.array_equal(accs[0], accs[1]), k
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_steered_xor_and_pair_targets_are_reached(orc, row):
    """every target is reached (a failed solve raises): the model's (BCE_XOR) and the oracle's (pairs) accumulator after the
    first step equals the target; the boundary set of the offset-free tail gives different b' on the two sides of each boundary
    (through the oracle's tail, after the model's own -(Q/8 + 1)); rotating a pair's boundary target by its exponent gives A2,
    which holds 0 and Q - 1 at the wrap index, next to it and at two negated positions; all three exponents occur."""
    o = base._oracle(orc, row)
    Q, N, n = o.params["Q"], o.N, o.n
    rng = np.random.default_rng(3912)
    reached = {"XOR": 0, "pair": 0}
    for what, bsk, steered in _steered_op_sets(o, rng, seconds=("uniform",), boundary_seconds=("uniform",)):     # (step one alone is checked)
        assert bsk.dtype == np.uint64 and int(bsk.max()) < Q
        _install(o, None, bsk, wc.extreme_ksk(o, "0", rng))
        for name, op, prep, first, want in steered:
            assert wc.executed_steps(o, first) == 1 and wc.executed_steps(o, prep) == 2, name
            if op == wc.XOR:
                acc = xm.blind_rotate(o, xm.xor_poly(o.params, int(first[n])), first)
            else:
                assert wc.is_pair(op)
                acc = o.blind_rotate(op & 0xFF, first)
            assert np.array_equal(acc, want), "%s | %s: accumulator after step one is not the target" % (what, name)
            reached["XOR" if op == wc.XOR else "pair"] += 1
    n_poly = len(wc.target_polys(o, rng))
    assert n_poly == 8 and reached == {"XOR": n_poly + 9, "pair": n_poly + 10}, reached
    # the offset-free tail's boundaries
    accs = base._tail_accumulators(o, rng, off=0)
    assert [int(a[1, 0]) for a in accs[:3]] == [0, 1, Q - 1] and len(accs) == 9
    shift = Q - (Q // 8 + 1)
    bprime = []
    for a in accs:
        s = a.reshape(-1).copy()
        s[N] = (int(s[N]) + shift) % Q
        bprime.append(int(o.extract_modswitch(s)[N]))
    qks = o.params["qKS"]
    for lo in (3, 5, 7):
        assert int(accs[lo + 1][1, 0]) == int(accs[lo][1, 0]) + 1 and bprime[lo + 1] == (bprime[lo] + 1) % qks, (lo, bprime)
    assert bprime[8] == 0 and bprime[7] == qks - 1            # the result qKS that wraps to 0
    # the rotated targets of the pairs' second tail
    targets, words, A2s = _pair_boundary_targets(o, rng)
    plainA = base._tail_accumulators(o, np.random.default_rng(1))
    assert len(targets) == len(plainA) == 10
    exps = set()
    for (name, _, t), w, A2 in zip(targets, words, A2s):
        op, op2 = w & 0xFF, (w >> 8) - 1
        e = pm.exponent(o.params, op, op2)
        exps.add(e)
        for j in range(2):
            assert np.array_equal(pm.rotate(t[j], e, Q), A2[j]), name
        assert int(A2[0, e % N]) == 0 and int(A2[0, (e - 1) % N]) == Q - 1
        lo, hi = (0, e % N) if e < N else (e % N, N)
        mid = (lo + hi) // 2
        assert lo <= mid < mid + 1 < hi and int(A2[0, mid]) == 0 and int(A2[0, mid + 1]) == Q - 1
        # negated positions: the target's source words are 0 (stays 0) and 1 (-1 = Q - 1)
        src = lambda i: (i - e) % N
        assert int(t[0][src(mid)]) == 0 and int(t[0][src(mid + 1)]) == 1
        assert int(t[0][0]) == 0 and int(t[0][N - 1]) in (1, Q - 1)
    assert exps == {N // 2, N, 3 * N // 2}
    o.close()
