"""The oracle alone: two gates from one blind rotation (tests/pair_model.py).  Pins the helper the GPU tests of pair
descriptors lean on: the tail applied to X^e * acc decrypts to the second gate's truth table, and XOR spelled
AND(OR, NAND) over a shared rotation equals a ^ b."""
import numpy as np
import pytest

import pair_model as pm

SEED = 0x0FE5EED


@pytest.fixture(scope="module", params=["GINX", "AP"])
def toy(orc, request):
    o = orc.Oracle(orc.TOY, getattr(orc, request.param))
    o.keygen(SEED)
    return o


def test_rotate_is_the_negacyclic_monomial_product():
    Q, N = 97, 8
    p = np.arange(1, N + 1, dtype=np.uint64)
    x = p.copy()
    for e in range(1, 2 * N + 1):               # multiply by X once more each round
        x = np.concatenate([[(Q - x[-1]) % Q], x[:-1]]).astype(np.uint64)
        assert np.array_equal(pm.rotate(p, e % (2 * N), Q), x), e


def test_every_ordered_pair_decrypts_to_both_truth_tables(toy):
    o = toy
    idx = 0
    for op, op2 in pm.ORDERED_PAIRS:
        for a in (0, 1):
            for b in (0, 1):
                ca, cb = o.encrypt(a, idx), o.encrypt(b, idx + 1)
                idx += 2
                r = pm.stages(o, op, op2, ca, cb)
                assert np.array_equal(r["out"][0], o.eval_bingate(op, ca, cb))
                assert o.decrypt(r["out"][0]) == pm.truth(op, a, b)
                assert o.decrypt(r["out"][1]) == pm.truth(op2, a, b), (op, op2, a, b)


def test_folded_nots_apply_to_both_outputs(toy):
    o = toy
    for k, (a, b, n0, n1) in enumerate([(0, 1, 1, 0), (1, 1, 0, 1), (1, 0, 1, 1)]):
        ca, cb = o.encrypt(a, 500 + 2 * k), o.encrypt(b, 501 + 2 * k)
        r = pm.stages(o, pm.NOR, pm.AND, ca, cb, n0, n1)
        assert o.decrypt(r["out"][0]) == pm.truth(pm.NOR, a ^ n0, b ^ n1)
        assert o.decrypt(r["out"][1]) == pm.truth(pm.AND, a ^ n0, b ^ n1)


def test_64_xors_through_the_shared_spelling(toy):
    o = toy
    rng = np.random.default_rng(5)
    for k in range(64):
        a, b = (int(v) for v in rng.integers(0, 2, 2))
        ca, cb = o.encrypt(a, 1000 + 2 * k), o.encrypt(b, 1001 + 2 * k)
        assert o.decrypt(pm.xor_shared(o, ca, cb)) == a ^ b, k
