"""The reference of BCE_XOR (tests/xor_single_model.py) on the CPU: its restated blind rotation is the oracle's, word for word,
on the plain gates' test polynomial (TOY GINX / AP and the `split` shape of noise_run.shapes); with the three-level polynomial
every input pair and every combination of folded NOTs decrypts to XOR, with the phase error of the output below q/16 (half the
margin a consumer has)."""
import numpy as np
import pytest

import noise_run
import pair_model as pm
import xor_single_model as xm

SEED = 0x0FE5EED
SHAPES = [("TOY", "GINX"), ("TOY", "AP"), ("split", "GINX"), ("split", "AP")]


@pytest.fixture(scope="module")
def oracles(orc):
    table = noise_run.shapes(orc.lib(), None)
    made = {}

    def get(shape, method):
        if (shape, method) not in made:
            custom = table[shape][1] if shape in table else None
            o = orc.Oracle(method=getattr(orc, method), custom=custom) if custom else orc.Oracle(getattr(orc, shape), getattr(orc, method))
            o.keygen(SEED)
            made[(shape, method)] = o
        return made[(shape, method)]

    return get


@pytest.mark.parametrize("shape,method", SHAPES)
def test_restated_blind_rotation_is_the_oracles(oracles, shape, method):
    o = oracles(shape, method)
    for k, op in enumerate(pm.GATES):
        a, b = k & 1, k >> 1
        ca, cb = o.encrypt(a, 40 + 2 * k), o.eval_not(o.encrypt(1 - b, 41 + 2 * k))
        prep = o.gate_prep(op, ca, cb)
        got = xm.blind_rotate(o, xm.plain_poly(o.params, op, int(prep[o.n])), prep)
        assert np.array_equal(got, o.blind_rotate(op, prep)), (shape, method, op)


def test_the_polynomial_is_negacyclic_with_three_levels():
    """f(t + q/2) = -f(t): coefficient j + q/2 of the full-period function is minus coefficient j, for every b"""
    params = {"q": 512, "Q": (1 << 27) - 39, "N": 512}
    Q, one = params["Q"], 2 * (params["Q"] // 8 + 1)
    for b in (0, 1, 63, 64, 65, 200, 256, 448, 511):
        m = xm.xor_poly(params, b)
        assert set(int(v) for v in m[::2]) <= {0, one, Q - one} and not m[1::2].any()
        flip = xm.xor_poly(params, (b + 256) % 512)
        assert np.array_equal((m + flip) % np.uint64(Q), np.zeros_like(m))
        assert int((m[::2] == one).sum()) + int((m[::2] == Q - one).sum()) == 128    # a quarter of the period each, half of them seen


@pytest.mark.parametrize("shape,method", SHAPES)
def test_every_input_and_negation_decrypts_to_xor(oracles, shape, method):
    o = oracles(shape, method)
    q = o.params["q"]
    idx = 500
    for a in (0, 1):
        for b in (0, 1):
            for n0 in (0, 1):
                for n1 in (0, 1):
                    ca, cb = o.encrypt(a, idx), o.encrypt(b, idx + 1)
                    idx += 2
                    out = xm.stages(o, ca, cb, n0, n1)["out"]
                    want = (a ^ n0) ^ (b ^ n1)
                    assert o.decrypt(out) == want, (shape, method, a, b, n0, n1)
                    assert abs(o.noise(out, want)) < q // 16, (shape, method, a, b, n0, n1, o.noise(out, want))


def test_eval_desc_falls_through_to_the_pair_model(oracles):
    o = oracles("TOY", "GINX")
    ca, cb = o.encrypt(1, 900), o.encrypt(0, 901)
    pool = {0: ca, 1: cb}
    xm.eval_desc(o, pool, (xm.XOR, 0, 1, 2, 0, 1))
    xm.eval_desc(o, pool, (pm.AND, 0, 1, 3))
    xm.eval_desc(o, pool, (pm.PAIR(pm.OR, pm.NAND), 0, 1, 4))
    xm.eval_desc(o, pool, (xm.OP_REFRESH, 0, 0, 6))
    assert np.array_equal(pool[2], xm.stages(o, ca, cb, 0, 1)["out"]) and o.decrypt(pool[2]) == 0
    assert np.array_equal(pool[3], o.eval_bingate(pm.AND, ca, cb))
    assert [o.decrypt(pool[s]) for s in (4, 5, 6)] == [1, 1, 1]
