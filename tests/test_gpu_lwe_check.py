"""k_lwe_check against the CPU oracle: the device-side decrypt / compare / repair of verify mode (bce_check_slots), which
restates bo_decrypt / bo_noise of oracle/binfhe_oracle.c (the reference: src/gate.cpp:153-160).  Same-seed keys on both
sides.  Shapes = the smallest at which the per-lane loop and the wave reduction can go wrong:

    custom, n = 63 (TOY's other parameters)   64 row words   exactly one pass of the 64 lanes
    TOY, n = 64                                65 row words   b alone in the second pass
    STD128_OPT, n = 502, q = 1024             503 row words   ragged last pass

All comparisons are exact (integers): report and log must equal what Oracle.decrypt / Oracle.noise give per ciphertext."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED
STRIDE, K = 16, 3                 # slots per instance, instances laid out
ORDER = [2, 0, 3, 1, 4]           # check order: AND output, FRESH, OR output, BOOTSTRAPPED, NAND output


def _pair(bce, orc, name):
    if name == "n63":
        t = orc.Oracle(orc.TOY, orc.GINX)
        p = t.params
        t.close()
        custom = (63, p["N"], p["q"], p["Q"], p["qKS"], p["baseKS"], p["baseG"], p["baseR"])
        o, c = orc.Oracle(method=orc.GINX, custom=custom), bce.BinFHEContext(method=bce.GINX, custom=custom)
    else:
        ps = {"toy": "TOY", "std128": "STD128_OPT"}[name]
        o, c = orc.Oracle(getattr(orc, ps), orc.GINX), bce.BinFHEContext(getattr(bce, ps), bce.GINX)
    assert o.params == c.params
    o.keygen(SEED)
    if name == "toy":
        c.import_keys(o.sk(), o.z(), o.bsk(), o.ksk())      # the import path uploads the secret too
    else:
        c.KeyGen(SEED)                                       # engine keygen == oracle keygen for the same seed
        assert np.array_equal(c.export_sk()[0], o.sk())
    return o, c


@pytest.fixture(scope="module")
def ctxs(bce, orc):
    """per context: K instances of {0: FRESH, 1: BOOTSTRAPPED, 2: AND, 3: OR, 4: NAND of slots 5, 6}, read back once"""
    made = {}
    for name in ("n63", "toy", "std128"):
        o, c = _pair(bce, orc, name)
        assert c.n == {"n63": 63, "toy": 64, "std128": 502}[name]
        c.pool_reserve(K * STRIDE + 600)
        rng = np.random.default_rng(len(made) + 5)
        bits = rng.integers(0, 2, (K, 4))
        idx = 1000
        for k in range(K):
            fresh = [o.encrypt(int(b), idx + i) for i, b in enumerate(bits[k])]
            idx += 4
            rows = [fresh[0], o.bootstrap(fresh[1]), fresh[2], fresh[3]]
            c.lwe_write(np.array([0, 1, 5, 6], dtype=np.uint32) + k * STRIDE, np.stack(rows))
        c.EvalGates([(bce.AND, 5, 6, 2), (bce.OR, 5, 6, 3), (bce.NAND, 5, 6, 4)], instances=K, slot_stride=STRIDE)
        cts = c.lwe_read(np.arange(K * STRIDE, dtype=np.uint32))
        truth = np.zeros((K, 5), dtype=np.uint8)
        for k in range(K):
            a, b = int(bits[k][2]), int(bits[k][3])
            truth[k] = [bits[k][0], bits[k][1], a & b, a | b, 1 - (a & b)]
            for s in range(5):
                assert o.decrypt(cts[k * STRIDE + s]) == truth[k][s], (name, k, s)
        made[name] = (o, c, cts, truth)
    yield made
    for o, c, _, _ in made.values():
        o.close()
        c.close()


def _want(o, cts, expect):
    """what the oracle says about checking ciphertext i against expect[i]: (report counters, set of log tuples sans tag)"""
    got = [o.decrypt(ct) for ct in cts]
    err = [o.noise(ct, int(e)) for ct, e in zip(cts, expect)]
    rep = {"checked": len(cts), "mismatches": sum(int(g != e) for g, e in zip(got, expect)),
           "max_abs_err": max(abs(e) for e in err), "sum_err": sum(err), "sum_sq_err": sum(e * e for e in err)}
    return rep, got, err


def _run(c, slots, expect, instances=1, stride=0, repair=False, tag=0):
    c.check_reset()
    c.check_slots(slots, expect, instances, stride, repair, tag)
    return c.check_get()


def _same(rep, want):
    return {k: rep[k] for k in want} == want


def test_every_rounding_boundary_of_the_decision(bce, orc, ctxs):
    """all q = 512 trivial ciphertexts (0, b) at TOY: independent of the key; against expect = 0 .. 3 every ciphertext is
    a mismatch three times and its (got, err) is logged; against the oracle's own decryption nothing is, and one check
    per ciphertext returns err itself"""
    o, c, _, _ = ctxs["toy"]
    q = c.params["q"]
    assert q == 512
    base = K * STRIDE
    slots = np.arange(base, base + q, dtype=np.uint32)
    cts = np.zeros((q, c.n + 1), dtype=np.uint64)
    cts[:, c.n] = np.arange(q)
    c.lwe_write(slots, cts)
    for e in range(4):
        expect = np.full(q, e, dtype=np.uint8)
        want, got, err = _want(o, cts, expect)
        rep, log = _run(c, slots, expect, tag=70 + e)
        assert _same(rep, want), (e, rep, want)
        assert rep["repaired"] == 0 and rep["log_count"] == want["mismatches"] == 3 * q // 4
        assert {(x["tag"], x["index"], x["instance"], x["slot"], x["got"], x["expect"], x["err"]) for x in log} == \
               {(70 + e, b, 0, base + b, got[b], e, err[b]) for b in range(q) if got[b] != e}
    expect = np.array([o.decrypt(ct) for ct in cts], dtype=np.uint8)
    want, _, err = _want(o, cts, expect)
    rep, log = _run(c, slots, expect)
    assert _same(rep, want) and rep["mismatches"] == 0 and log == [] and rep["margin"] == q // 8 - want["max_abs_err"]
    assert want["max_abs_err"] == q // 8                   # (q/8 itself rounds up: err = -q/8 for the next message)
    for b in range(q):                                     # one check per ciphertext: err word for word
        rep, log = _run(c, slots[b:b + 1], expect[b:b + 1])
        assert (rep["sum_err"], rep["max_abs_err"], rep["sum_sq_err"], rep["checked"]) == (err[b], abs(err[b]), err[b] ** 2, 1), b
    assert np.array_equal(c.lwe_read(slots), cts)


@pytest.mark.parametrize("instances", [1, 3])
@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("name", ["n63", "toy", "std128"])
def test_real_ciphertexts_report_log_and_repair(bce, orc, ctxs, name, count, instances):
    o, c, cts, truth = ctxs[name]
    q = c.params["q"]
    slots = np.array(ORDER[:count], dtype=np.uint32)
    all_slots = np.arange(K * STRIDE, dtype=np.uint32)
    rows = [cts[k * STRIDE + s] for k in range(instances) for s in slots]
    right = np.array([truth[k][s] for k in range(instances) for s in slots], dtype=np.uint8)
    # correct expectations: nothing logged, the noise statistics are the oracle's
    want, _, _ = _want(o, rows, right)
    rep, log = _run(c, slots, right, instances, STRIDE)
    assert _same(rep, want) and rep["mismatches"] == 0 and rep["repaired"] == 0 and log == []
    assert rep["margin"] > 0 and abs(rep["noise_rms"] ** 2 * rep["checked"] - want["sum_sq_err"]) < 1e-6 * max(1, want["sum_sq_err"])
    # a chosen subset of wrong expectations
    wrong = right.copy()
    subset = [i for i in range(len(wrong)) if (i // count + i % count) % 2 == 0]
    assert subset
    for i in subset:
        wrong[i] = 1 - wrong[i]
    want, got, err = _want(o, rows, wrong)
    assert want["mismatches"] == len(subset)
    expect_log = {(9, i % count, i // count, int(slots[i % count]) + (i // count) * STRIDE, got[i], int(wrong[i]), err[i]) for i in subset}
    rep, log = _run(c, slots, wrong, instances, STRIDE, repair=False, tag=9)
    assert _same(rep, want) and rep["repaired"] == 0
    assert {(x["tag"], x["index"], x["instance"], x["slot"], x["got"], x["expect"], x["err"]) for x in log} == expect_log
    assert np.array_equal(c.lwe_read(all_slots), cts), "repair = 0 changed the pool"
    try:
        rep, log = _run(c, slots, wrong, instances, STRIDE, repair=True, tag=9)
        assert _same(rep, want) and rep["repaired"] == len(subset)
        assert {(x["tag"], x["index"], x["instance"], x["slot"], x["got"], x["expect"], x["err"]) for x in log} == expect_log
        after = c.lwe_read(all_slots)
        fixed = cts.copy()
        for i in subset:
            row = np.zeros(c.n + 1, dtype=np.uint64)
            row[c.n] = int(wrong[i]) * (q // 4)
            fixed[int(slots[i % count]) + (i // count) * STRIDE] = row
        assert np.array_equal(after, fixed), "repair = 1: exactly the mismatching rows become (0, ..., 0, expect q/4)"
        rep, log = _run(c, slots, wrong, instances, STRIDE, repair=True)
        assert rep["mismatches"] == 0 and rep["repaired"] == 0 and log == []
        rslots = np.array([int(slots[i % count]) + (i // count) * STRIDE for i in subset], dtype=np.uint32)
        rep, _ = _run(c, rslots, wrong[subset])
        assert (rep["checked"], rep["mismatches"], rep["max_abs_err"], rep["sum_err"], rep["sum_sq_err"]) == (len(subset), 0, 0, 0, 0)
    finally:
        c.lwe_write(all_slots, cts)
    assert np.array_equal(c.lwe_read(all_slots), cts)


def test_counters_accumulate_until_reset(bce, orc, ctxs):
    o, c, cts, truth = ctxs["toy"]
    slots = np.arange(5, dtype=np.uint32)
    want, _, _ = _want(o, [cts[s] for s in slots], truth[0])
    c.check_reset()
    for _ in range(3):
        c.check_slots(slots, truth[0])
    rep, _ = c.check_get()
    assert rep["checked"] == 15 and rep["sum_sq_err"] == 3 * want["sum_sq_err"] and rep["sum_err"] == 3 * want["sum_err"]
    assert rep["max_abs_err"] == want["max_abs_err"]
    c.check_reset()
    assert c.check_get()[0]["checked"] == 0


def test_status_codes(bce, ctxs):
    _, c, _, _ = ctxs["toy"]
    n = c._L.bce_pool_slots(c.h)
    for slots, expect, inst, stride, code in (([n], [0], 1, 0, bce.ERR_POOL), ([n - 1], [0, 0], 2, 1, bce.ERR_POOL),
                                              ([0], [4], 1, 0, bce.ERR_ARG)):
        with pytest.raises(bce.BceError) as e:
            c.check_slots(slots, expect, inst, stride)
        assert e.value.code == code
    assert c._L.bce_check_slots(c.h, 1, None, None, 1, 0, 0, 0) == bce.ERR_ARG
    assert c._L.bce_check_get(c.h, None, None, 0) == bce.ERR_ARG
    bare = bce.BinFHEContext(bce.TOY, bce.GINX)
    bare.pool_reserve(4)
    with pytest.raises(bce.BceError) as e:
        bare.check_slots([0], [0])
    assert e.value.code == bce.ERR_NO_KEYS
    bare.close()
