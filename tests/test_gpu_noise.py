"""The size of the noise, on the device: keys from the device keygen, the engine's own Encrypt and every stage of a bootstrap
against the analytic model of tests/noise_model.py, at sample sizes only the GPU affords (65 536 bootstraps per shape, 262 144
on the headline set).  The parity tests pin the engine to the oracle bit for bit; these pin both to an independent statement
of how much noise the scheme leaves, on the paths that never meet the oracle (KeyGen(None), Encrypt without a seed).

Shapes (noise_run.shapes): each varies an INPUT OF THE MODEL -- gadget base and digit count, top-digit width, qKS = Q
against a power of two, baseKS 25 / 28 / 2^7, baseR 23 / 32 / 46, 2N/q = 1 or 2, both methods -- with small n, so that a
bootstrap costs n/502 of a real one.  Kernel selectors are pinned bit for bit elsewhere: no BCE_* variable is set here.

Bars: second moments within [0.90, 1.10] of the model (for the key at hand: noise_model.second_moment_for_key), |mean| <=
5 sqrt(V_bias + V/M), largest |error| <= 6.5 sigma, zero wrong bits; key and encryption errors: mean within 5 sigma / sqrt(count), second moment within 3 % of sigma^2, |e| <= 22."""
import math

import numpy as np
import pytest

import noise_model as nm
import noise_run

pytestmark = pytest.mark.gpu
SEED = 0x0FE5EED


def _shape_ids():
    # the ids are static; the moduli are looked up when a context is made
    return [("toy", "GINX"), ("toy", "AP"), ("split", "GINX"), ("split", "AP"), ("std256_like", "GINX"), ("std256_like", "AP"),
            ("std192_like", "AP"), ("std192_like", "GINX"), ("int64_40", "GINX")]


CASES = [pytest.param(s, m, id="%s-%s" % (s, m)) for s, m in _shape_ids()]


@pytest.fixture(scope="module")
def contexts(bce, orc):
    """one context per (shape, method), keys from OS entropy, made on first use and shared by the tests of this file"""
    table = noise_run.shapes(orc.lib(), bce.TOY)
    assert [(s, m) for s in table for m in table[s][2]] == _shape_ids()
    made = {}

    def get(shape, method):
        if (shape, method) not in made:
            paramset, custom, _ = table[shape]
            c = bce.BinFHEContext(paramset, getattr(bce, method)) if custom is None else bce.BinFHEContext(method=getattr(bce, method), custom=custom)
            c.KeyGen(None)
            made[(shape, method)] = c
        return made[(shape, method)]

    yield get
    for c in made.values():
        c.close()


def _in_band(ratio, what):
    assert nm.BAND[0] <= ratio <= nm.BAND[1], "%s: measured / model = %.3f outside [%.2f, %.2f]" % (what, ratio, nm.BAND[0], nm.BAND[1])


# ---- (a) keys --------------------------------------------------------------------------------------------------------------------
def _check_keys(c, what):
    p = c.params
    s, z = c.export_sk()
    nm.assert_ternary(s, what + " s")
    nm.assert_ternary(z, what + " z")
    ksk = c.export_ksk()
    nm.assert_key_errors(nm.ksk_errors(ksk, p, s, z), what + " key-switching key")
    nm.assert_uniform_buckets(ksk.reshape(-1, p["n"] + 1)[:, :-1], p["qKS"], what + " a-words of the key-switching key")
    # whole RGSW ciphertexts of every 4th (2nd, every) secret coefficient until 50 000 error coefficients enter; of the AP
    # key's many ciphertexts per coefficient an even subset of about 64
    per = 2 * p["dG"] * p["N"]
    for step in (4, 2, 1):
        ids = nm.rgsw_ids(p, s, step)
        if len(ids) * per >= 50000:
            break
    ids = ids[::max(1, len(ids) // 64)]
    assert len(ids) * per >= 50000
    bsk = c.export_bsk().reshape(-1, 2 * p["dG"], 2, p["N"])
    nm.assert_key_errors(nm.rgsw_errors(bsk, p, z, ids), what + " bootstrapping key")
    nm.assert_uniform_buckets(bsk[[i for i, _, _ in ids], :, 0, :], p["Q"], what + " a-words of the bootstrapping key")
    return s


@pytest.mark.parametrize("shape,method", CASES)
def test_keys_of_the_device_keygen_carry_sigma(contexts, shape, method):
    _check_keys(contexts(shape, method), "%s %s" % (shape, method))


def test_keygen_from_os_entropy_is_fresh_and_the_seeded_path_passes_the_same_bars(bce):
    c = bce.BinFHEContext(bce.TOY, bce.GINX)
    c.KeyGen(None)
    s1 = c.export_sk()[0].copy()
    c.KeyGen(None)
    assert not np.array_equal(s1, c.export_sk()[0]), "two KeyGen(None) calls gave the same secret"
    c.KeyGen(SEED)                  # the path pinned word for word to the oracle's keygen
    _check_keys(c, "toy GINX seeded")
    c.close()


# ---- (b) Encrypt -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["toy", "split"])
def test_encrypt_in_its_default_seed_state(contexts, shape):
    c = contexts(shape, "GINX")
    p = c.params
    s, z = c.export_sk()
    V = nm.model(p, s, z)
    M = 65536
    c.pool_reserve(M)
    slots = np.arange(M, dtype=np.uint32)
    bits = (np.arange(M) % 2).astype(np.uint8)
    c.Encrypt(bits, slots, mode=0)
    c.check_reset()
    c.check_slots(slots, bits)
    rep = c.check_get()[0]
    var, mean = rep["sum_sq_err"] / M, rep["sum_err"] / M
    print("%s FRESH: second moment %.3f (sigma^2 %.3f), mean %+.4f, max |e| %d" % (shape, var, nm.SIGMA2, mean, rep["max_abs_err"]))
    assert rep["checked"] == M and rep["mismatches"] == 0
    assert abs(var / nm.SIGMA2 - 1.0) <= 0.03
    assert abs(mean) <= 5 * nm.SIGMA / math.sqrt(M)
    back = c.lwe_read(slots[:4096])
    nm.assert_uniform_buckets(back[:, :-1], p["q"], shape + " a-words of fresh encryptions")
    assert int(np.abs(nm.lwe_phase_error(back, s, p["q"], bits[:4096])).max()) <= rep["max_abs_err"] <= 22   # host phases agree with the device's
    M2 = 16384
    for o in range(0, M2, 4096):    # BOOTSTRAPPED = encrypt + one refresh each, 4096 per launch
        c.Encrypt(bits[o:o + 4096], slots[o:o + 4096], mode=1)
    c.check_reset()
    c.check_slots(slots[:M2], bits[:M2])
    rep = c.check_get()[0]
    ratio, mean, bar, mx = nm.report_stats(rep, V["V_out"], V["B_out"])
    print("%s BOOTSTRAPPED: ratio %.3f, mean %+.3f (bar %.3f), max |e| %.2f sigma" % (shape, ratio, mean, bar, mx))
    assert rep["checked"] == M2 and rep["mismatches"] == 0
    _in_band(ratio, shape + " BOOTSTRAPPED")
    assert abs(mean) <= bar, (shape, mean, bar)


# ---- (c) stages --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,method", CASES)
def test_every_stage_fits_the_model(contexts, shape, method):
    c = contexts(shape, method)
    s, z = c.export_sk()
    V = nm.model(c.params, s, z)
    err, wrong = noise_run.stage_run(c, np.random.default_rng(21), total=8192, chunk=4096, n_in=1024)
    stats = {tag: nm.stage_stats(err[tag], V["V_" + tag], V["B_" + tag]) for tag in ("N", "ks", "out")}
    for tag, (ratio, raw, mean, bar, mx, m2) in stats.items():
        print("%s %s stage %-3s second moment %.2f, model %.2f, ratio %.3f (against V itself %.3f); mean %+.3f (bar %.3f); max |e| %.2f sigma" % (
            shape, method, tag, m2, V["V_" + tag], ratio, raw, mean, bar, mx))
    assert wrong == 0
    for tag, (ratio, raw, mean, bar, mx, m2) in stats.items():
        _in_band(ratio, "%s %s stage %s" % (shape, method, tag))
        assert abs(mean) <= bar, (tag, mean, bar)       # the final stage is what a caller sees; the earlier ones hold to the same bar


# ---- (d) end level -------------------------------------------------------------------------------------------------------------------
def _end_level_bars(reps, V, what):
    stats = [nm.report_stats(r, V["V_out"], V["B_out"]) for r in reps]
    for lvl, (r, (ratio, mean, bar, mx)) in enumerate(zip(reps, stats), 1):
        print("%s level %d: M %d, rms %.3f (model %.3f), ratio %.3f, mean %+.3f (bar %.3f), max |e| %d = %.2f sigma, margin %d" % (
            what, lvl, r["checked"], r["noise_rms"], math.sqrt(V["V_out"]), ratio, mean, bar, r["max_abs_err"], mx, r["margin"]))
    for lvl, (r, (ratio, mean, bar, mx)) in enumerate(zip(reps, stats), 1):
        assert r["mismatches"] == 0, (what, lvl, r)
        _in_band(ratio, "%s level %d" % (what, lvl))
        assert abs(mean) <= bar, (what, lvl, mean, bar)
        assert mx <= nm.MAX_SIGMAS, (what, lvl, mx)
    # a bootstrap's output noise does not depend on its inputs' noise: the two second moments agree
    m2 = [r["sum_sq_err"] / r["checked"] for r in reps]
    assert abs(m2[0] / m2[1] - 1.0) <= 0.05, (what, m2)
    return stats


@pytest.mark.parametrize("shape,method", CASES)
def test_two_dependent_levels_fit_the_model(bce, contexts, shape, method):
    c = contexts(shape, method)
    s, z = c.export_sk()
    V = nm.model(c.params, s, z)
    reps = noise_run.end_run(c, bce.GateDesc, np.random.default_rng(22), per_level=32768, n_in=1024)
    assert [r["checked"] for r in reps] == [32768, 32768]
    _end_level_bars(reps, V, "%s %s" % (shape, method))


# ---- (e) the headline set at size ------------------------------------------------------------------------------------------------------
def test_std128_opt_quarter_of_a_million_bootstraps(bce):
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    c.KeyGen(SEED)
    s, z = c.export_sk()
    V = nm.model(c.params, s, z)
    sd, q = math.sqrt(V["V_out"]), c.params["q"]
    reps = noise_run.end_run(c, bce.GateDesc, np.random.default_rng(23), per_level=131072, n_in=1024)
    assert [r["checked"] for r in reps] == [131072, 131072]
    _end_level_bars(reps, V, "STD128_OPT GINX")
    for r in reps:
        assert r["margin"] > q / 8 - nm.MAX_SIGMAS * sd
    c.close()
