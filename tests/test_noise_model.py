"""The size of the noise, on the CPU: the analytic model of tests/noise_model.py against the oracle, and the oracle's keys
and encryptions against sigma = 3.19.  Every other test of the oracle asks which bit comes out; these ask how much noise a
key row, an encryption and each stage of a bootstrap carry, which a shared misreading of the scheme (unsigned digits, a wrong
Gaussian width, key rows without error, a floor for a rounding) changes without changing a single decrypted bit.

Bars (all set by the model and sigma, none by what the oracle happens to give): second moments within [0.90, 1.10] of the
model ([0.80, 1.20] for the one test at 600 samples), means within 5 sqrt(V_bias + V/M), key and encryption errors with mean
within 5 sigma / sqrt(count), second moment within 3 % of sigma^2 and |e| <= 22."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import noise_model as nm

SEED = 0x0FE5EED


def _q27(L, N):
    return int(L.bo_previous_prime(L.bo_first_prime(27, 2 * N), 2 * N))


def _ratio_in(ratio, band, what):
    assert band[0] <= ratio <= band[1], "%s: measured / model = %.3f outside [%.2f, %.2f]" % (what, ratio, band[0], band[1])


# ---- model against oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GINX", "AP"])
def test_gate_output_noise_of_the_oracle_fits_the_model(orc, method):
    """TOY, 4000 gates (the four two-input gates) on distinct random pairs of 64 fresh encryptions"""
    o = orc.Oracle(orc.TOY, getattr(orc, method))
    o.keygen(SEED)
    p, s = o.params, o.sk()
    V = nm.model(p, s, o.z())
    rng = np.random.default_rng(11)
    n_in, M = 64, 4000
    bits = rng.integers(0, 2, n_in)
    pool = np.zeros((n_in + M, o.n + 1), dtype=np.uint64)
    for i, b in enumerate(bits):
        pool[i] = o.encrypt(int(b), 7000 + i)
    op, in0, in1 = nm.random_gates(rng, M, n_in)
    assert o.eval_gates(pool, [(int(g), int(a), int(b), n_in + k, 0, 0) for k, (g, a, b) in enumerate(zip(op, in0, in1))]) == M
    want = np.array([nm.gate_truth(g, bits[a], bits[b]) for g, a, b in zip(op, in0, in1)])
    outs = pool[n_in:]
    wrong = sum(int(o.decrypt(ct) != w) for ct, w in zip(outs, want))
    err = np.array([o.noise(ct, int(w)) for ct, w in zip(outs, want)], dtype=np.int64)
    assert np.array_equal(err, nm.lwe_phase_error(outs, s, p["q"], want)), "host phase arithmetic differs from bo_noise"
    ratio, raw, mean, bar, mx, m2 = nm.stage_stats(err, V["V_out"], V["B_out"])
    print("TOY %s: second moment %.2f, model %.2f, ratio %.3f (against V itself %.3f); mean %+.3f (bar %.3f); max |e| %.2f sigma" % (
        method, m2, V["V_out"], ratio, raw, mean, bar, mx))
    assert wrong == 0
    _ratio_in(ratio, nm.BAND, "TOY " + method)
    assert abs(mean) <= bar
    o.close()


@pytest.mark.parametrize("method", ["GINX", "AP"])
def test_every_stage_of_the_oracle_fits_the_model(orc, method):
    """n = 32, N = 1024, q = 1024, the 27-bit prime, base 2^7, qKS = 2^14, baseKS = 2^7: 600 bootstraps taken apart into
    extract + ModSwitch (phase under z), KeySwitch and the final ModSwitch (phases under s).  The stage plumbing the GPU
    test reuses; at M = 600 the sampling error is 6 %, hence (here only) the band [0.80, 1.20]."""
    L = orc.lib()
    o = orc.Oracle(method=getattr(orc, method), custom=(32, 1024, 1024, _q27(L, 1024), 1 << 14, 1 << 7, 1 << 7, 32))
    o.keygen(SEED + 1)
    p, s, z = o.params, o.sk(), o.z()
    V = nm.model(p, s, z)
    rng = np.random.default_rng(12)
    n_in, M = 64, 600
    bits = rng.integers(0, 2, n_in)
    fresh = [o.encrypt(int(b), 100 + i) for i, b in enumerate(bits)]
    op, in0, in1 = nm.random_gates(rng, M, n_in)

    def one(k):
        g = int(op[k])
        acc = o.blind_rotate(g, o.gate_prep(g, fresh[in0[k]], fresh[in1[k]]))
        lweN = o.extract_modswitch(acc)
        ks = o.keyswitch(lweN)
        return lweN, ks, o.modswitch_final(ks)

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(M)))
    want = np.array([nm.gate_truth(g, bits[a], bits[b]) for g, a, b in zip(op, in0, in1)])
    stages = (("N", np.stack([r[0] for r in res]), z, p["qKS"]), ("ks", np.stack([r[1] for r in res]), s, p["qKS"]),
              ("out", np.stack([r[2] for r in res]), s, p["q"]))
    assert [o.decrypt(ct) for ct in stages[2][1]] == list(want)
    for tag, cts, key, mod in stages:
        ratio, raw, mean, bar, mx, m2 = nm.stage_stats(nm.lwe_phase_error(cts, key, mod, want), V["V_" + tag], V["B_" + tag])
        print("%s stage %-3s second moment %.2f, model %.2f, ratio %.3f (against V itself %.3f); mean %+.3f (bar %.3f); max |e| %.2f sigma" % (
            method, tag, m2, V["V_" + tag], ratio, raw, mean, bar, mx))
        _ratio_in(ratio, nm.BAND_M600, "%s stage %s" % (method, tag))
        assert abs(mean) <= bar, (tag, mean, bar)
    o.close()


# ---- keys and encryptions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["GINX", "AP"])
def test_keys_of_the_oracle_keygen_carry_sigma(orc, method):
    """TOY: every key-switch row decrypts to z_i v baseKS^j + e, every RGSW row under z to m B^l in the right component and
    coefficient + e (a wrong message shows as |e| of the order of the modulus); the secrets are ternary"""
    o = orc.Oracle(orc.TOY, getattr(orc, method))
    o.keygen(SEED)
    p, s, z = o.params, o.sk(), o.z()
    nm.assert_ternary(s, "s")
    nm.assert_ternary(z, "z")
    nm.assert_key_errors(nm.ksk_errors(o.ksk(), p, s, z), "key-switching key")
    ids = nm.rgsw_ids(p, s)
    assert len(ids) == (2 * p["n"] if method == "GINX" else p["n"] * (p["baseR"] - 1) * p["dR"])
    nm.assert_key_errors(nm.rgsw_errors(o.bsk(), p, z, ids), "bootstrapping key " + method)
    o.close()


def test_fresh_encryptions_carry_sigma(orc):
    """20 000 encryptions of one fixed index range.  At this size the 3 % bar is three standard errors of a second moment
    (sqrt(2/M) = 1 %): about one range in 400 misses it by chance, and the range starting at 50 000 is such a one (10.49;
    760 000 encryptions over fourteen ranges pool to 10.186 against sigma^2 = 10.176)."""
    o = orc.Oracle(orc.TOY, orc.GINX)
    o.keygen(SEED)
    M = 20000
    bits = np.arange(M) % 2
    cts = np.stack([o.encrypt(int(b), 2000000 + i) for i, b in enumerate(bits)])
    err = nm.lwe_phase_error(cts, o.sk(), o.params["q"], bits)
    nm.assert_key_errors(err, "fresh encryptions")
    nm.assert_uniform_buckets(cts[:, :-1], o.params["q"], "a-words of fresh encryptions")
    o.close()


# ---- the model's own arithmetic -------------------------------------------------------------------------------------------------
def test_digit_second_moments_against_a_direct_count(orc):
    L = orc.lib()
    q27 = _q27(L, 1024)
    q37 = int(L.bo_previous_prime(L.bo_first_prime(37, 4096), 4096))
    rng = np.random.default_rng(13)
    for Q, B, dG in ((q27, 1 << 7, 4), (q27, 1 << 9, 3), (q37, 1 << 13, 3)):
        x = rng.integers(0, Q, 400000)
        d = nm.signed_digits(x, Q, B, dG)
        # the digits recompose the centred residue modulo B^dG (where Q/2 rounds up to B^dG / 2 the top digit wraps, as upstream)
        centred = np.where(x < (Q >> 1), x, x - Q)
        assert not (((d * (B ** np.arange(dG))[:, None]).sum(axis=0) - centred) % B ** dG).any(), "digits do not recompose"
        assert d.min() >= -B // 2 and d.max() < B // 2
        got = (d.astype(np.float64) ** 2).mean(axis=1)
        want = nm.digit_second_moments(Q, B, dG)
        print(Q, B, dG, [round(float(g / w), 4) for g, w in zip(got, want)], "digit means", d.mean(axis=1).round(3).tolist())
        for l in range(dG):
            assert abs(got[l] / want[l] - 1.0) <= 0.01, (Q, B, l, got[l], want[l])
        assert np.all(np.abs(d[:-1].mean(axis=1) + 0.5) < 5 * B / math.sqrt(12 * 400000.0)), "lower digits: mean -1/2"


def test_ap_step_count_against_brute_force():
    for q, baseR in ((512, 23), (1024, 32), (2048, 46)):
        dR = int(math.ceil(math.log(q) / math.log(baseR)))
        total = 0
        for a in range(q):
            for _ in range(dR):
                total += 1 if a % baseR else 0
                a //= baseR
        assert abs(nm.ap_nonzero_digits_mean(q, baseR, dR) - total / q) < 1e-12
        assert total / q < dR * (baseR - 1.0) / baseR or baseR ** dR == q     # the top digit of a non-power base is rarely set
