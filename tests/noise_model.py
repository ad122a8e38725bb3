"""Analytic noise model of EvalBinGate (FHEW / GINX and AP gate bootstrap) and the host-side phase arithmetic of the noise
tests.  A helper, not a test: plain Python / numpy, no import of the oracle or of the engine, so that what it states is
independent of both.  DESIGN.md "Noise" carries the same formulas with the measured ratios.

Model (sigma^2 = 3.19^2, the error width of every key row and fresh encryption):

  digits     a signed gadget digit is uniform on [-B/2, B/2): E[d_l^2] = (B^2 + 2) / 12 for l < dG - 1; the top digit spans
             only w = Q / B^(dG-1) values: E[d_top^2] = w^2 / 12.  D = sum_l E[d_l^2].
  product    one external product (2 dG rows, two RLWE components) adds P = 2 N D sigma^2 per accumulator coefficient.
  GINX       V_acc = (n - 1) (1 - 1/q) 4 P: two keys per step, the factor (X^a - 1) doubles the variance, a rotation by 0
             adds nothing, and the first step multiplies the noiseless test polynomial (tiny digits), hence n - 1.
  AP         V_acc = (n E_a[#non-zero base-baseR digits of a] - 1) P, the expectation by enumeration of a in [0, q).
  lweN       V_N = V_acc (qKS/Q)^2 + (1 + |z|^2) / 12, the rounding term 0 when qKS = Q (RoundqQ is then the identity).
  ks         V_ks = V_N + N dKS sigma^2 (the rows of digit 0 are real encryptions and are subtracted too).
  out        V_out = V_ks (q/qKS)^2 + (1 + |s|^2) / 12.
  mean       key-dependent, not zero: signed digits have mean -1/2 and the key switch picks one of baseKS FIXED error terms
             per row.  V_bias = the variance, over keys, of that mean: the formulas above with every E[d_l^2] replaced by
             1/4, the key-switch term divided by baseKS and, for the rounding terms, only what RoundqQ's ties leave:
             round-to-nearest of a uniform word has mean zero whatever the key, except that floor(0.5 + x) rounds a tie up,
             and where the modulus ratio r is an even integer (qKS / q = 16 for the tabulated sets) one word in r is a tie:
             +1/(2r) per word, a mean of (1 - sum of the key) / (2r), whose square averages (1 + |key|^2) / (4 r^2) (0.33 of
             V_bias,out = 0.98 at STD128_OPT).  A floor in place of the rounding has mean -1/2 (1 - sum of the key), r times
             as much, which is what the bar on the mean is there to catch.  Bar: |mean| <= 5 sqrt(V_bias + V / M).
  one key    V is the second moment averaged over keys: of it, V_bias is the expected SQUARE of the key's mean.  For the key at
             hand the prediction is V - V_bias + mean^2 (second_moment_for_key), and that is what a measurement is held
             against.  The difference is below 1 % of V everywhere but after KeySwitch with a small baseKS (baseKS = 28, qKS =
             2^19: V_bias / V_ks = 3.5 %, so a key whose mean sits 2.4 bias-sigmas out measures 1.18 V_ks: seen on the device,
             DESIGN.md "Noise").
"""
import math

import numpy as np

SIGMA = 3.19
SIGMA2 = SIGMA * SIGMA
BAND = (0.90, 1.10)        # measured / modelled second moment, at sample sizes whose sampling error is <= 1.6 %
BAND_M600 = (0.80, 1.20)   # the one stage-level CPU test at M = 600 (sampling error 6 %)
MAX_SIGMAS = 6.5           # largest |error| of a bootstrap output over <= 2^18 samples
AP, GINX = 1, 2


# ---- the model -------------------------------------------------------------------------------------------------------------
def digit_second_moments(Q, B, dG):
    """E[d_l^2], l = 0 .. dG - 1, of SignedDigitDecompose of a uniform residue mod Q"""
    w = Q / float(B) ** (dG - 1)
    return [(B * B + 2) / 12.0] * (dG - 1) + [w * w / 12.0]


def ap_nonzero_digits_mean(q, baseR, dR):
    """E over a uniform on [0, q) of the number of non-zero base-baseR digits of a (the AP steps of one key coefficient)"""
    a = np.arange(q, dtype=np.int64)
    cnt = np.zeros(q, dtype=np.int64)
    for _ in range(dR):
        cnt += (a % baseR) != 0
        a //= baseR
    assert not a.any(), "dR digits do not cover q"
    return float(cnt.sum()) / q


def _tie_bias(frm, to, norm2):
    """variance over keys of the mean that the ties of RoundqQ(frm -> to) leave in a phase under a key of squared norm norm2"""
    if frm % to or (frm // to) % 2:
        return 0.0
    return (1.0 + norm2) / (4.0 * (frm // to) ** 2)


def _acc(p, D):
    n, N, q = p["n"], p["N"], p["q"]
    P = 2.0 * N * D * SIGMA2
    if p["method"] == GINX:
        return (n - 1) * (1.0 - 1.0 / q) * 4.0 * P
    return (n * ap_nonzero_digits_mean(q, p["baseR"], p["dR"]) - 1.0) * P


def model(p, s, z):
    """expected second moments of the phase error after extract + ModSwitch (under z, mod qKS), after KeySwitch (under s,
    mod qKS) and of the gate output (under s, mod q), and the variances of their key-dependent means.
    p: the parameter dict of a context; s, z: the actual secrets (only their squared norms enter)."""
    s2 = float(np.sum(np.asarray(s, dtype=np.int64) ** 2))
    z2 = float(np.sum(np.asarray(z, dtype=np.int64) ** 2))
    q, Q, qKS, N = p["q"], p["Q"], p["qKS"], p["N"]
    out = {}
    for tag, D, ks_div, round_N, round_out in (
            ("V", sum(digit_second_moments(Q, p["baseG"], p["dG"])), 1.0, (1.0 + z2) / 12.0 if qKS != Q else 0.0, (1.0 + s2) / 12.0),
            ("B", p["dG"] / 4.0, float(p["baseKS"]), _tie_bias(Q, qKS, z2), _tie_bias(qKS, q, s2))):
        acc = _acc(p, D)
        vN = acc * (float(qKS) / Q) ** 2 + round_N
        vks = vN + N * p["dKS"] * SIGMA2 / ks_div
        vout = vks * (float(q) / qKS) ** 2 + round_out
        out.update({tag + "_acc": acc, tag + "_N": vN, tag + "_ks": vks, tag + "_out": vout})
    return out


def second_moment_for_key(V, V_bias, mean):
    """the model's second moment for the key whose mean phase error is `mean`: the variance about the mean, V - V_bias, plus
    mean^2 (V itself is the average of this over keys)"""
    return V - V_bias + mean * mean


def mean_bar(V, V_bias, M):
    """bar on |sample mean| of M phase errors of second moment V whose key-dependent mean has variance V_bias"""
    return 5.0 * math.sqrt(V_bias + V / M)


def check_report(rep, V_out, min_band_samples=200):
    """asserts on a bce_check report whose checked slots are ALL bootstrap outputs: no sample beyond 6.5 sigma, and (from
    200 samples on: a dozen samples carry no band) the second moment within BAND of V_out, used as it stands (for a gate
    output V_bias is below 1 % of it).  Returns measured / modelled second moment."""
    sd = math.sqrt(V_out)
    ratio = rep["sum_sq_err"] / rep["checked"] / V_out
    assert rep["max_abs_err"] <= MAX_SIGMAS * sd, (rep["max_abs_err"], sd)
    if rep["checked"] >= min_band_samples:
        lo, hi = BAND
        assert lo <= ratio <= hi, "second moment %.2f, model %.2f, ratio %.3f outside [%.3f, %.3f] at M = %d" % (
            rep["sum_sq_err"] / rep["checked"], V_out, ratio, lo, hi, rep["checked"])
    return ratio


# ---- host-side phases ------------------------------------------------------------------------------------------------------
def centred(x, m):
    """residues mod m -> representatives in [-m/2, m/2)"""
    x = np.asarray(x, dtype=np.int64) % m
    return np.where(x >= (m + 1) // 2, x - m, x)


def lwe_phase_error(cts, key, modulus, bits):
    """centred (b - <a, key> - bit modulus / 4) mod modulus of ciphertext rows [count][len(key) + 1] encrypting `bits`"""
    cts = np.asarray(cts)
    key = np.asarray(key, dtype=np.int64)
    assert cts.ndim == 2 and cts.shape[1] == key.size + 1
    assert int(cts.max()) < modulus and key.size * modulus < (1 << 62)
    a = cts[:, :-1].astype(np.int64)
    msg = (np.asarray(bits, dtype=np.int64) * modulus + 2) // 4          # round(bit modulus / 4) for bit in 0 .. 3
    return centred(cts[:, -1].astype(np.int64) - a @ key - msg, modulus)


def negacyclic_matrix(z):
    """Z with (a * z mod X^N + 1) = a @ Z for row vectors a"""
    z = np.asarray(z, dtype=np.int64)
    N = z.size
    ext = np.concatenate([-z, z])                    # ext[N + d] = z[d], ext[d] = -z[d]: index N + k - i
    idx = N + np.arange(N)[None, :] - np.arange(N)[:, None]
    return ext[idx]


def negacyclic_mul(a, z, Q):
    """rows of a [rows][N] (residues mod Q) times the small polynomial z, mod (X^N + 1, Q).  The products run as an exact
    float64 matrix product: every partial sum is an integer below N Q max|z| < 2^53."""
    a = np.asarray(a)
    Z = negacyclic_matrix(z)
    assert a.shape[-1] == Z.shape[0] and Z.shape[0] * Q * max(1, int(np.abs(Z).max())) < (1 << 53)
    prod = a.astype(np.float64) @ Z.astype(np.float64)
    return prod.astype(np.int64) % Q


# ---- key noise ---------------------------------------------------------------------------------------------------------------
def ksk_errors(ksk, p, s, z):
    """every row of the key-switching key K[i][v][j] = LWE_s(z_i v baseKS^j) mod qKS: its error, [N][baseKS][dKS]"""
    n, N, B, D, qKS = p["n"], p["N"], p["baseKS"], p["dKS"], p["qKS"]
    rows = np.asarray(ksk).reshape(N * B * D, n + 1).astype(np.int64)
    zi = np.asarray(z, dtype=np.int64)[:, None, None]
    v = np.arange(B, dtype=np.int64)[None, :, None]
    pw = np.array([pow(B, j, qKS) for j in range(D)], dtype=np.int64)[None, None, :]
    msg = (zi * ((v * pw) % qKS)) % qKS
    e = rows[:, n] - rows[:, :n] @ np.asarray(s, dtype=np.int64) - msg.reshape(-1)
    return centred(e, qKS).reshape(N, B, D)


def rgsw_ids(p, s, step=1):
    """(id, sign, exponent) of the RGSW ciphertexts of the bootstrapping key that encrypt something: id in the order of
    export_bsk, message sign X^exponent (sign 0: an encryption of 0), for every step-th secret coefficient"""
    n, N, q = p["n"], p["N"], p["q"]
    out = []
    for i in range(0, n, step):
        si = int(s[i])
        if p["method"] == GINX:
            out.append((2 * i, int(si == 1), 0))
            out.append((2 * i + 1, int(si == -1), 0))
        else:
            BR, DR = p["baseR"], p["dR"]
            for v in range(1, BR):                       # v = 0 is never used and holds zeros
                for k in range(DR):
                    mm = ((si * v * BR ** k) % q) * (2 * N // q)
                    out.append(((i * BR + v) * DR + k, -1 if mm >= N else 1, mm % N))
    return out


def rgsw_errors(bsk, p, z, ids):
    """errors of the RGSW ciphertexts `ids` (from rgsw_ids) of a coefficient-form bootstrapping key in export_bsk's layout
    [id][row r = 2 l + component][a | b][N]: row r holds (a + [component 0] m B^l, a z + e + [component 1] m B^l).
    Returns [len(ids)][2 dG][N]; a wrong message, component or coefficient shows as an error of the order of Q."""
    N, Q, dG, B = p["N"], p["Q"], p["dG"], p["baseG"]
    R = 2 * dG
    bsk = np.asarray(bsk).reshape(-1, R, 2, N)
    sel = bsk[[i for i, _, _ in ids]].astype(np.int64)         # [ids][R][2][N]
    a, b = sel[:, :, 0, :].copy(), sel[:, :, 1, :].copy()
    for t, (_, sign, mm) in enumerate(ids):
        for r in range(R):
            g = (sign * pow(B, r >> 1, Q)) % Q
            tgt = b if (r & 1) else a
            tgt[t, r, mm] = (tgt[t, r, mm] - g) % Q
    az = negacyclic_mul(a.reshape(-1, N), z, Q).reshape(a.shape)
    return centred(b - az, Q)


def error_stats(e):
    """(count, mean, variance about 0, max |e|) of an integer error array"""
    e = np.asarray(e, dtype=np.int64).ravel()
    return e.size, float(e.mean()), float(np.mean(e.astype(np.float64) ** 2)), int(np.abs(e).max())


def assert_key_errors(e, what, var_tol=0.03, max_abs=22):
    """the bars on the error terms of a key or of fresh encryptions: mean within 5 sigma / sqrt(count) of 0, second moment
    within 3 % of sigma^2, |e| <= 22 (7 sigma)"""
    count, mean, var, mx = error_stats(e)
    print("%-28s count %8d  mean %+.4f  variance %.3f (sigma^2 = %.3f)  max |e| %d" % (what, count, mean, var, SIGMA2, mx))
    assert abs(mean) <= 5.0 * SIGMA / math.sqrt(count), (what, mean)
    assert abs(var / SIGMA2 - 1.0) <= var_tol, (what, var)
    assert mx <= max_abs, (what, mx)
    return count, mean, var, mx


def assert_ternary(key, what):
    """entries in {-1, 0, 1}; for a long key the three counts within 5 standard deviations of len / 3"""
    key = np.asarray(key, dtype=np.int64)
    assert set(np.unique(key)) <= {-1, 0, 1}, what
    if key.size >= 256:
        sd = math.sqrt(key.size * (1.0 / 3) * (2.0 / 3))
        for v in (-1, 0, 1):
            assert abs(int((key == v).sum()) - key.size / 3.0) <= 5.0 * sd, (what, v, int((key == v).sum()))


def assert_uniform_buckets(words, modulus, what, buckets=16):
    """words uniform on [0, modulus): the count of each of 16 equal buckets within 5 standard deviations of its expectation"""
    w = np.asarray(words).ravel().astype(np.float64)
    idx = np.minimum((w * buckets / float(modulus)).astype(np.int64), buckets - 1)
    cnt = np.bincount(idx, minlength=buckets)
    edges = np.ceil(np.arange(buckets + 1) * float(modulus) / buckets)
    prob = np.diff(edges) / float(modulus)
    exp = w.size * prob
    sd = np.sqrt(w.size * prob * (1.0 - prob))
    assert np.all(np.abs(cnt - exp) <= 5.0 * sd), (what, cnt.tolist(), exp.tolist())


def signed_digits(x, Q, B, dG):
    """SignedDigitDecompose of residues x mod Q as signed integers [dG][len(x)] (B a power of two)"""
    x = np.asarray(x, dtype=np.int64)
    d = np.where(x < (Q >> 1), x, x - Q)
    gb = B.bit_length() - 1
    assert 1 << gb == B
    out = []
    for _ in range(dG):
        r = ((d + B // 2) % B) - B // 2                  # signed remainder in [-B/2, B/2)
        d = (d - r) >> gb
        out.append(r)
    return np.stack(out)


# ---- gates -------------------------------------------------------------------------------------------------------------------
OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST = range(6)
TWO_INPUT = (OR, AND, NOR, NAND)


def gate_truth(op, a, b):
    """truth values of gates op (one op or an array of ops) on input bits a, b"""
    op, a, b = np.broadcast_arrays(np.asarray(op, dtype=np.int64), np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    either, both, differ = a | b, a & b, a ^ b
    table = np.stack([either, both, 1 - either, 1 - both, differ, 1 - differ])      # rows in the order of the op codes
    return np.take_along_axis(table, op[None], axis=0)[0]


def random_gates(rng, count, n_inputs, ops=TWO_INPUT):
    """`count` gates over distinct random ordered pairs (in0 != in1) of n_inputs registers: (ops, in0, in1)"""
    pairs = n_inputs * (n_inputs - 1)
    assert count <= pairs
    if pairs <= 4 * count:
        code = rng.permutation(pairs)[:count]
    else:
        code = np.unique(rng.integers(0, pairs, 2 * count))
        while code.size < count:
            code = np.unique(np.concatenate([code, rng.integers(0, pairs, count)]))
        code = rng.permutation(code)[:count]
    in0, r = code // (n_inputs - 1), code % (n_inputs - 1)
    in1 = r + (r >= in0)
    op = np.array(ops, dtype=np.int64)[rng.integers(0, len(ops), count)]
    return op, in0.astype(np.int64), in1.astype(np.int64)


# ---- statistics of a measurement ---------------------------------------------------------------------------------------------
def report_stats(rep, V, V_bias):
    """(second moment / the model's for this key, mean, its bar, max |e| in sigmas) of a device report"""
    M = rep["checked"]
    mean = rep["sum_err"] / M
    return rep["sum_sq_err"] / M / second_moment_for_key(V, V_bias, mean), mean, mean_bar(V, V_bias, M), rep["max_abs_err"] / math.sqrt(V)


def stage_stats(err, V, V_bias):
    """(second moment / the model's for this key, second moment / V, mean, its bar, max |e| in sigmas, second moment) of
    host-side phase errors"""
    M, mean, m2, mx = error_stats(err)
    return m2 / second_moment_for_key(V, V_bias, mean), m2 / V, mean, mean_bar(V, V_bias, M), mx / math.sqrt(V), m2
