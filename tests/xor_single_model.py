"""Reference for BCE_XOR (include/bce_gpu.h): XOR in one bootstrap of ct1 + ct2 with a three-level test polynomial.  The
oracle has no such gate and its blind rotation takes a gate, not a polynomial, so the blind rotation is restated here in numpy
from the oracle's exported primitives (bsk(), ntt_forward, ntt_inverse, signed_digit_decompose) for GINX and AP; with a plain
gate's polynomial the restatement gives bo_blind_rotate word for word (tests/test_xor_single_model.py), which anchors it.  The
tail is the oracle's own: extract_modswitch adds Q/8 + 1 to acc[1][0], BCE_XOR adds nothing, so that much is taken off first.
Nothing of the engine is imported."""
import numpy as np

import pair_model

XOR = 0x10006     # BCE_XOR: gate byte 6 with bit 16 (the bare code 6 is no op of the engine)
OP_REFRESH = 17
AP, GINX = 1, 2


def truth(a, b):
    return a ^ b


def mulmod(a, b, Q):
    """a * b mod Q on uint64 arrays of values below Q < 2^41, exact"""
    a, b, Q = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64), np.uint64(Q)
    if int(Q) < 1 << 32:
        return (a * b) % Q
    assert int(Q) < 1 << 41
    sh = np.uint64(20)
    return ((((a * (b >> sh)) % Q) << sh) + a * (b & np.uint64((1 << 20) - 1))) % Q


class _Keys:
    """the oracle's bootstrapping key in evaluation form, one RGSW ciphertext ([2 dG][2][N]) at a time, and the monomials"""

    def __init__(self, o):
        p = o.params
        self.o, self.R, self.N = o, 2 * p["dG"], o.N
        lead = (o.n, 2) if p["method"] == GINX else (o.n, p["baseR"], p["dR"])
        self.coef = o.bsk().reshape(lead + (self.R, 2, self.N))
        self.rgsw_, self.mono_ = {}, {}

    def rgsw(self, *idx):
        if idx not in self.rgsw_:
            self.rgsw_[idx] = np.stack([np.stack([self.o.ntt_forward(self.coef[idx][l][j]) for j in range(2)]) for l in range(self.R)])
        return self.rgsw_[idx]

    def mono(self, a):
        """X^a - 1 mod X^N + 1 in evaluation form, 0 <= a < 2N (the CGGI key encrypts s+ and s-: acc += acc (X^a - 1) s+ ...)"""
        if a not in self.mono_:
            Q = self.o.params["Q"]
            m = np.zeros(self.N, dtype=np.uint64)
            m[a % self.N] = 1 if a < self.N else Q - 1
            m[0] = (int(m[0]) + Q - 1) % Q
            self.mono_[a] = self.o.ntt_forward(m)
        return self.mono_[a]


def _keys(o):
    if getattr(o, "_xor_single_keys", None) is None:
        o._xor_single_keys = _Keys(o)
    return o._xor_single_keys


def plain_poly(params, op, b):
    """BootstrapGateCore's test polynomial of a plain gate (coefficient form)"""
    q, Q, N = params["q"], params["Q"], params["N"]
    f, q1 = 2 * N // q, pair_model.Q1_EIGHTHS[op] * (q // 8)
    q2 = (q1 + q // 2) % q
    t = (b - np.arange(q // 2)) % q
    inside = ((t >= q1) & (t < q2)) if q1 < q2 else ~((t >= q2) & (t < q1))
    m = np.zeros(N, dtype=np.uint64)
    m[::f] = np.where(inside, Q - (Q // 8 + 1), Q // 8 + 1)
    return m


def xor_poly(params, b):
    """the three-level polynomial of BCE_XOR: one = 2 (Q/8 + 1) on [q/8, 3q/8), Q - one on [5q/8, 7q/8), 0 elsewhere"""
    q, Q, N = params["q"], params["Q"], params["N"]
    f, e, one = 2 * N // q, q // 8, 2 * (Q // 8 + 1) % Q
    t = (b - np.arange(q // 2)) % q
    m = np.zeros(N, dtype=np.uint64)
    m[::f] = np.where((t >= e) & (t < 3 * e), one, np.where((t >= 5 * e) & (t < 7 * e), Q - one, 0))
    return m


def _digits(o, acc):
    """SignedDigitDecompose of acc (evaluation form [2][N]): [2 dG][N] in evaluation form"""
    dct = o.signed_digit_decompose(np.stack([o.ntt_inverse(acc[0]), o.ntt_inverse(acc[1])]))
    return np.stack([o.ntt_forward(d) for d in dct])


def _times(dct, ek, Q):
    """digits x one RGSW ciphertext ([2 dG][2][N]): [2][N], reduced"""
    return mulmod(dct[:, None, :], ek, Q).sum(axis=0, dtype=np.uint64) % np.uint64(Q)     # 2 dG <= 16 terms below Q < 2^41: no overflow


def blind_rotate(o, m, prep):
    """the accumulator (0, m) after the blind rotation by the prepared ciphertext, coefficient form [2 N] like bo_blind_rotate
    (rgsw-acc-cggi.cpp / rgsw-acc-dm.cpp EvalAcc as the oracle restates them)"""
    p, K = o.params, _keys(o)
    q, Q, N = p["q"], p["Q"], o.N
    f = 2 * N // q
    acc = np.stack([np.zeros(N, dtype=np.uint64), o.ntt_forward(m)])
    for i in range(o.n):
        a = (q - int(prep[i])) % q
        if p["method"] == GINX:   # acc += (dct x ek1) mono[a] + (dct x ek2) mono[-a]
            if a == 0:
                continue          # mono[0] = X^0 - 1 = 0: the step adds nothing, word for word
            dct, ipos = _digits(o, acc), (a * f) % (2 * N)
            r1, r2 = _times(dct, K.rgsw(i, 0), Q), _times(dct, K.rgsw(i, 1), Q)
            acc = (mulmod(r1, K.mono(ipos)[None, :], Q) + mulmod(r2, K.mono((2 * N - ipos) % (2 * N))[None, :], Q) + acc) % np.uint64(Q)
        else:                     # acc = dct x ek, one key per non-zero base-baseR digit of -a_i
            for k in range(p["dR"]):
                a0 = a % p["baseR"]
                a //= p["baseR"]
                if a0:
                    acc = _times(_digits(o, acc), K.rgsw(i, a0, k), Q)
    return np.concatenate([o.ntt_inverse(acc[0]), o.ntt_inverse(acc[1])])


def stages(o, ca, cb, neg0=0, neg1=0):
    """every stage of BCE_XOR on the ciphertexts ca, cb (EvalNOT folded in where neg0 / neg1): acc / lweN / ks / out"""
    Q, N = o.params["Q"], o.N
    a = o.eval_not(ca) if neg0 else ca
    b = o.eval_not(cb) if neg1 else cb
    prep = o.gate_prep(pair_model.AND, a, b)          # ct1 + ct2
    acc = blind_rotate(o, xor_poly(o.params, int(prep[o.n])), prep)
    shifted = acc.copy()
    shifted[N] = (int(acc[N]) + Q - (Q // 8 + 1)) % Q   # the oracle's tail adds Q/8 + 1; BCE_XOR's adds nothing
    lweN = o.extract_modswitch(shifted)
    ks = o.keyswitch(lweN)
    return {"acc": acc, "lweN": lweN, "ks": ks, "out": o.modswitch_final(ks)}


def eval_desc(o, pool, d):
    """one descriptor (op, in0, in1, out, neg0, neg1) on a pool {slot: ciphertext}: BCE_XOR through stages(), a refresh through
    the oracle's Bootstrap, everything else through pair_model.eval_desc"""
    op, in0, in1, out, neg0, neg1 = (tuple(d) + (0, 0))[:6]
    if op == XOR:
        pool[out] = stages(o, pool[in0], pool[in1], neg0, neg1)["out"]
    elif op == OP_REFRESH:
        pool[out] = o.bootstrap(o.eval_not(pool[in0]) if neg0 else pool[in0])
    else:
        pair_model.eval_desc(o, pool, d)
