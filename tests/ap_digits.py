"""The AP (DM) digit geometry (baseR, dR) as a test dimension (test helper: plain numpy and Python integers, nothing of the engine).

A blind rotation of the AP method walks the dR = ceil(log q / log baseR) base-baseR digits of -a_i mod q of every LWE
coefficient; digit a0 != 0 at position k of coefficient i is one step, which multiplies the accumulator by the RGSW ciphertext
number (i baseR + a0) dR + k of a key of n baseR dR ciphertexts that encrypt X^(s_i a0 baseR^k 2N/q).  Every tabulated set
has dR = 2 (baseR = 23, 32 or 46), so that is all the other suites run.  This module restates the digit count, the digits, the
key index and the key size in a few lines, names the classes of (q, baseR) the formulas produce, lists the geometries the
sweep (tests/test_gpu_ap_digits.py) runs on every AP build of the four kernel bodies that decode a step, and builds the edge
ciphertexts.  The CPU half of the sweep asserts that the lists hit every class on every body and build, so a shortened list fails
on any machine.
"""
import math

import numpy as np

import worst_case as wc
import xor_single_model as xm

AP = wc.AP
KEY_BYTES_MAX = 250 * 10 ** 6           # a bootstrapping key as u64 words, the largest the sweep makes


# ---- the rules, restated -----------------------------------------------------------------------------------------------
def digit_count(q, base):
    """ceil(log q / log base) in doubles: the engine's and the oracle's digit_count, OpenFHE's dR"""
    return int(math.ceil(math.log(float(q)) / math.log(float(base))))


def digits(q, baseR, dR, a):
    """the dR base-baseR digits of -a mod q, lowest first"""
    v, out = (q - int(a)) % q, []
    for _ in range(dR):
        out.append(v % baseR)
        v //= baseR
    assert v == 0, "dR digits do not hold q - 1"
    return out


def value(q, baseR, digs):
    """the a whose -a mod q has the digits `digs` (which must stay below q)"""
    v = sum(d * baseR ** k for k, d in enumerate(digs))
    assert v < q, (q, baseR, digs)
    return (q - v) % q


def key_index(i, a0, k, baseR, dR):
    """the RGSW ciphertext a step reads: layout [n][baseR][dR]"""
    return (i * baseR + a0) * dR + k


def rgsw_count(n, baseR, dR):
    return n * baseR * dR


def bsk_words(n, N, dG, baseR, dR):
    """words of the AP key: an RGSW ciphertext is 2 dG rows of 2 polynomials"""
    return rgsw_count(n, baseR, dR) * 2 * dG * 2 * N


def digit_max(q, baseR, dR, k):
    """the largest digit position k of any -a mod q can show: baseR - 1 below the top (dR >= 2 means baseR < q), and
    (q - 1) // baseR^(dR - 1) at the top, which is below baseR - 1 unless q is a power of baseR"""
    return baseR - 1 if k < dR - 1 else (q - 1) // baseR ** (dR - 1)


CLASSES = ("dR=1, baseR=q", "dR=1, baseR>q", "dR=3, exact power", "dR=3, non-power", "long digit string")


def classify(q, baseR):
    """the class of a geometry, from the formulas alone (dR = 2 belongs to the other suites: None)"""
    dR = digit_count(q, baseR)
    if dR == 1:
        return CLASSES[0] if baseR == q else CLASSES[1]
    if dR == 3:
        return CLASSES[2] if baseR ** 3 == q else CLASSES[3]
    return CLASSES[4] if dR >= 7 else None


# ---- the sweep's geometries ----------------------------------------------------------------------------------------------
# name -> {N: (q, baseR)}: baseR = q keeps q small on the large rings, so that n baseR RGSW ciphertexts stay below KEY_BYTES_MAX
GEOMETRIES = {
    "A": {512: (512, 512), 1024: (256, 256), 2048: (128, 128)},     # dR = 1: one step per coefficient, digit = -a itself
    "B": {512: (256, 300), 1024: (256, 300), 2048: (128, 150)},     # dR = 1, baseR > q: the digit never reaches baseR - 1, the
                                                                    # key rows a0 >= q are generated and never read
    "C": {512: (512, 8), 1024: (512, 8), 2048: (512, 8)},           # dR = 3, q = baseR^3: every digit reaches baseR - 1
    "D1": {512: (1024, 23), 1024: (1024, 23), 2048: (1024, 23)},    # dR = 3, 23^2 = 529: the top digit is 0 or 1
    "D2": {1024: (2048, 45), 2048: (2048, 45)},                     # dR = 3, 45^2 = 2025: top digit 0 or 1; 2N/q = 1 at N = 1024
    "E1": {512: (1024, 2), 1024: (1024, 2), 2048: (1024, 2)},       # dR = 10: every digit 0 or 1, 10 n steps at the most
    "E2": {512: (1024, 3), 1024: (1024, 3), 2048: (1024, 3)},       # dR = 7, 3^6 = 729: top digit 0 or 1
}
GEOMETRY_CLASS = {"A": CLASSES[0], "B": CLASSES[1], "C": CLASSES[2], "D1": CLASSES[3], "D2": CLASSES[3], "E1": CLASSES[4], "E2": CLASSES[4]}
DR = {"A": 1, "B": 1, "C": 3, "D1": 3, "D2": 3, "E1": 10, "E2": 7}

# The four kernel bodies that decode an AP step (i, k, a0 -> key index), and per body the AP builds the engine can launch:
# (body, build, N, log2 baseG, modulus, selectors, accessor expectations, (a dR = 1 geometry, a dR >= 3 geometry)).
# modulus: "q27" the 27-bit prime of the tabulated sets, or the number of bits b: the largest prime below 2^b.
SITES = ("wave32", "split", "int64", "fp64")
BUILDS = [
    # k_blind_rotate<logN, dG, lazy, occupancy, AP>
    ("wave32", "9_3_lazy", 512, 9, "q27", {}, {"lazy_arithmetic": 1}, ("A", "C")),
    ("wave32", "9_4_lazy", 512, 7, "q27", {}, {"lazy_arithmetic": 1}, ("B", "D1")),
    ("wave32", "10_3_lazy", 1024, 9, "q27", {}, {"lazy_arithmetic": 1}, ("A", "E1")),
    ("wave32", "10_4_variant1", 1024, 7, "q27", {"BCE_VARIANT": "1"}, {"lazy_arithmetic": 1}, ("B", "D2")),
    ("wave32", "11_3_lazy", 2048, 9, "q27", {}, {"lazy_arithmetic": 1}, ("A", "E2")),
    ("wave32", "9_3_occupancy2", 512, 9, "q27", {"BCE_OCCUPANCY": "2"}, {"lazy_arithmetic": 1}, ("B", "D1")),
    ("wave32", "10_3_nonlazy", 1024, 10, 28, {}, {"lazy_arithmetic": 0}, ("A", "D2")),
    # k_blind_rotate_lat<LatVariant<wps, AP, fused tail, Rows | RowsAndHalves>>: N = 1024, four digits of base 2^7
    ("split", "variant2", 1024, 7, "q27", {"BCE_VARIANT": "2"}, {"forward_transforms_per_step": 6}, ("A", "E1")),
    ("split", "variant2_plain_key", 1024, 7, "q27", {"BCE_VARIANT": "2", "BCE_FOLD": "0"}, {"forward_transforms_per_step": 8}, ("B", "D1")),
    ("split", "variant3", 1024, 7, "q27", {"BCE_VARIANT": "3"}, {"forward_transforms_per_step": 6}, ("A", "D2")),
    ("split", "variant3_plain_key", 1024, 7, "q27", {"BCE_VARIANT": "3", "BCE_FOLD": "0"}, {"forward_transforms_per_step": 8}, ("B", "C")),
    ("split", "variant3_separate_tail", 1024, 7, "q27", {"BCE_VARIANT": "3", "BCE_FUSE_TAIL": "0"}, {"forward_transforms_per_step": 6}, ("A", "E2")),
    # k_blind_rotate64<logN, dG, AP>: integer words
    ("int64", "9_3_39bit", 512, 14, 39, {"BCE_FP64": "0"}, {"fp64": 0}, ("A", "C")),
    ("int64", "10_3", 1024, 14, 40, {}, {"fp64": 0}, ("B", "D2")),
    ("int64", "11_3", 2048, 14, 40, {}, {"fp64": 0}, ("A", "E1")),
    ("int64", "9_4", 512, 10, 40, {}, {"fp64": 0}, ("B", "D1")),
    ("int64", "10_4_narrow", 1024, 8, 31, {}, {}, ("A", "E2")),
    ("int64", "11_4_narrow", 2048, 8, 31, {}, {}, ("B", "C")),
    # bootstrap64d<WdVariant<logN, dG, AP, body, folded key, fused tail>>: doubles
    ("fp64", "9_3_wave", 512, 14, 39, {}, {"fp64": 1}, ("A", "D1")),
    ("fp64", "10_3_wave", 1024, 14, 39, {}, {"fp64": 1}, ("B", "D2")),
    ("fp64", "9_4_wave", 512, 10, 39, {}, {"fp64": 1}, ("A", "C")),
    ("fp64", "split8_fold", 2048, 14, 39, {"BCE_VARIANT": "2"}, {"fp64": 1, "forward_transforms_per_step": 4}, ("B", "E1")),
    ("fp64", "split8_plain_key", 2048, 14, 39, {"BCE_VARIANT": "2", "BCE_FOLD": "0"}, {"fp64": 1, "forward_transforms_per_step": 6}, ("A", "D1")),
    ("fp64", "split16_fold_separate_tail", 2048, 14, 39, {"BCE_VARIANT": "3", "BCE_FUSE_TAIL": "0"}, {"fp64": 1, "forward_transforms_per_step": 4}, ("B", "E2")),
    ("fp64", "split16_plain_key", 2048, 14, 39, {"BCE_VARIANT": "3", "BCE_FOLD": "0"}, {"fp64": 1, "forward_transforms_per_step": 6}, ("A", "C")),
    ("fp64", "split16_fused", 2048, 14, 39, {"BCE_VARIANT": "3"}, {"fp64": 1, "forward_transforms_per_step": 4}, ("B", "D2")),
]
# the persistent kernels share the step loop of their body (lat_bootstrap, bootstrap64d); one small DAG each
DAG_BUILDS = [
    ("split", "dag", 1024, 7, "q27", {}, {}, ("A", "E1")),
    ("fp64", "dag64", 2048, 14, 39, {}, {"fp64": 1, "forward_transforms_per_step": 4}, ("A",)),
]


def gadget_digits(bits, gbits):
    """dG = ceil(bits / gbits) for a modulus of `bits` bits ("q27": 27)"""
    return -(-(27 if bits == "q27" else bits) // gbits)


def lwe_dimension(N, dG, q, baseR):
    """n of a sweep context: 8 (4 at N = 2048), less where the key as u64 words would pass KEY_BYTES_MAX"""
    n = 4 if N == 2048 else 8
    while bsk_words(n, N, dG, baseR, digit_count(q, baseR)) * 8 > KEY_BYTES_MAX:
        n -= 1
    return n


def contexts(builds=None):
    """[(body, build, geometry name, N, gbits, modulus, selectors, expectations, (n, q, baseR))] of the sweep"""
    out = []
    for site, build, N, gb, mod, env, expect, geoms in (BUILDS if builds is None else builds):
        for g in geoms:
            q, baseR = GEOMETRIES[g][N]
            out.append((site, build, g, N, gb, mod, env, expect, (lwe_dimension(N, gadget_digits(mod, gb), q, baseR), q, baseR)))
    return out


# ---- edge ciphertexts ----------------------------------------------------------------------------------------------------
def edge_a(q, baseR, dR, n):
    """[(name, prepared a[n], executed steps claimed)]:
      * a = 0: no step, the accumulator stays the test polynomial;
      * for every position k, exactly one non-zero digit at k (1, the position's maximum and a value between them in turn over
        the coefficients);
      * every digit at its maximum: the low digits baseR - 1 with the largest top digit that keeps the value below q, and
        -a = q - 1, whose top digit is the top position's maximum (q - 1) // baseR^(dR - 1);
      * -a = 1."""
    out = [("a=0", [0] * n, 0)]
    for k in range(dR):
        top = digit_max(q, baseR, dR, k)
        ds = [(1, top, max(1, top // 2))[i % 3] for i in range(n)]
        out.append(("one digit, position %d" % k, [value(q, baseR, [0] * k + [d] + [0] * (dR - 1 - k)) for d in ds], n))
    low = [baseR - 1] * (dR - 1)
    top = min(digit_max(q, baseR, dR, dR - 1), (q - 1 - sum(d * baseR ** k for k, d in enumerate(low))) // baseR ** (dR - 1))
    full = low + [top]
    out.append(("low digits baseR-1, top digit %d" % top, [value(q, baseR, full)] * n, n * sum(1 for d in full if d)))
    out.append(("-a=q-1", [1] * n, n * sum(1 for d in digits(q, baseR, dR, 1) if d)))
    out.append(("-a=1", [q - 1] * n, n))
    return out


def random_a(q, n, rng, count=4):
    return [("uniform a %d" % t, [int(v) for v in rng.integers(0, q, n)], None) for t in range(count)]


def cases(o, rng):
    """[(name, gate, prepared ciphertext, ct1)] for the plain gates in turn (ct1 = the prepared ciphertext: the second input
    is the all-zero ciphertext), b on the edges of the gate's window in turn"""
    p = o.params
    q, n = p["q"], o.n
    out = []
    for t, (name, a, _) in enumerate(edge_a(q, p["baseR"], p["dR"], n) + random_a(q, n, rng)):
        gate = wc.PLAIN[t % 4]
        b = wc.b_patterns(q, gate)[(t + 2) % 6]
        prep = np.array(list(a) + [b], dtype=np.uint64)
        out.append(("%s b=%d %s" % (name, b, wc.GATE_NAMES[gate]), gate, prep, prep.copy()))
    return out


def two_operand_cases(o, rng):
    """one BCE_XOR and one pair on two real operands (worst_case.split_operands): the XOR on the ciphertext with every digit
    at its maximum, b on a boundary of its polynomial, first operand negated; the pair on a uniform a, b on an edge of its
    second gate's window, second operand negated"""
    p = o.params
    q, n = p["q"], o.n
    edge = edge_a(q, p["baseR"], p["dR"], n)
    plan = [(wc.XOR, edge[-3][1], 3 * (q // 8), (1, 0)),
            (wc.pair_word(wc.AND, wc.OR), random_a(q, n, rng, 1)[0][1], wc.gate_window(q, wc.OR)[0], (0, 1))]
    out = []
    for op, a, b, (n0, n1) in plan:
        prep = np.array(list(a) + [b], dtype=np.uint64)
        ct1, ct2 = wc.split_operands(q, prep, n0, n1)
        out.append(("%s b=%d neg=%d%d" % (wc.op_name(op), b, n0, n1), op, ct1, ct2, n0, n1, prep))
    return out


# ---- the key as the restated index reads it ----------------------------------------------------------------------------------
class IndexedKeys(xm._Keys):
    """what xor_single_model.blind_rotate reads of the oracle's key, addressed through key_index() on the flat list of RGSW
    ciphertexts, with a record of the indices read"""

    def __init__(self, o):
        p = o.params
        self.o, self.R, self.N = o, 2 * p["dG"], o.N
        self.baseR, self.dR = p["baseR"], p["dR"]
        self.flat = o.bsk().reshape(rgsw_count(o.n, self.baseR, self.dR), self.R, 2, self.N)
        self.rgsw_, self.mono_, self.read = {}, {}, []

    def rgsw(self, i, a0, k):
        idx = key_index(i, a0, k, self.baseR, self.dR)
        self.read.append(idx)
        if idx not in self.rgsw_:
            self.rgsw_[idx] = np.stack([np.stack([self.o.ntt_forward(self.flat[idx][l][j]) for j in range(2)]) for l in range(self.R)])
        return self.rgsw_[idx]
