"""Builders of adversarial operands for the gate-bootstrapping kernels (test helper: plain numpy and Python integers).

Honest keys and ciphertexts are close to uniform, so they sit in the middle of every range the kernels' bound arguments
speak about.  What is built here sits at the ends:

  * edge ciphertexts: every rotation exponent 0, N, odd, 2 mod 4, 0 mod 4 at once; b on the edges of every gate's window;
  * two-operand cases (two_operand_cases): a chosen prepared word vector split into two real inputs under all four
    negation combinations (the second a fixed cycle through 0, 1, q/4, q/2 +- 1, q/2, 3q/4, q - 1, the first solved, so
    that most sums wrap mod q), for BCE_XOR (b on both sides of the four boundaries of its three-level polynomial), all
    12 ordered pairs (b on the window edges of both gates; a = 0: the rotation works on the polynomial itself) and the
    plain gates;
  * extreme keys: every bootstrapping / key-switching key word 0, 1 or the modulus minus one;
  * steered accumulators: the key of the first executed step is SOLVED so that the accumulator after that step is a
    polynomial pair the test chose (digits at -B/2 and B/2 - 1 in every row, residues round floor(Q/2), evaluation-form
    words at (Q +- 1)/2 and Q - 1); the second step then decomposes, transforms and multiplies exactly that pair.  The
    polynomial the blind rotation starts from is the caller's (steered_keys' `poly`): the plain gates' by default.

Crafted keys encrypt nothing.  Both sides (the oracle through import_keys_eval, the engine through import_keys_eval)
evaluate the same function of the same words, and the tests compare them word for word.  All key words are reduced.

`o` is always an oracle.Oracle of the context under test (with or without keys); only its parameter block, its
transforms and its SignedDigitDecompose are used to build operands.
"""
import numpy as np

OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST = range(6)
GATES = (OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST)
GATE_NAMES = ("OR", "AND", "NOR", "NAND", "XOR_FAST", "XNOR_FAST")
AP, GINX = 1, 2


# ---- parameters ------------------------------------------------------------------------------------------------------
def gate_window(q, gate):
    """(q1, q2) of BootstrapGateCore: the window [q1, q2) mod q of the gate's test vector"""
    q1 = (5, 7, 1, 3, 5, 1)[gate] * (q >> 3)
    return q1, (q1 + q // 2) % q


def is_xor(gate):
    return gate in (XOR_FAST, XNOR_FAST)


def bsk_shape(o):
    """the oracle's (and bce_import_keys_eval's) layout: GINX [n][2][R][2][N], AP [n][baseR][dR][R][2][N]"""
    p = o.params
    R = 2 * p["dG"]
    if p["method"] == GINX:
        return (o.n, 2, R, 2, o.N)
    return (o.n, p["baseR"], p["dR"], R, 2, o.N)


def ksk_shape(o):
    p = o.params
    return (o.N, p["baseKS"], p["dKS"], o.n + 1)


# ---- SignedDigitDecompose in Python integers (independent of the oracle's C) -------------------------------------------
def centred(v, Q):
    """the representative SignedDigitDecompose works on: t < floor(Q/2) stays, anything else is t - Q"""
    return v if v < (Q >> 1) else v - Q


def signed_digits(v, Q, gbits, dG):
    """digits r_l in [-B/2, B/2) of the centred residue, lowest first; the carry out of the top digit is dropped"""
    d, B, out = centred(int(v), Q), 1 << gbits, []
    for _ in range(dG):
        r = ((d + B // 2) % B) - B // 2
        out.append(r)
        d = (d - r) >> gbits
    return out


def digit_extremes(Q, gbits, dG):
    """per digit row l: (smallest, largest) digit any residue mod Q can show.  Rows below the top reach -B/2 and B/2 - 1.
    The value that enters the top row is floor((d_l + B/2) / B) applied dG - 1 times, monotone in the centred residue d in
    [-(Q - floor(Q/2)), floor(Q/2)), so it covers a contiguous range; the top digit is that value wrapped into [-B/2, B/2)
    (the dropped carry of an inexact gadget)."""
    B = 1 << gbits

    def enters_top(d):
        for _ in range(dG - 1):
            d = (d + B // 2) >> gbits
        return d

    lo, hi = enters_top(-(Q - (Q >> 1))), enters_top((Q >> 1) - 1)
    if hi - lo + 1 >= B:
        top = (-B // 2, B // 2 - 1)
    else:
        wrapped = [((v + B // 2) % B) - B // 2 for v in range(lo, hi + 1)]
        top = (min(wrapped), max(wrapped))
    return [(-B // 2, B // 2 - 1)] * (dG - 1) + [top]


def extreme_residue(Q, gbits, dG, sign):
    """the residue whose digits are all at -B/2 (sign < 0) or all at B/2 - 1 (sign > 0) in every row that can hold that digit:
    the top digit is moved towards zero until the value is a centred residue mod Q"""
    B = 1 << gbits
    ext = digit_extremes(Q, gbits, dG)
    low = sum(((-B // 2) if sign < 0 else (B // 2 - 1)) * B ** l for l in range(dG - 1))
    top = ext[-1][0] if sign < 0 else ext[-1][1]
    lo, hi = -(Q - (Q >> 1)), (Q >> 1) - 1
    while not (lo <= low + top * B ** (dG - 1) <= hi):
        top -= 1 if top > 0 else -1
    return (low + top * B ** (dG - 1)) % Q


# ---- edge ciphertexts ------------------------------------------------------------------------------------------------
def ginx_exponents(o, prep):
    """rotation exponents a' = (2N/q)(-a mod q) of a prepared ciphertext (GINX)"""
    q = o.params["q"]
    return [((q - int(a)) % q) * (2 * o.N // q) for a in prep[:o.n]]


def ap_digits(o, prep):
    """per coefficient, the base-baseR digits of -a mod q, lowest first (AP: one step per non-zero digit)"""
    q, br, dr = o.params["q"], o.params["baseR"], o.params["dR"]
    out = []
    for a in prep[:o.n]:
        v, ds = (q - int(a)) % q, []
        for _ in range(dr):
            ds.append(v % br)
            v //= br
        out.append(ds)
    return out


def executed_steps(o, prep):
    """AddToAcc steps that change the accumulator: GINX one per a' != 0, AP one per non-zero digit of -a"""
    if o.params["method"] == GINX:
        return sum(1 for e in ginx_exponents(o, prep) if e % (2 * o.N))
    return sum(1 for ds in ap_digits(o, prep) for d in ds if d)


def _ap_value(q, br, dr, digits):
    return (q - sum(d * br ** k for k, d in enumerate(digits)) % q) % q


def a_patterns(o):
    """[(name, a[n], executed steps per coefficient claimed)] of PREPARED a vectors (what the blind rotation sees).
    Steps claimed: GINX 0 or 1 per coefficient, AP the number of non-zero digits of -a."""
    q, n = o.params["q"], o.n
    ap = o.params["method"] == AP
    br, dr = o.params["baseR"], o.params["dR"]

    def steps_of(a):
        if not ap:
            return 0 if a % q == 0 else 1
        v, k = (q - a) % q, 0
        while v:
            k += 1 if v % br else 0
            v //= br
        return k

    pats = [("a=0", [0] * n), ("a=q/2", [q // 2] * n), ("a=q-1", [q - 1] * n), ("a=1", [1] * n),
            ("a=q/2-1", [q // 2 - 1] * n), ("a=q/2+1", [q // 2 + 1] * n), ("a=2", [2] * n),
            ("a=q/4", [q // 4] * n), ("a=3q/4", [3 * q // 4] * n),
            ("a=cycle", [(0, 1, 2, 3, q // 2, q - 1)[i % 6] for i in range(n)])]
    if ap:
        low = [br - 1] * (dr - 1)
        top = min(br - 1, (q - 1 - sum(d * br ** k for k, d in enumerate(low))) // br ** (dr - 1))
        pats += [("-a digits all baseR-1", [_ap_value(q, br, dr, low + [top])] * n),
                 ("-a low digit baseR-1 only", [_ap_value(q, br, dr, [br - 1] + [0] * (dr - 1))] * n),
                 ("-a top digit only", [_ap_value(q, br, dr, [0] * (dr - 1) + [1])] * n),
                 ("-a top digit largest only", [_ap_value(q, br, dr, [0] * (dr - 1) + [(q - 1) // br ** (dr - 1)])] * n)]
    return [(name, a, sum(steps_of(x) for x in a)) for name, a in pats]


def b_patterns(q, gate):
    """prepared b values on the edges of the gate's window and of Z_q"""
    q1, q2 = gate_window(q, gate)
    return [0, q - 1, (q1 - 1) % q, q1, (q2 - 1) % q, q2]


def prepare(q, gate, ct1):
    """gate_prep against the all-zero second input: ct1 itself, 2 ct1 mod q for the XOR gates"""
    ct1 = np.asarray(ct1, dtype=np.uint64)
    return (ct1 * np.uint64(2)) % np.uint64(q) if is_xor(gate) else ct1.copy()


def unprepare(q, gate, prep, lift=None):
    """ct1 with prepare(q, gate, ct1) == prep, or None when prep is not reachable (the XOR gates prepare 2 (ct1 - ct2): odd
    words cannot be reached).  For the XOR gates every prepared word has two inputs, prep / 2 and prep / 2 + q/2; `lift`
    (0 / 1 per word) picks the second one, whose double wraps mod q."""
    prep = np.asarray(prep, dtype=np.uint64)
    if not is_xor(gate):
        return prep.copy()
    if (prep & np.uint64(1)).any():
        return None
    half = prep // np.uint64(2)
    if lift is not None:
        half = half + np.asarray(lift, dtype=np.uint64) * np.uint64(q // 2)
    return half


def edge_cases(o):
    """[(name, gate, prepared ciphertext, executed steps claimed, input ct1)]; the second input of every gate is the all-zero
    ciphertext, so gate_prep leaves ct1 (2 ct1 mod q for the XOR gates).  Three groups:
      * every a pattern, gates in turn, b on a window edge.  Under an XOR gate a pattern of even words is reached through
        prep / 2, with every other word lifted by q/2 (its double wraps); a pattern with odd words is fed as it is and doubled;
      * "xor input": both XOR gates on INPUT patterns q/4, 3q/4 (double q/2: a' = N), q/2 (double q, wraps to 0: no step),
        q/2 + 1, q - 1 and a cycle through them, with an input b >= q/2 whose double wraps onto a window edge;
      * "window edge": for every gate, every window-edge b under the cycle pattern (XOR gates: the even edges and their even
        neighbours, alternately through b / 2 and b / 2 + q/2)."""
    q, n = o.params["q"], o.n
    pats = a_patterns(o)
    out = []

    def add(name, gate, ct1):
        ct1 = np.asarray(ct1, dtype=np.uint64)
        prep = prepare(q, gate, ct1)
        out.append((name, gate, prep, executed_steps(o, prep), ct1))

    alternate = np.arange(n + 1) % 2
    k = 0
    for name, a, steps in pats:
        for gate in (GATES[k % 6], GATES[(k + 4) % 6] if k % 3 == 0 else None):
            if gate is None:
                continue
            b = b_patterns(q, gate)[(k + 2) % 6]
            prep = np.array(list(a) + [b], dtype=np.uint64)
            nm = "%s b=%d %s" % (name, b, GATE_NAMES[gate])
            ct1 = unprepare(q, gate, prep, alternate)
            if ct1 is None:
                ct1, nm = prep, "2x(" + nm + ")"
            add(nm, gate, ct1)
        k += 1
    xin = [("q/4", [q // 4] * n), ("3q/4", [3 * q // 4] * n), ("q/2", [q // 2] * n), ("q/2+1", [q // 2 + 1] * n), ("q-1", [q - 1] * n),
           ("cycle", [(0, q // 4, q // 2, 3 * q // 4, q // 2 + 1, q - 1)[i % 6] for i in range(n)])]
    for gate in (XOR_FAST, XNOR_FAST):
        edges = [e for e in b_patterns(q, gate) if e % 2 == 0]
        for t, (name, a) in enumerate(xin):
            b_in = edges[t % len(edges)] // 2 + q // 2
            add("xor input a=%s b=%d %s" % (name, b_in, GATE_NAMES[gate]), gate, list(a) + [b_in])
    cyc = dict((nm, a) for nm, a, _ in pats)["a=cycle"]
    for gate in GATES:
        bs = b_patterns(q, gate) + ([(gate_window(q, gate)[0] - 2) % q, (gate_window(q, gate)[1] - 2) % q] if is_xor(gate) else [])
        for t, b in enumerate(bs):
            if is_xor(gate):
                if b & 1:
                    continue                     # not reachable through 2 (ct1 - ct2); the even neighbours are listed
                ct1 = np.array(list(cyc) + [b // 2 + (t % 2) * (q // 2)], dtype=np.uint64)
            else:
                ct1 = np.array(list(cyc) + [b], dtype=np.uint64)
            add("window edge b=%d %s (a=cycle)" % (int(prepare(q, gate, ct1)[n]), GATE_NAMES[gate]), gate, ct1)
    return out


def test_vector(o, gate, b):
    """the test vector m of BootstrapGateCore for a prepared b, coefficient form: +-(Q/8 + 1) at the multiples of 2N/q"""
    q, Q, N = o.params["q"], o.params["Q"], o.N
    q1, q2 = gate_window(q, gate)
    f = 2 * N // q
    m = np.zeros(N, dtype=np.uint64)
    pos, neg = Q // 8 + 1, Q - (Q // 8 + 1)
    for j in range(q // 2):
        t = (b - j) % q
        if q1 < q2:
            m[j * f] = neg if q1 <= t < q2 else pos
        else:
            m[j * f] = pos if q2 <= t < q1 else neg
    return m


# ---- two real operands: BCE_XOR, pairs, the preparation itself -------------------------------------------------------------
XOR = 0x10006                                         # BCE_XOR (include/bce_gpu.h)
PLAIN = (OR, AND, NOR, NAND)
ORDERED_PAIRS = [(a, b) for a in PLAIN for b in PLAIN if a != b]
NEGATIONS = ((0, 0), (1, 0), (0, 1), (1, 1))
SWEEP = "sweep: "                                    # name prefix of the per-boundary b sweep (left out of the subset)


def pair_word(op, op2):
    """the descriptor word of a pair (the macro BCE_PAIR)"""
    return op | ((op2 + 1) << 8)


def is_pair(op):
    return op != XOR and (op >> 8) != 0


def op_name(op):
    if op == XOR:
        return "XOR"
    return "PAIR(%s,%s)" % (GATE_NAMES[op & 0xFF], GATE_NAMES[(op >> 8) - 1]) if is_pair(op) else GATE_NAMES[op]


def xor_b_values(q):
    """prepared b of BCE_XOR on the ends of Z_q and on both sides of its four window boundaries k q/8, k = 1, 3, 5, 7"""
    e = q // 8
    return [0, q - 1] + [k * e - d for k in (1, 3, 5, 7) for d in (1, 0)]


def op_b_values(q, op):
    """the window-edge b values of any descriptor word (a pair rotates its first gate's polynomial)"""
    return xor_b_values(q) if op == XOR else b_patterns(q, op & 0xFF)


def lwe_not(q, ct):
    """EvalNOT: (-a, q/4 - b); its own inverse"""
    ct = np.asarray(ct, dtype=np.uint64)
    out = (np.uint64(q) - ct) % np.uint64(q)
    out[-1] = (q // 4 + q - int(ct[-1])) % q
    return out


def second_operand(q, n):
    """the fixed second input: a cycle through 0, 1, q/4, q/2 - 1, q/2, q/2 + 1, 3q/4, q - 1, the b word >= q/2"""
    cyc = (0, 1, q // 4, q // 2 - 1, q // 2, q // 2 + 1, 3 * q // 4, q - 1)
    ct2 = np.array([cyc[(i + 1) % 8] for i in range(n + 1)], dtype=np.uint64)
    ct2[n] = cyc[4 + n % 4]
    return ct2


def split_operands(q, prep, neg0, neg1):
    """(ct1, ct2) with ct1' + ct2' = prep mod q word for word, x' = EvalNOT(x) where the flag is set: ct2 is second_operand,
    ct1 is solved"""
    prep = np.asarray(prep, dtype=np.uint64)
    ct2 = second_operand(q, prep.size - 1)
    eff2 = lwe_not(q, ct2) if neg1 else ct2
    eff1 = (prep + np.uint64(q) - eff2) % np.uint64(q)
    return (lwe_not(q, eff1) if neg0 else eff1), ct2


def wrapped_sums(q, ct1, ct2, neg0, neg1):
    """how many of the n + 1 word sums ct1' + ct2' reach q (and are reduced)"""
    a = lwe_not(q, ct1) if neg0 else np.asarray(ct1, dtype=np.uint64)
    b = lwe_not(q, ct2) if neg1 else np.asarray(ct2, dtype=np.uint64)
    return int(((a + b) >= np.uint64(q)).sum())


def two_operand_cases(o):
    """[(name, op, ct1, ct2, neg0, neg1, prep)]: op is BCE_XOR, a pair word or a plain gate; prep is the sum of the (negated)
    operands, chosen first and split by split_operands; the four (neg0, neg1) combinations rotate over the cases.
      * BCE_XOR: every a pattern with one of the ten b values of xor_b_values in turn, and (SWEEP) with the one five further;
        then (SWEEP) all ten under a=cycle;
      * pairs: all 12 ordered pairs, a=0 (no step: the rotation works on the first gate's polynomial itself) with b next to an
        edge, a=cycle with b on the first edge of op, then (SWEEP) on every other window edge of op and of op2;
      * the four plain gates under every negation combination, b on a window edge, a=cycle: the preparation alone."""
    q, n = o.params["q"], o.n
    pats = a_patterns(o)
    cyc = dict((nm, a) for nm, a, _ in pats)["a=cycle"]
    out = []

    def add(name, op, a, b):
        neg0, neg1 = NEGATIONS[len(out) % 4]
        prep = np.array(list(a) + [b], dtype=np.uint64)
        ct1, ct2 = split_operands(q, prep, neg0, neg1)
        out.append(("%s%s b=%d %s neg=%d%d" % (name[0], name[1], b, op_name(op), neg0, neg1), op, ct1, ct2, neg0, neg1, prep))

    xb = xor_b_values(q)
    for k, (name, a, _) in enumerate(pats):
        add(("", name), XOR, a, xb[k % 10])
        add((SWEEP, name), XOR, a, xb[(k + 5) % 10])
    for b in xb:
        add((SWEEP, "a=cycle"), XOR, cyc, b)
    for k, (op, op2) in enumerate(ORDERED_PAIRS):
        w = pair_word(op, op2)
        edges = []
        for e in gate_window(q, op) + gate_window(q, op2):
            if e not in edges:
                edges.append(e)
        add(("", "a=0"), w, [0] * n, (edges[k % len(edges)] - 1) % q)
        for t, b in enumerate(edges):
            add((SWEEP if t else "", "a=cycle"), w, cyc, b)
    for gate in PLAIN:
        for t in range(4):
            add(("", "a=cycle"), gate, cyc, b_patterns(q, gate)[2 + (gate + t) % 4])
    return out


def operand_subset(cases):
    """the cases without the per-boundary b sweeps"""
    return [x for x in cases if not x[0].startswith(SWEEP)]


# ---- extreme keys ----------------------------------------------------------------------------------------------------
BSK_PATTERNS = ("Q-1", "1", "0", "rows 0/Q-1", "uniform+forced")
KSK_PATTERNS = ("qKS-1", "0", "uniform")


def extreme_bsk(o, pattern, rng):
    Q = o.params["Q"]
    shape = bsk_shape(o)
    if pattern == "Q-1":
        return np.full(shape, Q - 1, dtype=np.uint64)
    if pattern == "1":
        return np.ones(shape, dtype=np.uint64)
    if pattern == "0":
        return np.zeros(shape, dtype=np.uint64)
    if pattern == "rows 0/Q-1":
        k = np.zeros(shape, dtype=np.uint64)
        k[..., 1::2, :, :] = Q - 1           # RGSW rows (digit l, component j) = 2l + j: the odd rows
        return k
    if pattern == "uniform+forced":
        k = rng.integers(0, Q, size=shape, dtype=np.uint64)
        flat = k.reshape(-1)
        flat[0::16] = Q - 1                   # one word in eight at an end of the range
        flat[8::16] = 0
        return k
    raise ValueError(pattern)


def extreme_ksk(o, pattern, rng):
    qks = o.params["qKS"]
    shape = ksk_shape(o)
    if pattern == "qKS-1":
        return np.full(shape, qks - 1, dtype=np.uint32)
    if pattern == "0":
        return np.zeros(shape, dtype=np.uint32)
    if pattern == "uniform":
        return rng.integers(0, qks, size=shape, dtype=np.uint32)
    raise ValueError(pattern)


def zero_secret(o):
    """crafted keys encrypt nothing; the secrets only have to be well-formed"""
    return np.zeros(o.n, dtype=np.int32), np.zeros(o.N, dtype=np.int32)


# ---- steered accumulator ---------------------------------------------------------------------------------------------
def _inv_many(vals, Q):
    """modular inverses of Python ints (Q prime), one exponentiation for the whole list (Montgomery's trick)"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % Q
    inv = pow(acc, Q - 2, Q)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % Q
        inv = inv * vals[i] % Q
    return out


def target_polys(o, rng):
    """[(name, form, pair)]: the accumulators the first step is steered to.  form 'coeff': pair [2][N] is the coefficient-form
    accumulator; form 'eval': pair is the evaluation-form accumulator itself."""
    Q, N, gb, dG = o.params["Q"], o.N, int(o.params["baseG"]).bit_length() - 1, o.params["dG"]
    B = 1 << gb
    hi = sum((B // 2 - 1) * B ** l for l in range(dG))
    lo = sum((B // 2) * B ** l for l in range(dG))
    h = Q >> 1
    lead = [0, 1, h - 1, h, h + 1, Q - 2, Q - 1, hi % Q, (hi + 1) % Q, (hi - 1) % Q, (-lo) % Q, (-lo + 1) % Q, (-lo - 1) % Q,
            extreme_residue(Q, gb, dG, -1), extreme_residue(Q, gb, dG, +1)]
    # every row's own extremes on some coefficient: digit l at an end, the others zero
    ext = digit_extremes(Q, gb, dG)
    for l in range(dG):
        for e in ext[l]:
            lead.append((e * B ** l) % Q)
    edges = rng.integers(0, Q, size=(2, N), dtype=np.uint64)
    for j in range(2):
        vals = lead if j == 0 else lead[::-1]
        edges[j, :len(vals)] = np.array(vals, dtype=np.uint64)
        edges[j, N - len(vals):] = np.array(vals, dtype=np.uint64)
    out = [("coeff edges", "coeff", edges),
           ("coeff all digits -B/2", "coeff", np.full((2, N), extreme_residue(Q, gb, dG, -1), dtype=np.uint64)),
           ("coeff all digits B/2-1", "coeff", np.full((2, N), extreme_residue(Q, gb, dG, +1), dtype=np.uint64)),
           ("eval (Q-1)/2", "eval", np.full((2, N), (Q - 1) // 2, dtype=np.uint64)),
           ("eval (Q+1)/2", "eval", np.full((2, N), (Q + 1) // 2, dtype=np.uint64)),
           ("eval Q-1", "eval", np.full((2, N), Q - 1, dtype=np.uint64))]
    alt = np.full((2, N), Q - 1, dtype=np.uint64)
    alt[:, 1::2] = (Q + 1) // 2
    out.append(("eval alternating Q-1,(Q+1)/2", "eval", alt))
    out.append(("coeff uniform", "coeff", rng.integers(0, Q, size=(2, N), dtype=np.uint64)))
    return out


def _eval_pair(o, form, pair):
    if form == "eval":
        return np.array(pair, dtype=np.uint64)
    return np.stack([o.ntt_forward(pair[0]), o.ntt_forward(pair[1])])


def _coeff_pair(o, form, pair):
    if form == "coeff":
        return np.array(pair, dtype=np.uint64)
    return np.stack([o.ntt_inverse(pair[0]), o.ntt_inverse(pair[1])])


def _solve_rows(o, m, E, mono):
    """RGSW rows [R][2][N] of the first executed step: sum_r D_r(k) rows[r][j][k] * mono(k) = E_j(k) - acc0_j(k) for every
    evaluation point k, where D_r = NTT(digit row r of the accumulator (0, m)), acc0 = (0, NTT(m)) for GINX (mono = NTT(X^a' - 1):
    the step ADDS) and acc0 = 0, mono = 1 for AP (the step REPLACES).  One row per point carries the whole word; the rows
    take turns.  None when some point has no non-zero D_r(k) (the caller picks another b)."""
    Q, N, dG = o.params["Q"], o.N, o.params["dG"]
    R = 2 * dG
    D = o.signed_digit_decompose(np.stack([np.zeros(N, dtype=np.uint64), m]))
    D = np.stack([o.ntt_forward(D[r]) for r in range(R)])
    if mono is None:
        T = [[int(v) for v in E[j]] for j in range(2)]
        mono = [1] * N
    else:
        m_ev = o.ntt_forward(m)
        T = [[int(v) for v in E[0]], [(int(E[1][k]) - int(m_ev[k])) % Q for k in range(N)]]
        mono = [int(v) for v in mono]
    rows = np.zeros((R, 2, N), dtype=np.uint64)
    pick, den = [], []
    for k in range(N):
        cand = [r for r in range(R) if D[r][k] != 0]
        if not cand or mono[k] == 0:
            return None
        r = cand[k % len(cand)]
        pick.append(r)
        den.append(int(D[r][k]) * mono[k] % Q)
    inv = _inv_many(den, Q)
    for k in range(N):
        for j in range(2):
            rows[pick[k], j, k] = T[j][k] * inv[k] % Q
    return rows


def steered_keys(o, targets, second, rng, gates=(AND, OR, NAND, NOR), poly=None):
    """One key set steering one ciphertext per target.  Returns (bsk, cases): cases = [(name, gate, prepared ciphertext,
    first-step-only prepared ciphertext, expected coefficient-form accumulator after the first step)].
    `poly` (o, op, b) -> m makes the test polynomial the blind rotation of `op` starts from (default: test_vector, the plain
    gates' own); `gates` may then hold any descriptor word: target t is steered under gates[t % len(gates)].
    GINX: ciphertext t has a[2t] and a[2t+1] non-zero only; the keys of coefficient 2t are solved (ek+; ek- = 0), those of
    2t+1 are the `second` pattern ('Q-1' or 'uniform').  AP: -a[2t] has two non-zero digits; the key of its low digit is
    solved, the key of its next digit is the `second` pattern.  The first-step-only ciphertext drops the second step."""
    p = o.params
    q, Q, N, n = p["q"], p["Q"], o.N, o.n
    ginx = p["method"] == GINX
    assert len(targets) <= n // 2
    bsk = np.zeros(bsk_shape(o), dtype=np.uint64)
    R = 2 * p["dG"]

    def second_rows():
        if second == "Q-1":
            return np.full((R, 2, N), Q - 1, dtype=np.uint64)
        return rng.integers(0, Q, size=(R, 2, N), dtype=np.uint64)

    firsts = [1, q // 2, q - 1, 2, q // 2 + 1, 3 * q // 4, q // 2 - 1, q // 4, 3, q - 2, q // 2 + 2, 5]
    cases = []
    for t, (name, form, pair) in enumerate(targets):
        gate = gates[t % len(gates)]
        E = _eval_pair(o, form, pair)
        a1 = firsts[t % len(firsts)]
        a2 = firsts[(t + 5) % len(firsts)]
        if 2 * N // q == 1 and t % 2 == 0:
            a1 |= 1                              # odd exponents where the context has them
        rows, tries = None, 0
        while rows is None:
            cand = op_b_values(q, gate)
            b = (cand[(t + tries) % len(cand)] + tries // len(cand)) % q
            m = (poly or test_vector)(o, gate, b)
            if ginx:
                e1 = ((q - a1) % q) * (2 * N // q)
                x = np.zeros(N, dtype=np.uint64)
                x[e1 % N] = 1 if e1 < N else Q - 1
                x[0] = (int(x[0]) + Q - 1) % Q
                rows = _solve_rows(o, m, E, o.ntt_forward(x))
            else:
                rows = _solve_rows(o, m, E, None)
            tries += 1
            assert tries < len(cand) * q, "no b gives a first step that can be steered (%s)" % name
        prep = np.zeros(n + 1, dtype=np.uint64)
        prep[n] = b
        first_only = prep.copy()
        if ginx:
            prep[2 * t], prep[2 * t + 1] = a1, a2
            first_only[2 * t] = a1
            bsk[2 * t, 0] = rows
            bsk[2 * t + 1, 0] = second_rows()
            bsk[2 * t + 1, 1] = second_rows()
        else:
            br = p["baseR"]
            d0, d1 = 1 + a1 % (br - 1), 1 + a2 % min(br - 1, (q - br) // br)     # d0 + d1 baseR < q
            prep[2 * t] = (q - (d0 + d1 * br)) % q
            first_only[2 * t] = (q - d0) % q
            bsk[2 * t, d0, 0] = rows
            bsk[2 * t, d1, 1] = second_rows()
        cases.append((name, gate, prep, first_only, _coeff_pair(o, "eval", E).reshape(-1)))
    return bsk, cases
