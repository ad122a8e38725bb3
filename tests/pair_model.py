"""Reference for pair descriptors (BCE_PAIR, include/bce_gpu.h): two gates from one blind rotation, built from the oracle's own
stages.  The second output of a pair is NOT eval_bingate(op2, ...): the gadget decomposition's rounding is not symmetric under
the rotation, so the reference is the oracle's tail applied to the rotated accumulator,

    acc = blind_rotate(op, gate_prep(op, ca, cb));   out2 = modswitch_final(keyswitch(extract_modswitch(X^e acc)))
    e = ((q1 - q1') mod q) (2N / q),  q1 = window constant of op, q1' of op2 (BootstrapGateCore)

with the negacyclic shift done here in numpy.  Nothing of the engine is imported."""
import numpy as np

OR, AND, NOR, NAND = range(4)
GATES = (OR, AND, NOR, NAND)
Q1_EIGHTHS = {OR: 5, AND: 7, NOR: 1, NAND: 3}           # q1 of BootstrapGateCore in units of q / 8
ORDERED_PAIRS = [(a, b) for a in GATES for b in GATES if a != b]
DISTINCT_PAIRS = [(a, b) for a in GATES for b in GATES if a < b]


def PAIR(op, op2):
    """the descriptor word of a pair (the macro BCE_PAIR)"""
    return op | ((op2 + 1) << 8)


def truth(op, a, b):
    return [a | b, a & b, 1 - (a | b), 1 - (a & b)][op]


def exponent(params, op, op2):
    q, N = params["q"], params["N"]
    return (((Q1_EIGHTHS[op] - Q1_EIGHTHS[op2]) * (q // 8)) % q) * (2 * N // q)


def rotate(poly, e, Q):
    """X^e * poly mod (X^N + 1, Q), 0 <= e < 2N: coefficient i is s p[i - e'] for i >= e', -s p[N + i - e'] below"""
    poly = np.asarray(poly, dtype=np.uint64)
    N = poly.size
    neg = lambda v: np.where(v == 0, v, np.uint64(Q) - v)
    r = np.roll(poly, e % N)
    r[:e % N] = neg(r[:e % N])
    return neg(r) if e >= N else r


def stages(o, op, op2, ca, cb, neg0=0, neg1=0):
    """every stage of the pair (op, op2) on the ciphertexts ca, cb (EvalNOT folded in where neg0 / neg1): a dict with the
    shared accumulator and, for both outputs, lweN / ks / out"""
    a = o.eval_not(ca) if neg0 else ca
    b = o.eval_not(cb) if neg1 else cb
    acc = o.blind_rotate(op, o.gate_prep(op, a, b))
    Q, N = o.params["Q"], o.N
    e = exponent(o.params, op, op2)
    acc2 = np.concatenate([rotate(acc[:N], e, Q), rotate(acc[N:], e, Q)])
    res = {"acc": acc, "lweN": [], "ks": [], "out": []}
    for x in (acc, acc2):
        lweN = o.extract_modswitch(x)
        ks = o.keyswitch(lweN)
        res["lweN"].append(lweN)
        res["ks"].append(ks)
        res["out"].append(o.modswitch_final(ks))
    return res


def eval_desc(o, pool, d):
    """one descriptor (op, in0, in1, out, neg0, neg1) of a plan on a pool {slot: ciphertext}, pairs through stages()"""
    op, in0, in1, out, neg0, neg1 = (tuple(d) + (0, 0))[:6]
    if op >> 8:
        r = stages(o, op & 0xFF, (op >> 8) - 1, pool[in0], pool[in1], neg0, neg1)
        pool[out], pool[out + 1] = r["out"]
    else:
        a = o.eval_not(pool[in0]) if neg0 else pool[in0]
        b = o.eval_not(pool[in1]) if neg1 else pool[in1]
        pool[out] = o.eval_bingate(op, a, b)


def xor_shared(o, ca, cb):
    """XOR through the shared spelling: AND(OR(a, b), NAND(a, b)), the first two from one blind rotation"""
    t = stages(o, OR, NAND, ca, cb)["out"]
    return o.eval_bingate(AND, t[0], t[1])
