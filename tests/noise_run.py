"""The measurements of the noise tests on a device context: shapes, gate lists, staged and end-level runs.  Shared by
tests/test_gpu_noise.py and tools/noise_report.py.  The context is handed in: nothing of the engine is imported here; the
model and the host-side phase arithmetic are in noise_model.py."""
import numpy as np

from noise_model import AND, NAND, NOR, OR, XNOR_FAST, XOR_FAST, gate_truth, lwe_phase_error, random_gates

def shapes(L, toy):
    """the shapes of the GPU noise tests, each varying an input of the model: id -> (tabulated set or None, custom tuple
    (n, N, q, Q, qKS, baseKS, baseG, baseR) or None, methods).  L: the oracle's library (prime search); toy: the id of TOY."""
    prime = lambda bits, N: int(L.bo_previous_prime(L.bo_first_prime(bits, 2 * N), 2 * N))
    below = lambda limit, N: int(L.bo_previous_prime((limit // (2 * N)) * (2 * N) + 1, 2 * N))
    return {
        "toy": (toy, None, ("GINX", "AP")),                                       # qKS = Q prime, baseKS 25, baseR 23
        "split": (None, (32, 1024, 1024, prime(27, 1024), 1 << 14, 1 << 7, 1 << 7, 32), ("GINX", "AP")),
        "std256_like": (None, (32, 2048, 2048, prime(29, 2048), 1 << 14, 1 << 7, 1 << 8, 46), ("GINX", "AP")),
        "std192_like": (None, (32, 2048, 1024, prime(37, 2048), 1 << 19, 28, 1 << 13, 32), ("AP", "GINX")),
        "int64_40": (None, (16, 1024, 1024, below(1 << 40, 1024), 1 << 14, 1 << 7, 1 << 14, 32), ("GINX",)),
    }


def desc_array(desc_type, op, in0, in1, out):
    """ctypes array of gate descriptors from index arrays (no Python loop)"""
    a = np.zeros((len(op), 6), dtype=np.uint32)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = op, in0, in1, out
    return (desc_type * len(op)).from_buffer(a)


LAUNCH = 8192      # gates per EvalGates / checks per check_slots call of the measurements below


def fresh_inputs(cc, rng, n_in):
    """n_in fresh encryptions of random bits in slots 0 .. n_in - 1 (the context's default encryption state)"""
    bits = rng.integers(0, 2, n_in).astype(np.uint8)
    cc.Encrypt(bits, np.arange(n_in, dtype=np.uint32), mode=0)
    return bits.astype(np.int64)


def stage_run(cc, rng, total=8192, chunk=4096, n_in=1024):
    """`total` bootstraps (the four two-input gates on distinct random pairs of n_in fresh encryptions) through
    debug_eval_stages: phase errors after extract + ModSwitch (under z), KeySwitch and of the output (under s), and the
    number of outputs that decrypt to the wrong bit.  The accumulators come back `chunk` bootstraps at a time."""
    p = cc.params
    s, z = cc.export_sk()
    cc.pool_reserve(n_in + total)
    bits = fresh_inputs(cc, rng, n_in)
    op, in0, in1 = random_gates(rng, total, n_in)
    want = gate_truth(op, bits[in0], bits[in1])
    out = n_in + np.arange(total)
    err = {"N": [], "ks": []}
    for o in range(0, total, chunk):
        sl = slice(o, o + chunk)
        _, lweN, ks = cc.debug_eval_stages([(int(g), int(a), int(b), int(t)) for g, a, b, t in zip(op[sl], in0[sl], in1[sl], out[sl])])
        err["N"].append(lwe_phase_error(lweN, z, p["qKS"], want[sl]))
        err["ks"].append(lwe_phase_error(ks, s, p["qKS"], want[sl]))
    final = cc.lwe_read(out.astype(np.uint32))
    res = {"N": np.concatenate(err["N"]), "ks": np.concatenate(err["ks"]), "out": lwe_phase_error(final, s, p["q"], want)}
    wrong = int((np.asarray(cc.Decrypt(out.astype(np.uint32)), dtype=np.int64) != want).sum())
    return res, wrong


def _level(cc, desc_type, op, in0, in1, out, want):
    """one level of gates in launches of LAUNCH, then its device-side check: the report of check_get()"""
    for o in range(0, len(op), LAUNCH):
        sl = slice(o, o + LAUNCH)
        cc.EvalGates(desc_array(desc_type, op[sl], in0[sl], in1[sl], out[sl]))
    cc.check_reset()
    for o in range(0, len(op), LAUNCH):
        sl = slice(o, o + LAUNCH)
        cc.check_slots(out[sl].astype(np.uint32), want[sl].astype(np.uint8))
    return cc.check_get()[0]


def end_run(cc, desc_type, rng, per_level=32768, n_in=1024):
    """two dependent levels of per_level bootstraps each: level 1 = all six ops on distinct random pairs of n_in fresh
    encryptions, level 2 = the four two-input gates on distinct random pairs of level-1 outputs (XOR_FAST / XNOR_FAST double
    a difference: 8 x the input variance, which bootstrapped inputs do not leave room for).  Returns the two device reports."""
    cc.pool_reserve(n_in + 2 * per_level)
    bits = fresh_inputs(cc, rng, n_in)
    op, in0, in1 = random_gates(rng, per_level, n_in, ops=(OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST))
    want1 = gate_truth(op, bits[in0], bits[in1])
    out1 = n_in + np.arange(per_level)
    rep1 = _level(cc, desc_type, op, in0, in1, out1, want1)
    op, a, b = random_gates(rng, per_level, per_level)
    want2 = gate_truth(op, want1[a], want1[b])
    rep2 = _level(cc, desc_type, op, out1[a], out1[b], out1 + per_level, want2)
    return rep1, rep2
