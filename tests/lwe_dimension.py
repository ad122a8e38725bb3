"""The LWE dimension n as a test dimension (test helper: plain numpy and Python integers, nothing of the engine).

n decides the row geometry of the key-switch tail -- how many 16-byte groups a key row has, how many waves share a row, how
many row slices a workgroup walks, whether a scalar pass follows -- and the size of the last LDS region of the blind-rotation
kernels.  This module restates those rules in a few lines (TailGeom and its fused_fits of csrc/fused_tail.hpp, as launch_tail,
fused_tail and fused_tail_fits use them, LatLds::bytes, tail_split), names the classes and in-class edges they produce for n = 1 .. N_MAX, and
lists the n the GPU sweep (tests/test_gpu_lwe_dimension.py) runs.  Its CPU half asserts that the lists hit every class and
edge, so a shortened list fails on any machine.

It also builds the operands of the full-bootstrap part of the sweep: ciphertexts whose prepared `a` is non-zero only at the
indices where a loop pass of the prologue or the step loop changes, and bootstrapping keys that are uniform on exactly those
rows and zero elsewhere, made in place.
"""
import numpy as np

import pair_model as pm
import worst_case as wc
import xor_single_model as xm

N_MAX = 1099
WIDTHS = ("u16", "u32")
VW = {"u16": 8, "u32": 4}                   # key elements per 16-byte load
QKS = {"u16": 1 << 14, "u32": 1 << 17}      # rows are u16 while qKS <= 2^16
SEPARATE_CAP, FUSED_CAP = 256, 512          # lanes of the vector pass: k_tail_gather (256 threads), fused tail at T = 512


# ---- the rules, restated -----------------------------------------------------------------------------------------------
def groups(n, vw):
    """16-byte groups that hold elements 0 .. n of a key row"""
    return (n + vw) // vw


def tail_geometry(n, vw, cap):
    """(waves per row RW, row slices SL, elements left to a scalar pass) of a tail with `cap` lanes (cap / 64 waves)"""
    gv = min(groups(n, vw), cap)
    rw = -(-gv // 64)
    return rw, (cap // 64) // rw, max(0, n + 1 - gv * vw)


def separate_class(n, vw):
    """(RW, SL, capped) of k_tail_gather"""
    rw, sl, scalar = tail_geometry(n, vw, SEPARATE_CAP)
    return rw, sl, scalar > 0


def fused_class(n, vw):
    """(RW, SL) of the fused tail at 512 threads; 8 - RW SL trailing waves sit out"""
    return tail_geometry(n, vw, FUSED_CAP)[:2]


def edges(n, vw, cap):
    """the in-class edges n sits on"""
    g = groups(n, vw)
    gv = min(g, cap)
    out = set()
    if g == 1:
        out.add("G = 1")
    if (n + 1) % vw == 0:
        out.add("n + 1 a multiple of VW")
    if (n + 1) % vw == 1:
        out.add("one element into a new group")
    if gv > 1 and gv % 64 == 1:
        out.add("last wave with a single active lane, Gv = %d" % gv)
    return out


# what the formulas give for n = 1 .. N_MAX, as (first n, last n, class): the table the sweep was chosen from
SEPARATE_TABLE = {"u16": [(1, 511, (1, 4, False)), (512, 1023, (2, 2, False)), (1024, N_MAX, (3, 1, False))],
                  "u32": [(1, 255, (1, 4, False)), (256, 511, (2, 2, False)), (512, 767, (3, 1, False)), (768, 1023, (4, 1, False)),
                          (1024, N_MAX, (4, 1, True))]}
FUSED_TABLE = {"u16": [(1, 511, (1, 8)), (512, 1023, (2, 4)), (1024, N_MAX, (3, 2))],
               "u32": [(1, 255, (1, 8)), (256, 511, (2, 4)), (512, 767, (3, 2)), (768, 1023, (4, 2)), (1024, N_MAX, (5, 1))]}


def tail_split(cu, N, boots):
    """workgroups a bootstrap's rows are spread over by the separate tail"""
    s = 1
    while s < 16 and boots * s * 2 <= 4 * cu and N // (s * 2) >= 64:
        s *= 2
    return s


def launch_counts(cu):
    return [1, cu // 4 + 1, cu // 2 + 1, cu + 1, 2 * cu + 1]


LAT_TAIL_BYTES = (8 * 1088 + 4 * 1280) * 4      # LatLds::tail_bytes: digit rows + exchange buffers of the split-transform kernel


def fused_tail_need(n, N, dKS, vw):
    """LDS bytes of the fused tail at 512 threads: row numbers + partial sums"""
    gv = min(groups(n, vw), FUSED_CAP)
    sl = fused_class(n, vw)[1]
    return ((N * dKS + 3) & ~3) * 4 + sl * gv * vw * 8


def fused_tail_fits(n, N, dKS, vw):
    return n + 1 <= FUSED_CAP * vw and fused_class(n, vw)[0] <= 8 and fused_tail_need(n, N, dKS, vw) <= LAT_TAIL_BYTES


LDS_BYTES_PER_CU = 160 * 1024


def lat_lds_bytes(mfma, n):
    """LatLds::bytes: twiddles, accumulator, digit rows, exchange buffers, (matrix-pipe build) byte matrices, then n + 1 words"""
    return (2 * 1024 + 2 * 1088 + 8 * 1088 + 4 * 1280 + (6 * 256 if mfma else 0) + ((n + 1 + 3) & ~3)) * 4


# ---- the sweep's n ---------------------------------------------------------------------------------------------------------
SEPARATE_N = {"u16": (7, 8, 511, 512, 1023, 1024),
              "u32": (3, 4, 255, 256, 511, 512, 767, 768, 1023, 1024, 1025)}
# full bootstraps with the fused tail.  7, 512 (u16) and 3, 1023 (u32) are there for the in-class edges alone: G = 1, the u16
# single-lane wave at Gv = 65 and a u32 row whose last group is full
FUSED_N = {"u16": (7, 511, 512, 1023, 1024),
           "u32": (3, 256, 512, 768, 1023, 1024, 1025)}
ROW_KERNEL_N = tuple(sorted(set(SEPARATE_N["u32"]) | {63, 64, 65, 127, 128, 129}))
KEYGEN_N = (63, 64, 65, 128)


# ---- sparse ciphertexts and keys of the full-bootstrap part ----------------------------------------------------------------
def loop_indices(n):
    """the coefficients at which a loop pass of 512 threads (or of the step loop) begins or ends, below n"""
    return sorted(set(i for i in (0, 511, 512, 1023, n - 1) if 0 <= i < n))


def _subsets(n):
    idx = loop_indices(n)
    mid = [i for i in idx if i in (511, 512)] or idx[:1]
    return {"all": idx, "ends": sorted(set((idx[0], idx[-1]))), "middle": mid, "none": []}


A_VALUES = lambda q: (1, q // 2, q - 1, 2, q // 2 + 1)


def sparse_cases(o):
    """[(name, op, ct1, ct2, neg0, neg1, prep, subset)]: two real operands (worst_case.split_operands) whose prepared sum has
    a non-zero only at `subset`.  Plain gates with b on a window edge and in mid-window, all four negation combinations, one
    BCE_XOR on a boundary of its polynomial, one pair of each kind of exponent below and from N."""
    q, n = o.params["q"], o.n
    sub = _subsets(n)
    plan = [(wc.AND, "all", wc.gate_window(q, wc.AND)[0], (0, 0)),                         # window edge q1
            (wc.OR, "ends", (wc.gate_window(q, wc.OR)[0] + q // 4) % q, (1, 0)),            # mid-window
            (wc.NAND, "middle", (wc.gate_window(q, wc.NAND)[1] - 1) % q, (0, 1)),           # last b inside the window
            (wc.NOR, "none", (wc.gate_window(q, wc.NOR)[1] + q // 4) % q, (1, 1)),          # middle of the complement
            (wc.XOR, "all", 3 * (q // 8), (1, 0)),
            (wc.pair_word(wc.AND, wc.OR), "all", wc.gate_window(q, wc.OR)[0], (0, 1)),      # exponent N / 2
            (wc.pair_word(wc.OR, wc.NOR), "ends", (wc.gate_window(q, wc.NOR)[1] - 1) % q, (1, 1))]   # exponent N
    out = []
    for op, which, b, (n0, n1) in plan:
        prep = np.zeros(n + 1, dtype=np.uint64)
        for k, i in enumerate(sub[which]):
            prep[i] = A_VALUES(q)[(k + len(out)) % 5]
        prep[n] = b
        ct1, ct2 = wc.split_operands(q, prep, n0, n1)
        out.append(("%s a!=0 at %s b=%d neg=%d%d" % (wc.op_name(op), sub[which], b, n0, n1), op, ct1, ct2, n0, n1, prep, sub[which]))
    return out


def sparse_bsk(o, rng):
    """uniform RGSW words on the rows of loop_indices(n), zeros elsewhere (the zero pages are never written)"""
    bsk = np.zeros(wc.bsk_shape(o), dtype=np.uint64)
    for i in loop_indices(o.n):
        bsk[i] = rng.integers(0, o.params["Q"], size=bsk.shape[1:], dtype=np.uint64)
    return bsk


class SparseKeys(xm._Keys):
    """what xor_single_model.blind_rotate reads of a key, served from the evaluation-form words that were imported: the
    oracle's bsk() would transform every row of a key that is zero but for a handful"""

    def __init__(self, o, bsk):
        self.o, self.R, self.N = o, 2 * o.params["dG"], o.N
        self.bsk = bsk
        self.rgsw_, self.mono_ = {}, {}

    def rgsw(self, *idx):
        return self.bsk[idx]


def install(o, c, bsk, ksk):
    """the same key words on the oracle, the numpy blind rotation and (c not None) the engine"""
    s, z = wc.zero_secret(o)
    o.import_keys_eval(s, z, bsk, ksk)
    o._xor_single_keys = SparseKeys(o, bsk)
    if c is not None:
        c.import_keys_eval(s, z, bsk.reshape(-1), ksk.reshape(-1))


def oracle_tail(o, acc):
    lweN = o.extract_modswitch(acc)
    ks = o.keyswitch(lweN)
    return lweN, ks, o.modswitch_final(ks)


def reference(o, case, anchor=False):
    """(accumulator, [(lweN, ks, pool row) per output]) of a sparse case.  The oracle's C blind rotation walks all n
    coefficients (0.7 s at n = 1024), so the accumulator comes from the numpy restatement, which skips a = 0 word for word;
    `anchor` also runs the oracle's own and asserts that the two agree (plain gates and pairs).  The tails are the oracle's."""
    _, op, ct1, ct2, n0, n1, prep, _ = case
    if op == wc.XOR:
        r = xm.stages(o, ct1, ct2, n0, n1)
        return r["acc"], [(r["lweN"], r["ks"], r["out"])]
    first = op & 0xFF
    a, b = (o.eval_not(ct1) if n0 else ct1), (o.eval_not(ct2) if n1 else ct2)
    assert np.array_equal(o.gate_prep(first, a, b), prep)
    acc = xm.blind_rotate(o, xm.plain_poly(o.params, first, int(prep[o.n])), prep)
    if anchor:
        assert np.array_equal(acc, o.blind_rotate(first, prep)), "numpy blind rotation differs from the oracle's"
    outs = [oracle_tail(o, acc)]
    if wc.is_pair(op):
        Q, N, e = o.params["Q"], o.N, pm.exponent(o.params, first, (op >> 8) - 1)
        outs.append(oracle_tail(o, np.concatenate([pm.rotate(acc[:N], e, Q), pm.rotate(acc[N:], e, Q)])))
    return acc, outs


# ---- LWE rows against a known secret ---------------------------------------------------------------------------------------
def phase(q, s, ct):
    """b - <a, s> mod q"""
    ct = np.asarray(ct, dtype=np.int64)
    return int((ct[-1] - int(np.dot(ct[:-1], np.asarray(s, dtype=np.int64)))) % q)


def decision(q, ph):
    """(message Round(4 phase / q) mod 4, as k_lwe_check and bo_decrypt round it: floor(4 (phase + q/8) / q))"""
    return (4 * ((ph + q // 8) % q)) // q


def centred_error(q, ph, expect):
    r = (ph - expect * (q // 4)) % q
    return r - q if r > q // 2 else r


def check_rows(q, s, rng):
    """[(name, row)]: rows whose phase under `s` sits on both sides of every rounding boundary of the decision (phase = k q/8 - 1
    and k q/8, k odd), on both sides of the sign change of the centred error against message 0 (phase q/2, q/2 + 1), a row of
    all q - 1, and the row that is zero but for ones in its last pass of 64 lanes (b included, on lane n % 64)"""
    n = len(s)
    s64 = np.asarray(s, dtype=np.int64)
    rows = []

    def with_phase(name, a, ph):
        row = np.zeros(n + 1, dtype=np.uint64)
        row[:n] = a
        row[n] = (ph + int(np.dot(np.asarray(a, dtype=np.int64), s64))) % q
        assert phase(q, s, row) == ph
        rows.append((name, row))

    for k in (1, 3, 5, 7):
        for d in (1, 0):
            with_phase("phase %dq/8 - %d" % (k, d), rng.integers(0, q, n), k * (q // 8) - d)
    with_phase("phase q/2", rng.integers(0, q, n), q // 2)
    with_phase("phase q/2 + 1", rng.integers(0, q, n), q // 2 + 1)
    rows.append(("all q - 1", np.full(n + 1, q - 1, dtype=np.uint64)))
    last = np.zeros(n + 1, dtype=np.uint64)
    last[64 * (n // 64):] = 1
    rows.append(("ones in the last pass", last))
    return rows
