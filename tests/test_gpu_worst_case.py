"""Worst-case operands: crafted keys, edge ciphertexts and the largest moduli of every kernel class, engine against oracle.

Every other GPU parity test feeds the kernels honest data (fresh encryptions under keygen'd keys), which sits in the middle
of every range the kernels' bound arguments speak about.  Here both sides import the SAME caller-made key words
(tests/worst_case.py) and evaluate the same edge ciphertexts; bce_debug_eval_stages must return the oracle's accumulator,
extract + ModSwitch, KeySwitch and final ciphertext.  Bar: bit for bit at every stage -- the oracle computes with exact
128-bit integers, the engine claims the same residues.  Nothing is decrypted: crafted keys encrypt nothing.

Operand families (one test id each, per kernel class and selector):
  keys     edge ciphertexts (every rotation exponent 0 / N / odd / 2 mod 4 / 0 mod 4 at once, AP digits 0 and baseR - 1,
           b on every window edge, XOR-gate inputs whose doubles wrap mod q onto 0 and q/2) under bootstrapping keys of all Q - 1, all 1, all 0, rows alternating 0 / Q - 1 and
           uniform with forced ends, and key-switching keys of all qKS - 1, all 0 and uniform; export_bsk_eval returns the
           extreme words (fold / un-fold wrap mod Q);
  steered  the first executed step's key is solved so that the accumulator after it is a chosen polynomial pair (digits
           -B/2 and B/2 - 1 in every row, residues round floor(Q/2), evaluation-form words (Q +- 1)/2 and Q - 1); the second
           step multiplies it by a key of all Q - 1 / a uniform key;
  fused    (classes with a fused tail) all descriptors of `keys` and `steered`, and a set steered to the rounding-boundary
           accumulators of `tail`, replicated into one saturated launch: one more fused_tail_launches, every replica equal to
           the small launch at all four stages; both fused tails also with qKS = 2^26 and 2^29;
  tail     bce_debug_tail on accumulators holding both neighbours of every rounding boundary of RoundqQ (including the
           result qKS that wraps to 0), crossed with the three key-switching key patterns; also with qKS = 2^26 and 2^29
           (u32 partial sums folded every 64 / 8 rows).

The CPU half (not marked gpu) asserts on the oracle alone that the operands are what they claim to be.

Every gate here reads the all-zero second input with neg0 = neg1 = 0 and starts from a plain gate's test polynomial.  The
descriptors with two real inputs -- BCE_XOR, BCE_PAIR, the preparation under negations, the persistent kernel -- run on this
file's row table, key families and steering in tests/test_gpu_worst_case_ops.py; _tail_accumulators (an offset) and
_rotated_tail_targets (a pair's second tail) build their tails' boundary accumulators.
"""
import functools

import numpy as np
import pytest

import pair_model as pm
import worst_case as wc

gpu = pytest.mark.gpu
STAGES = ("accumulator", "extract + ModSwitch", "KeySwitch", "final ciphertext")


# ---- moduli ------------------------------------------------------------------------------------------------------------
def _prime_below(L, limit, N):
    """largest prime < limit that is 1 mod 2N"""
    m = 2 * N
    return int(L.bo_previous_prime((limit // m) * m + 1 + (m if limit % m > 1 else 0), m))


def _prime_above(L, p, N):
    """smallest prime > p that is 1 mod 2N"""
    m, x = 2 * N, p + 2 * N
    while int(L.bo_previous_prime(x + m, m)) == p:
        x += m
    return int(L.bo_previous_prime(x + m, m))


def _q27(L, N):
    """the 27-bit prime of the tabulated sets: PreviousPrime(FirstPrime(27, 2N), 2N)"""
    return int(L.bo_previous_prime(L.bo_first_prime(27, 2 * N), 2 * N))


#            n   N     q     Q     qKS      baseKS baseG baseR
def _custom(n, N, q, Q, baseG, qKS=1 << 14, baseKS=32, baseR=32):
    return (n, N, q, Q, qKS, baseKS, baseG, baseR)


def _split_params(L, Q=None, q=1024, n=16, qKS=1 << 14):
    return _custom(n, 1024, q, Q or _q27(L, 1024), 1 << 7, qKS=qKS)


@functools.lru_cache(maxsize=None)
def _mfma_edge(bce_mod, orc_mod, start):
    """largest prime <= start (walking bo_previous_prime down) whose matrix-pipe forward tables pass their bounds"""
    L = orc_mod.lib()
    Q = start
    while bce_mod.forward_mfma_tables(Q)[0] != 1:
        Q = _prime_below(L, Q, 1024)
    return Q


@functools.lru_cache(maxsize=None)
def _lazy_edge(bce_mod, orc_mod):
    """(largest prime = 1 mod 2048 for which the split-transform shape (N = 1024, base 2^7) is granted lazy arithmetic, the
    next prime above it).  Every condition ok1..ok5 of derive_ctx is an upper bound on Q apart from ok3, whose left side
    (sum >> 32) c32 + 2^32 < 2^30 2^28 + 2^32 stays below its right side 2^(32 + red_shift) >= 2^57 in this range, so the
    answer of the accessor is monotone and the walk down from 2^28 is a bisection; the two neighbours are then checked."""
    L = orc_mod.lib()

    def lazy(Q):
        c = bce_mod.BinFHEContext(method=bce_mod.GINX, custom=_split_params(L, Q))
        try:
            return c.lazy_arithmetic()
        finally:
            c.close()

    lo, hi = _q27(L, 1024), _prime_below(L, 1 << 28, 1024)
    assert lazy(lo) == 1 and lazy(hi) == 0
    while True:
        mid = _prime_below(L, (lo + hi) // 2 + 1, 1024)
        if mid <= lo:
            break
        if lazy(mid):
            lo = mid
        else:
            hi = mid
    while True:                      # lo is lazy, hi is not; close the gap prime by prime from above
        below = _prime_below(L, hi, 1024)
        if below == lo:
            break
        if lazy(below):
            lo = below
        else:
            hi = below
    assert lazy(lo) == 1 and _prime_above(L, lo, 1024) == hi and lazy(hi) == 0
    assert _mfma_edge(bce_mod, orc_mod, lo) == lo, "the matrix-pipe tables fail their bounds at the lazy edge"
    print("admission edge of the split-transform class: lazy up to Q = %d, not from Q = %d" % (lo, hi))
    return lo, hi


# ---- the table: one row per kernel class and selector ----------------------------------------------------------------------
class Row:
    def __init__(self, cls, selector, method, params, env=None, fused=0, expect=None):
        self.cls, self.selector, self.method, self.params, self.env = cls, selector, method, params, env or {}
        self.fused = fused          # replicas of the saturated launch (0: the class has no fused tail)
        self.expect = expect or {}  # accessor -> value the context must report
        self.id = "%s-%s-%s" % (cls, selector, "GINX" if method == wc.GINX else "AP")


def _rows():
    G, A = wc.GINX, wc.AP
    R = []
    sp = lambda L, b, o: _split_params(L)
    # split-transform, lazy: N = 1024, base 2^7 (4 digits), q = 1024, the 27-bit prime
    for sel, env, fused, expect in (
            ("default", {}, 300, {"lazy_arithmetic": 1, "forward_mfma": 1}),
            ("variant1", {"BCE_VARIANT": "1"}, 0, {"lazy_arithmetic": 1}),
            ("variant2", {"BCE_VARIANT": "2"}, 0, {}),
            ("variant3_mfma", {"BCE_VARIANT": "3"}, 600, {"forward_mfma": 1, "forward_units": 1}),
            ("variant3_quarters", {"BCE_VARIANT": "3", "BCE_FWD_MFMA": "0"}, 600, {"forward_mfma": 0, "forward_units": 1}),
            ("variant3_old_bodies", {"BCE_VARIANT": "3", "BCE_FWD_UNITS": "0"}, 600, {"forward_units": 0, "forward_transforms_per_step": 6}),
            ("variant3_plain_key", {"BCE_VARIANT": "3", "BCE_FOLD": "0"}, 600, {"forward_transforms_per_step": 8}),
            ("variant2_plain_key", {"BCE_VARIANT": "2", "BCE_FOLD": "0"}, 0, {"forward_transforms_per_step": 8})):
        R.append(Row("split", sel, G, sp, env, fused, expect))
    R.append(Row("split", "q2048_general_mac_tail", G, lambda L, b, o: _split_params(L, q=2048, n=24), {"BCE_VARIANT": "3"}, 600,
                 {"forward_units": 0}))
    R.append(Row("split", "default", A, sp, {}, 300, {"lazy_arithmetic": 1}))
    R.append(Row("split", "variant2", A, sp, {"BCE_VARIANT": "2"}, 0))
    R.append(Row("split", "variant1", A, sp, {"BCE_VARIANT": "1"}, 0))
    # the same class at its admission edges
    lazy_edge = lambda L, b, o: _split_params(L, _lazy_edge(b, o)[0])
    above = lambda L, b, o: _split_params(L, _lazy_edge(b, o)[1])
    # (the matrix-pipe forward body needs the split class; its own table bounds still pass at the lazy edge, so that prime is
    # also the largest with forward_mfma() == 1: asserted by the row's expectations and by _lazy_edge itself)
    R.append(Row("split_lazy_edge", "default", G, lazy_edge, {}, 300, {"lazy_arithmetic": 1, "forward_mfma": 1}))
    R.append(Row("split_lazy_edge", "variant1", G, lazy_edge, {"BCE_VARIANT": "1"}, 0, {"lazy_arithmetic": 1}))
    R.append(Row("split_lazy_edge", "variant3_quarters", G, lazy_edge, {"BCE_VARIANT": "3", "BCE_FWD_MFMA": "0"}, 600, {"forward_mfma": 0, "forward_units": 1}))
    R.append(Row("split_lazy_edge", "default", A, lazy_edge, {}, 300, {"lazy_arithmetic": 1}))
    R.append(Row("above_lazy_edge", "fall_back", G, above, {}, 0, {"lazy_arithmetic": 0, "forward_mfma": 0}))
    R.append(Row("above_lazy_edge", "fall_back", A, above, {}, 0, {"lazy_arithmetic": 0}))
    for m in (G, A):
        # one wave per transform, inexact gadget: TOY's class
        R.append(Row("wave_inexact", "default", m, lambda L, b, o: _custom(16, 512, 512, _q27(L, 512), 1 << 9, baseR=23)))
        # non-lazy 32-bit: the largest prime below 2^28
        R.append(Row("nonlazy32", "default", m, lambda L, b, o: _custom(16, 1024, 1024, _prime_below(L, 1 << 28, 1024), 1 << 10),
                     expect={"lazy_arithmetic": 0}))
        # narrow 64-bit integer: four digits, the largest modulus kernel_class64 admits for the shape (Q < 2^31)
        for N in (1024, 2048):
            R.append(Row("narrow64_N%d" % N, "default", m, lambda L, b, o, N=N: _custom(16, N, 1024, _prime_below(L, 1 << 31, N), 1 << 8),
                         expect={"forward_transforms_per_step": 8}))
        # doubles at the largest prime below 2^39, and the integer 64-bit kernels on the same shapes and below 2^40
        for bits, env, cls in ((39, {}, "fp64"), (39, {"BCE_FP64": "0"}, "int64_39bit"), (40, {}, "int64_40bit")):
            shapes = [(512, 512, 14, "N512_3digits_base14"), (512, 512, 10, "N512_4digits_base10"), (1024, 1024, 14, "N1024_base14"),
                      (2048, 1024, 14, "N2048_base14")]
            if bits == 39:
                shapes += [(512, 512, 13, "N512_base13_inexact"), (1024, 1024, 13, "N1024_base13_inexact"), (2048, 1024, 13, "N2048_base13_inexact")]
            for N, q, gb, name in shapes:
                variants = [("", {})]
                if cls == "fp64" and N == 2048:
                    variants = [("_8waves", {"BCE_VARIANT": "2"}), ("_16waves", {"BCE_VARIANT": "3"})]
                for vname, venv in variants:
                    e = dict(env)
                    e.update(venv)
                    fused = 300 if (cls == "fp64" and N == 2048 and gb == 14 and m == A and vname == "_16waves") else 0
                    # which build ran: the folded key (doubles, N = 2048, exact gadget of base 2^14) transforms 2 dG - 2 rows
                    # per step, every other 64-bit context all 2 dG
                    dG = -(-bits // gb)
                    folded = cls == "fp64" and N == 2048 and gb == 14
                    R.append(Row(cls, name + vname, m, lambda L, b, o, N=N, q=q, gb=gb, bits=bits: _custom(16, N, q, _prime_below(L, 1 << bits, N), 1 << gb),
                                 e, fused, {"forward_transforms_per_step": 2 * dG - 2 if folded else 2 * dG, "lazy_arithmetic": 1}))
    # the doubles class with a fused tail, tail kernels kept separate (BCE_FUSE_TAIL=0)
    R.append(Row("fp64", "N2048_base14_16waves_separate_tail", A,
                 lambda L, b, o: _custom(16, 2048, 1024, _prime_below(L, 1 << 39, 2048), 1 << 14), {"BCE_VARIANT": "3", "BCE_FUSE_TAIL": "0"},
                 expect={"forward_transforms_per_step": 4}))
    return R


ROWS = _rows()
ROW_PARAMS = [pytest.param(r, id=r.id) for r in ROWS]
FUSED_PARAMS = [pytest.param(r, id=r.id) for r in ROWS if r.fused]
# CPU conditions: one row of every parameter shape that needs no GPU to find its modulus
CPU_ROWS = [pytest.param(r, id=r.id) for r in ROWS
            if (r.cls, r.selector) in (("split", "default"), ("split", "q2048_general_mac_tail"), ("wave_inexact", "default"),
                                       ("nonlazy32", "default"), ("narrow64_N1024", "default"), ("fp64", "N512_base13_inexact"),
                                       ("fp64", "N512_3digits_base14"), ("int64_40bit", "N512_3digits_base14"),
                                       ("int64_40bit", "N512_4digits_base10"), ("fp64", "N2048_base14_16waves"))]


def _oracle(orc, row, bce=None):
    return orc.Oracle(method=row.method, custom=row.params(orc.lib(), bce, orc))


def _pair(bce, orc, row, monkeypatch):
    """(oracle, engine context) of a row; a shape the engine refuses fails the test with the engine's message"""
    for k in ("BCE_VARIANT", "BCE_FWD_MFMA", "BCE_FWD_UNITS", "BCE_FOLD", "BCE_FP64", "BCE_FUSE_TAIL", "BCE_OCCUPANCY"):
        monkeypatch.delenv(k, raising=False)
    params = row.params(orc.lib(), bce, orc)        # (may create contexts of its own: before this row's selectors are set)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    o = orc.Oracle(method=row.method, custom=params)
    c = bce.BinFHEContext(method=row.method, custom=params)
    assert o.params == c.params, (o.params, c.params)
    print("context %s: Q = %d (%d bits), N = %d, dG = %d, q = %d, lazy = %d, forward units / mfma = %d / %d, transforms per step = %d"
          % (row.id, c.params["Q"], c.params["Q"].bit_length(), c.N, c.params["dG"], c.params["q"], c.lazy_arithmetic(),
             c.forward_units(), c.forward_mfma(), c.forward_transforms_per_step()))
    for acc, val in row.expect.items():
        assert getattr(c, acc)() == val, "%s() = %d, expected %d" % (acc, getattr(c, acc)(), val)
    return o, c


def _install(o, c, bsk, ksk):
    s, z = wc.zero_secret(o)
    o.import_keys_eval(s, z, bsk, ksk)
    c.import_keys_eval(s, z, bsk.reshape(-1), ksk.reshape(-1))


def _oracle_stages(o, gate, prep):
    acc = o.blind_rotate(gate, prep)
    lweN = o.extract_modswitch(acc)
    ks = o.keyswitch(lweN)
    return acc, lweN, ks, o.modswitch_final(ks)


def _write_inputs(o, c, cases, extra_out=0):
    """slot 0: the all-zero ciphertext; slot 1 + i: ct1 of case i; outputs from 1 + len(cases).  Returns the descriptors."""
    q, nb = o.params["q"], len(cases)
    c.pool_reserve(1 + 2 * nb + extra_out)
    cts = [np.zeros(o.n + 1, dtype=np.uint64)]
    for name, gate, prep, ct1 in cases:
        assert np.array_equal(o.gate_prep(gate, ct1, cts[0]), prep), name
        cts.append(ct1)
    c.lwe_write(np.arange(1 + nb, dtype=np.uint32), np.stack(cts))
    return [(gate, 1 + i, 0, 1 + nb + i) for i, (_, gate, _, _) in enumerate(cases)]


def _run_and_compare(o, c, cases, what):
    """small launch of every case, every stage against the oracle; returns (failures, engine results)"""
    nb = len(cases)
    descs = _write_inputs(o, c, cases)
    acc, lweN, ks = c.debug_eval_stages(descs)
    out = c.lwe_read(np.arange(1 + nb, 1 + 2 * nb, dtype=np.uint32))
    bad = []
    for i, (name, gate, prep, _) in enumerate(cases):
        ref = _oracle_stages(o, gate, prep)
        for stage, got, want in zip(STAGES, (acc[i], lweN[i], ks[i], out[i]), ref):
            if not np.array_equal(got, want):
                k = int(np.flatnonzero(got != want)[0])
                bad.append("%s | %s | %s: %d words differ, first at %d: engine %d, oracle %d"
                           % (what, name, stage, int((got != want).sum()), k, int(got[k]), int(want[k])))
                break
    return bad, (acc, lweN, ks, out)


def _edge(o, subset=False):
    cases = [(name, gate, prep, ct1) for name, gate, prep, _, ct1 in wc.edge_cases(o)]
    return [x for x in cases if not x[0].startswith("window edge")] if subset else cases


KEY_FAMILIES = (("Q-1", "qKS-1", False), ("uniform+forced", "uniform", False), ("1", "0", True), ("0", "uniform", True),
                ("rows 0/Q-1", "qKS-1", True))


# ---- GPU: extreme keys x edge ciphertexts ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_edge_ciphertexts_under_extreme_keys(bce, orc, monkeypatch, row):
    """family `keys`: all edge ciphertexts under keys of all Q - 1 / qKS - 1 and uniform with forced ends, the a patterns
    under all 1, all 0 and alternating rows; every stage equals the oracle's; the extreme words come back from
    export_bsk_eval (a folded key is un-folded mod Q)."""
    o, c = _pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3901)
    bad = []
    for bpat, kpat, subset in KEY_FAMILIES:
        bsk, ksk = wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng)
        _install(o, c, bsk, ksk)
        if bpat in ("Q-1", "uniform+forced"):
            back = c.export_bsk_eval()
            assert np.array_equal(back, bsk.reshape(-1)), "export_bsk_eval does not return the %s key words" % bpat
            assert np.array_equal(c.export_ksk(), ksk.reshape(-1))
        b, _ = _run_and_compare(o, c, _edge(o, subset), "bsk %s, ksk %s" % (bpat, kpat))
        bad += b
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- GPU: steered accumulators ---------------------------------------------------------------------------------------------
def _steered_sets(o, rng):
    """[(what, bsk, cases)]: every target under a second-step key of all Q - 1 and under a uniform one"""
    targets = wc.target_polys(o, rng)
    per = o.n // 2
    out = []
    for second in ("Q-1", "uniform"):
        for lo in range(0, len(targets), per):
            bsk, cases = wc.steered_keys(o, targets[lo:lo + per], second, rng)
            out.append(("steered, second key %s" % second, bsk, cases))
    return out


@gpu
@pytest.mark.parametrize("row", ROW_PARAMS)
def test_steered_accumulator(bce, orc, monkeypatch, row):
    """family `steered`: the accumulator after the first executed step is the chosen pair (asserted on the engine too, through
    the ciphertext that stops after that step); the second step decomposes, transforms and multiplies it."""
    o, c = _pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3902)
    bad = []
    for what, bsk, cases in _steered_sets(o, rng):
        _install(o, c, bsk, wc.extreme_ksk(o, "uniform", rng))
        two = [(name, gate, prep, prep) for name, gate, prep, _, _ in cases]           # steered gates are never XOR: ct1 = prep
        one = [(name + " (first step only)", gate, first, first) for name, gate, _, first, _ in cases]
        b, (acc, _, _, _) = _run_and_compare(o, c, two + one, what)
        bad += b
        for i, (name, _, _, _, want) in enumerate(cases):
            if not np.array_equal(acc[len(two) + i], want):
                bad.append("%s | %s: the engine's accumulator after the first step is not the target" % (what, name))
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- GPU: the same descriptors in one saturated launch (fused tail) --------------------------------------------------------
def _saturated(o, c, cases, replicas, what, small_is_separate):
    nb = len(cases)
    descs = _write_inputs(o, c, cases, extra_out=replicas)
    t0 = c.timing()["fused_tail_launches"]
    small = c.debug_eval_stages(descs)
    small = tuple(np.array(x) for x in small) + (c.lwe_read(np.arange(1 + nb, 1 + 2 * nb, dtype=np.uint32)),)
    t1 = c.timing()["fused_tail_launches"]
    if small_is_separate:
        assert t1 == t0, "the small launch was expected to run the separate tail kernels"
    big = [(descs[i % nb][0], descs[i % nb][1], 0, 1 + 2 * nb + i) for i in range(replicas)]
    acc, lweN, ks = c.debug_eval_stages(big)
    out = c.lwe_read(np.arange(1 + 2 * nb, 1 + 2 * nb + replicas, dtype=np.uint32))
    assert c.timing()["fused_tail_launches"] == t1 + 1, "the saturated launch did not run the tail in its epilogue"
    bad = []
    for i in range(replicas):
        for stage, got, want in zip(STAGES, (acc[i], lweN[i], ks[i], out[i]), (x[i % nb] for x in small)):
            if not np.array_equal(got, want):
                bad.append("%s | replica %d of %s | %s differs from the small launch" % (what, i, cases[i % nb][0], stage))
                break
    for i, (name, gate, prep, _) in enumerate(cases):
        for stage, got, want in zip(STAGES, (x[i] for x in small), _oracle_stages(o, gate, prep)):
            if not np.array_equal(got, want):
                bad.append("%s | %s | %s: small launch differs from the oracle" % (what, name, stage))
                break
    return bad


@gpu
@pytest.mark.parametrize("row", FUSED_PARAMS)
def test_saturated_launch_with_fused_tail(bce, orc, monkeypatch, row):
    """family `fused`: everything the `keys` and `steered` families run in small launches -- the edge ciphertexts under all five
    key patterns, both steered sets (two-step and first-step-only ciphertexts) -- and a steered set whose targets are the
    rounding-boundary accumulators of the `tail` family (the only way to hand the fused epilogue a chosen accumulator),
    replicated into one launch of 300 bootstraps (600 where the two-workgroups-per-CU build is pinned): fused_tail_launches
    goes up by one and every replica equals the small launch (and the oracle) at all four stages."""
    o, c = _pair(bce, orc, row, monkeypatch)
    bad = _fused_family(o, c, row, np.random.default_rng(3903))
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


def _fused_family(o, c, row, rng, key_families=None):
    # small launches keep the separate tail kernels in the split class unless the two-workgroups-per-CU build is pinned
    # (BCE_VARIANT=3 fuses whatever the launch size); the doubles class fuses every launch it may fuse
    separate = row.cls.startswith("split") and row.env.get("BCE_VARIANT") != "3"
    bad = []
    for bpat, kpat, subset in key_families or KEY_FAMILIES:
        _install(o, c, wc.extreme_bsk(o, bpat, rng), wc.extreme_ksk(o, kpat, rng))
        bad += _saturated(o, c, _edge(o, subset), row.fused, "bsk %s, ksk %s" % (bpat, kpat), separate)
    accs = _tail_accumulators(o, rng)
    boundary = [("coeff RoundqQ boundaries %d" % k, "coeff", accs[k]) for k in range(min(len(accs), o.n // 2))]
    sets = _steered_sets(o, rng)
    bsk, cases = wc.steered_keys(o, boundary, "uniform", rng)
    sets.append(("steered to the rounding boundaries", bsk, cases))
    for k, (what, bsk, cases) in enumerate(sets):
        _install(o, c, bsk, wc.extreme_ksk(o, wc.KSK_PATTERNS[k % 3], rng))
        both = [(name, gate, prep, prep) for name, gate, prep, _, _ in cases]
        both += [(name + " (first step only)", gate, first, first) for name, gate, _, first, _ in cases]
        bad += _saturated(o, c, both, row.fused, what, separate)
    return bad


@gpu
@pytest.mark.parametrize("cls", ["split", "fp64_N2048_AP"])
@pytest.mark.parametrize("log_qks", [26, 29])
def test_saturated_launch_fused_tail_large_qks(bce, orc, monkeypatch, log_qks, cls):
    """Both fused tails' multi-chunk key-switch sums: qKS = 2^26 (u32 sums folded every 64 rows) and 2^29 (every 8 rows, the
    smallest admitted chunk), key words all qKS - 1 (the sums reach their bound) and uniform; the steered sets bring the
    rounding-boundary accumulators of these qKS into the epilogue."""
    if cls == "split":
        row = Row("split", "qKS_2^%d" % log_qks, wc.GINX, lambda L, b, o: _split_params(L, qKS=1 << log_qks), {}, 300)
    else:
        row = Row("fp64", "N2048_base14_16waves_qKS_2^%d" % log_qks, wc.AP,
                  lambda L, b, o: _custom(16, 2048, 1024, _prime_below(L, 1 << 39, 2048), 1 << 14, qKS=1 << log_qks), {"BCE_VARIANT": "3"}, 300,
                  {"forward_transforms_per_step": 4})
    o, c = _pair(bce, orc, row, monkeypatch)
    bad = _fused_family(o, c, row, np.random.default_rng(3904), (("uniform+forced", "qKS-1", True), ("Q-1", "uniform", True)))
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- GPU: the class limits the table is built on are the engine's -------------------------------------------------------------
@gpu
def test_class_limits_are_where_the_table_assumes(bce, orc):
    """The rows above take the largest prime below 2^28, 2^31, 2^39 and 2^40.  The first prime ABOVE each limit must leave the
    class (or be refused with BCE_ERR_UNSUPPORTED), so that a drift of a limit in derive_ctx / kernel_class64 shows here."""
    L = orc.lib()

    def ctx(N, q, Q, gb, method=bce.GINX):
        return bce.BinFHEContext(method=method, custom=_custom(16, N, q, Q, 1 << gb))

    def first_above(bits, N):
        Q = int(L.bo_first_prime(bits, 2 * N))
        assert Q > (1 << bits) and _prime_below(L, Q, N) == _prime_below(L, 1 << bits, N)
        return Q

    # 2^28: 32-bit words below, 64-bit words from there on (key bytes per bootstrap double at the same digit count)
    lo, hi = ctx(1024, 1024, _prime_below(L, 1 << 28, 1024), 10), ctx(1024, 1024, first_above(28, 1024), 10)
    assert lo.params["dG"] == hi.params["dG"] == 3
    assert hi.bytes_per_bootstrap_parts()["bsk"] == 2 * lo.bytes_per_bootstrap_parts()["bsk"]
    lo.close(), hi.close()
    # 2^31: four digits on N >= 1024 have the narrow integer build below and no kernel from there on
    for N in (1024, 2048):
        with pytest.raises(bce.BceError) as e:
            ctx(N, 1024, first_above(31, N), 8)
        print("refused: N = %d, Q = %d: %s" % (N, first_above(31, N), e.value))
        assert e.value.code == bce.ERR_UNSUPPORTED
    # 2^39: doubles (folded key at N = 2048, base 2^14: 4 transforms per step) below, the integer kernel (plain key: 6) from there on
    lo, hi = ctx(2048, 1024, _prime_below(L, 1 << 39, 2048), 14, bce.AP), ctx(2048, 1024, first_above(39, 2048), 14, bce.AP)
    assert (lo.forward_transforms_per_step(), hi.forward_transforms_per_step()) == (4, 6)
    lo.close(), hi.close()
    # 2^40: nothing from there on
    for N in (512, 2048):
        with pytest.raises(bce.BceError) as e:
            ctx(N, 512, first_above(40, N), 14)
        print("refused: N = %d, Q = %d: %s" % (N, first_above(40, N), e.value))
        assert e.value.code == bce.ERR_UNSUPPORTED


# ---- GPU: the tail alone on rounding boundaries ----------------------------------------------------------------------------
def _round_boundaries(o, count=64):
    """For `count` values t spread over [0, qKS] (both ends included; t = qKS is the result that wraps to 0): the two v on
    either side of the boundary RoundqQ(v - 1) = t - 1, RoundqQ(v) = t (qKS > Q: RoundqQ(v - 1) < t <= RoundqQ(v)), found by
    bisection on the oracle's own RoundqQ (extract_modswitch of an accumulator whose coefficient 0 is v)."""
    Q, qks, N = o.params["Q"], o.params["qKS"], o.N
    acc = np.zeros(2 * N, dtype=np.uint64)

    def rnd(v):                       # unwrapped: the result qKS of the top residues comes back as 0
        acc[0] = v
        r = int(o.extract_modswitch(acc)[0])
        return qks if (r == 0 and v > Q // 2) else r

    ts = sorted(set([1, 2, qks // 2, qks // 2 + 1, qks - 1, qks] + [int(x) for x in np.linspace(1, qks, count - 6)]))
    vals = []
    for t in ts:
        if rnd(Q - 1) < t:
            continue                  # qKS > Q (the split row with qKS = 2^29): RoundqQ(Q - 1) = qKS - qKS/Q rounded, so the top
                                      # few t -- the wrapping result qKS among them -- have no preimage in that context
        lo, hi = 0, Q - 1             # rnd(lo) < t <= rnd(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if rnd(mid) >= t:
                hi = mid
            else:
                lo = mid
        assert rnd(lo) < t <= rnd(hi)
        if qks <= Q:                  # switching down: consecutive v never skip a result
            assert rnd(lo) == t - 1 and rnd(hi) == t
        vals += [lo, hi]
    return ts, vals


def _tail_accumulators(o, rng, off=None):
    """accumulators [count][2][N] for a tail that extracts b' = acc[1][0] + off (default Q/8 + 1, every gate's; 0: BCE_XOR's):
    component 0 holds the boundary values (directly at coefficient 0, negated elsewhere: the extraction reads a(X^-1)),
    acc[1][0] walks through 0, 1, Q - 1, the two residues round the conditional subtraction of b + off (off > 0), and
    boundary values shifted by -off: with off = 0 the boundary values themselves, both neighbours of the first, the middle
    and the last boundary (the last is the result qKS that wraps to 0 wherever it has a preimage)"""
    Q, N = o.params["Q"], o.N
    off = Q // 8 + 1 if off is None else off
    _, vals = _round_boundaries(o)
    assert len(vals) <= N
    if off:
        b0 = [0, 1, Q - 1, Q - off, Q - off - 1] + [(v - off) % Q for v in (vals[0], vals[1], vals[-2], vals[-1], vals[len(vals) // 2])]
    else:
        mid = 2 * (len(vals) // 4)                  # vals = [below, at] per boundary
        b0 = [0, 1, Q - 1, vals[0], vals[1], vals[mid], vals[mid + 1], vals[-2], vals[-1]]
    accs = rng.integers(0, Q, size=(len(b0), 2, N), dtype=np.uint64)
    for k, b in enumerate(b0):
        rot = vals[k % len(vals):] + vals[:k % len(vals)]
        accs[k, 0, 0] = rot[0]
        for i in range(1, len(rot)):
            accs[k, 0, N - i] = (Q - rot[i]) % Q       # a'_i = -a_{N-i}
        accs[k, 1, 0] = b
    return accs


def _rotated_tail_targets(o, rng, pairs):
    """[(pair word, target, A2)] for a pair's SECOND tail, one per accumulator of _tail_accumulators, the ordered pairs of
    `pairs` in turn: A2 is the boundary accumulator of the default tail with, in component 0, 0 at the wrap index e mod N (the
    word the rotation reads from coefficient 0) and Q - 1 at its neighbour below (read from coefficient N - 1), and 0 and
    Q - 1 at two positions in the middle of the range the rotation negates; the target is X^(2N - e) A2, so that the second
    tail of a pair whose shared accumulator is the target reads A2 itself (and the first tail the target)."""
    Q, N = o.params["Q"], o.N
    out = []
    for k, A2 in enumerate(_tail_accumulators(o, rng)):
        op, op2 = pairs[k % len(pairs)]
        e = pm.exponent(o.params, op, op2)
        lo, hi = (0, e % N) if e < N else (e % N, N)          # positions i of X^e p whose source word is negated
        A2 = A2.copy()
        A2[0, e % N], A2[0, (e - 1) % N] = 0, Q - 1
        A2[0, (lo + hi) // 2], A2[0, (lo + hi) // 2 + 1] = 0, Q - 1
        target = np.stack([pm.rotate(A2[j], (2 * N - e) % (2 * N), Q) for j in range(2)])
        out.append((wc.pair_word(op, op2), target, A2))
    return out


# one ordered pair per distinct rotation exponent N/2, N, 3N/2
EXPONENT_PAIRS = ((wc.AND, wc.OR), (wc.OR, wc.NOR), (wc.OR, wc.AND))


TAIL_ROWS = [pytest.param(r, id=r.id) for r in ROWS if (r.cls, r.selector, r.method) in
             (("split", "default", wc.GINX), ("fp64", "N512_3digits_base14", wc.GINX), ("int64_40bit", "N2048_base14", wc.GINX),
              ("wave_inexact", "default", wc.GINX))]
TAIL_ROWS += [pytest.param(Row("split", "qKS_2^%d_baseKS_%d" % (lg, bk), wc.GINX, lambda L, b, o, lg=lg, bk=bk: _custom(16, 1024, 1024, _q27(L, 1024), 1 << 7, qKS=1 << lg, baseKS=bk)),
                           id="split-qKS_2^%d_baseKS_%d-GINX" % (lg, bk)) for lg, bk in ((26, 32), (29, 32), (16, 16))]
TAIL_ROWS += [pytest.param(Row("fp64", "N512_qKS_2^29", wc.GINX, lambda L, b, o: _custom(16, 512, 512, _prime_below(L, 1 << 39, 512), 1 << 14, qKS=1 << 29)),
                           id="fp64-N512_qKS_2^29-GINX")]


@gpu
@pytest.mark.parametrize("row", TAIL_ROWS)
def test_tail_on_rounding_boundaries(bce, orc, monkeypatch, row):
    """family `tail`: bce_debug_tail (the separate tail kernels) on the boundary accumulators under the three key-switching
    key patterns: extract + ModSwitch, KeySwitch and the final ciphertext equal the oracle's."""
    o, c = _pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(3905)
    accs = _tail_accumulators(o, rng)
    nb = accs.shape[0]
    c.pool_reserve(nb)
    bad = []
    bsk = wc.extreme_bsk(o, "0", rng)
    for kpat in wc.KSK_PATTERNS:
        _install(o, c, bsk, wc.extreme_ksk(o, kpat, rng))
        lweN, ks = c.debug_tail(accs, np.arange(nb, dtype=np.uint32))
        out = c.lwe_read(np.arange(nb, dtype=np.uint32))
        for i in range(nb):
            r_lweN = o.extract_modswitch(accs[i].reshape(-1))
            r_ks = o.keyswitch(r_lweN)
            for stage, got, want in zip(STAGES[1:], (lweN[i], ks[i], out[i]), (r_lweN, r_ks, o.modswitch_final(r_ks))):
                if not np.array_equal(got, want):
                    k = int(np.flatnonzero(got != want)[0])
                    bad.append("ksk %s | accumulator %d | %s: first difference at %d: engine %d, oracle %d"
                               % (kpat, i, stage, k, int(got[k]), int(want[k])))
                    break
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- CPU: the operands are what they claim to be (oracle alone) ------------------------------------------------------------
@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_steered_accumulator_equals_target_and_holds_the_extremes(orc, row):
    """After step one the oracle's accumulator equals the target word for word; over all coefficient-form targets every digit
    row shows both digits digit_extremes() says it can show (-B/2 and B/2 - 1 below the top row), and the listed residues
    (0, 1, floor(Q/2) - 1, floor(Q/2), floor(Q/2) + 1, Q - 2, Q - 1) are there; every crafted word is reduced."""
    o = _oracle(orc, row)
    p = o.params
    Q, gb, dG = p["Q"], int(p["baseG"]).bit_length() - 1, p["dG"]
    rng = np.random.default_rng(3902)
    seen = [set() for _ in range(dG)]
    residues = set()
    for what, bsk, cases in _steered_sets(o, rng):
        assert bsk.dtype == np.uint64 and int(bsk.max()) < Q
        s, z = wc.zero_secret(o)
        o.import_keys_eval(s, z, bsk, wc.extreme_ksk(o, "0", rng))
        for name, gate, prep, first, want in cases:
            assert wc.executed_steps(o, first) == 1 and wc.executed_steps(o, prep) == 2, name
            assert int(prep.max()) < p["q"]
            assert np.array_equal(o.blind_rotate(gate, first), want), "%s: accumulator after step one is not the target" % name
            if name.startswith("coeff"):
                dct = o.signed_digit_decompose(want)
                for r in range(2 * dG):
                    row_digits = dct[r].astype(np.int64)
                    row_digits = np.where(row_digits > Q // 2, row_digits - Q, row_digits)
                    seen[r // 2].update((int(row_digits.min()), int(row_digits.max())))
                residues.update(int(v) for v in want[:32])
    for l, (lo, hi) in enumerate(wc.digit_extremes(Q, gb, dG)):
        assert lo in seen[l] and hi in seen[l], "digit row %d shows %s, can show %d..%d" % (l, sorted(seen[l]), lo, hi)
        if l < dG - 1:
            assert (lo, hi) == (-(1 << gb) // 2, (1 << gb) // 2 - 1)
    assert {0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 2, Q - 1} <= residues
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_signed_digits_match_the_oracle(orc, row):
    """worst_case.signed_digits (Python integers) against the oracle's SignedDigitDecompose on the extreme residues"""
    o = _oracle(orc, row)
    Q, gb, dG = o.params["Q"], int(o.params["baseG"]).bit_length() - 1, o.params["dG"]
    vals = [0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 2, Q - 1, wc.extreme_residue(Q, gb, dG, -1), wc.extreme_residue(Q, gb, dG, +1)]
    ct = np.zeros((2, o.N), dtype=np.uint64)
    ct[0, :len(vals)] = vals
    dct = o.signed_digit_decompose(ct)
    for k, v in enumerate(vals):
        assert [int(dct[2 * l][k]) for l in range(dG)] == [d % Q for d in wc.signed_digits(v, Q, gb, dG)], v
    lo, hi = wc.signed_digits(vals[-2], Q, gb, dG), wc.signed_digits(vals[-1], Q, gb, dG)
    assert all(d == -(1 << gb) // 2 for d in lo[:-1]) and all(d == (1 << gb) // 2 - 1 for d in hi[:-1])
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_edge_ciphertexts_execute_the_steps_they_claim(orc, row):
    """all-zero a: no step; a pattern without a zero: n steps (GINX), one per non-zero digit of -a (AP); the inputs written
    through lwe_write prepare to the pattern (doubled for the XOR gates); every word is reduced."""
    o = _oracle(orc, row)
    p = o.params
    q, n, ap = p["q"], o.n, p["method"] == wc.AP
    pats = dict((name, (a, steps)) for name, a, steps in wc.a_patterns(o))
    assert pats["a=0"][1] == 0
    for name in ("a=q/2", "a=q-1", "a=1", "a=2", "a=q/2+1"):
        a, steps = pats[name]
        if not ap:
            assert steps == n, name
        else:
            assert steps == sum(1 for ds in wc.ap_digits(o, a) for d in ds if d) and steps >= n, name
    assert pats["a=cycle"][1] == (sum(1 for ds in wc.ap_digits(o, pats["a=cycle"][0]) for d in ds if d) if ap else n - len([i for i in range(n) if i % 6 == 0]))
    if ap:
        br, dr = p["baseR"], p["dR"]
        assert pats["-a top digit only"][1] == n and pats["-a low digit baseR-1 only"][1] == n
        assert all(ds == [0] * (dr - 1) + [1] for ds in wc.ap_digits(o, pats["-a top digit only"][0]))
        assert all(ds[:-1] == [br - 1] * (dr - 1) and ds[-1] > 0 for ds in wc.ap_digits(o, pats["-a digits all baseR-1"][0]))
        assert pats["-a digits all baseR-1"][1] == n * dr
    else:
        N = o.N
        exps = set(e % (2 * N) for _, _, prep, _, _ in wc.edge_cases(o) for e in wc.ginx_exponents(o, prep))
        assert 0 in exps and N in exps and any(e % 4 == 0 and e % (2 * N) for e in exps)
        if 2 * N // q <= 2:                      # a factor of 4 makes every exponent 0 mod 4
            assert any(e % 4 == 2 for e in exps)
        if 2 * N // q == 1:
            assert any(e & 1 for e in exps)
    zero = np.zeros(n + 1, dtype=np.uint64)
    names = set()
    xor_half, xor_wrapped_a, xor_wrapped_b, xor_no_step = False, False, False, False
    for name, gate, prep, steps, ct1 in wc.edge_cases(o):
        assert name not in names, "duplicate case " + name
        names.add(name)
        assert int(prep.max()) < q
        assert int(ct1.max()) < q and np.array_equal(o.gate_prep(gate, ct1, zero), prep), name
        assert steps == wc.executed_steps(o, prep)
        if wc.is_xor(gate):
            xor_half |= bool((prep[:n] == q // 2).any())                       # a' = N (GINX), the double of q/4 or 3q/4
            xor_wrapped_a |= bool((ct1[:n] >= q // 2).any())                   # 2 a >= q: the doubling wraps
            xor_wrapped_b |= bool(ct1[n] >= q // 2)
            xor_no_step |= bool(((ct1[:n] == q // 2) & (prep[:n] == 0)).any())  # input q/2 doubles to q = 0
    assert xor_half and xor_wrapped_a and xor_wrapped_b and xor_no_step
    # with a key of all zeros the accumulator of the all-zero a is the test vector itself, untouched by any step
    rng = np.random.default_rng(1)
    s, z = wc.zero_secret(o)
    o.import_keys_eval(s, z, wc.extreme_bsk(o, "uniform+forced", rng), wc.extreme_ksk(o, "0", rng))
    for gate in wc.GATES:
        prep = np.array([0] * n + [wc.b_patterns(q, gate)[3]], dtype=np.uint64)
        acc = o.blind_rotate(gate, prep)
        assert not acc[:o.N].any() and np.array_equal(acc[o.N:], wc.test_vector(o, gate, int(prep[n])))
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS[:3])
def test_cpu_window_edges_move_exactly_one_coefficient(orc, row):
    """b on a window edge and its neighbour b - 1 give test vectors that differ in exactly one coefficient: j (2N/q) with
    b - j = q1 or q2 (mod q), the one index in [0, q/2) at which b - j is on an edge of the window and b - 1 - j is not."""
    o = _oracle(orc, row)
    q, N = o.params["q"], o.N
    f = 2 * N // q
    s, z = wc.zero_secret(o)
    o.import_keys_eval(s, z, wc.extreme_bsk(o, "0", None), wc.extreme_ksk(o, "0", None))
    for gate in wc.GATES:
        q1, q2 = wc.gate_window(q, gate)
        for b in wc.b_patterns(q, gate):
            m, m1 = wc.test_vector(o, gate, b), wc.test_vector(o, gate, (b - 1) % q)
            js = [j for j in ((b - q1) % q, (b - q2) % q) if j < q // 2]
            assert len(js) == 1
            assert list(np.flatnonzero(m != m1)) == [js[0] * f], (gate, b)
            # and the helper's test vector is the oracle's (zero rotation: the accumulator is (0, m))
            prep = np.array([0] * o.n + [b], dtype=np.uint64)
            assert np.array_equal(o.blind_rotate(gate, prep)[N:], m)
    o.close()


@pytest.mark.parametrize("row", CPU_ROWS)
def test_cpu_extreme_keys_are_reduced_and_extreme(orc, row):
    o = _oracle(orc, row)
    Q, qks = o.params["Q"], o.params["qKS"]
    rng = np.random.default_rng(5)
    for pat in wc.BSK_PATTERNS:
        k = wc.extreme_bsk(o, pat, rng)
        assert k.size == o.bsk_words() and int(k.max()) < Q
        if pat != "1" and pat != "0":
            assert int(k.max()) == Q - 1
        if pat == "uniform+forced":
            flat = k.reshape(-1)
            assert (flat[0::16] == Q - 1).all() and (flat[8::16] == 0).all()
        if pat == "rows 0/Q-1":
            rg = k.reshape(-1, 2 * o.params["dG"], 2, o.N)
            assert not rg[:, 0::2].any() and (rg[:, 1::2] == Q - 1).all()
    for pat in wc.KSK_PATTERNS:
        k = wc.extreme_ksk(o, pat, rng)
        assert k.size == o.N * o.params["baseKS"] * o.params["dKS"] * (o.n + 1)
        assert int(k.max()) < qks
    o.close()
