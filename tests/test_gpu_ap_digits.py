"""AP digit-geometry sweep: key generation and every AP step-decode site at dR = 1, 3, 7 and 10.

Every other bit-exact test of the AP method runs at dR = 2 digits per LWE coefficient with baseR in {23, 32, 46}: what the
parameter table gives.  baseR and dR decide how many steps a blind rotation has (n dR), which RGSW ciphertext a step reads
((i baseR + a0) dR + k), which exponents key generation encrypts (s_i v baseR^k 2N/q) and how large the key is.  The index
arithmetic lives in four kernel bodies (k_blind_rotate, lat_bootstrap, k_blind_rotate64, bootstrap64d).  tests/ap_digits.py
restates the rules, names the classes of (q, baseR) and assigns to every AP build of the four bodies one geometry with dR = 1
and one with dR >= 3, so that every body sees every class.  Per context, bit for bit against the oracle:

  params    dR included;
  keys      KeyGen(seed): every word of export_bsk / export_ksk (k_gen_bsk_rows with its v baseR^k exponents, the v = 0 rows
            it skips, for baseR > q the rows v >= q that no step reads);
  steps     the edge ciphertexts of ap_digits.edge_a (a = 0; one non-zero digit at every position; every digit at its
            maximum; -a = q - 1; -a = 1) and four uniform ones through bce_debug_eval_stages: accumulator, extract +
            ModSwitch, KeySwitch and the pool row;
  two real  one BCE_XOR and one BCE_PAIR descriptor (references: xor_single_model, pair_model);
  dataflow  a small DAG on k_bootstrap_dag at dR = 1 and dR = 10 and on k_bootstrap_dag64 at dR = 1, against the references and
            the frontier path.

Keys are honest, the ciphertexts' masks are chosen, so what a gate decrypts to means nothing and nothing is decrypted (at
q = 128 and 256 the noise of a bootstrap would not leave a bit anyway).  The CPU half (not marked gpu) asserts that the table
hits every class on every body and every build, that no key passes 250 MB, and, on the oracle alone, that the edge ciphertexts
execute the steps they claim and read the key indices the restated formula gives.
"""
import numpy as np
import pytest

import ap_digits as ad
import test_gpu_worst_case as base
import test_gpu_worst_case_ops as ops
import worst_case as wc
import xor_single_model as xm

gpu = pytest.mark.gpu
Row = base.Row


def _modulus(L, mod, N):
    return base._q27(L, N) if mod == "q27" else base._prime_below(L, 1 << mod, N)


def _row(ctx):
    site, build, g, N, gb, mod, env, expect, (n, q, baseR) = ctx
    params = lambda L, b, o: base._custom(n, N, q, _modulus(L, mod, N), 1 << gb, baseR=baseR)
    r = Row(site, "%s-%s_q%d_baseR%d_n%d" % (build, g, q, baseR, n), wc.AP, params, env, expect=expect)
    r.geometry = g
    return r


ROWS = [_row(x) for x in ad.contexts()]
DAG_ROWS = [_row(x) for x in ad.contexts(ad.DAG_BUILDS)]
ids = lambda rows: [pytest.param(r, id=r.id) for r in rows]
# one oracle context per geometry for the CPU half: the smallest ring that has it, 27-bit prime
CPU_CONTEXTS = [pytest.param(g, min(by_N), id="%s_N%d_q%d_baseR%d" % ((g, min(by_N)) + by_N[min(by_N)])) for g, by_N in ad.GEOMETRIES.items()]


# ---- CPU half ------------------------------------------------------------------------------------------------------------------
def test_cpu_restated_rules_and_classes():
    """digit counts of the table and of the tabulated sets; every geometry is in the class it stands for on every ring"""
    assert [ad.digit_count(q, b) for q, b in ((512, 512), (256, 256), (128, 128), (256, 300), (128, 150), (512, 8), (1024, 23), (2048, 45), (1024, 2), (1024, 3))] \
        == [1, 1, 1, 1, 1, 3, 3, 3, 10, 7]
    assert [ad.digit_count(q, b) for q, b in ((512, 23), (1024, 32), (2048, 46))] == [2, 2, 2]      # the table: the other suites
    assert ad.classify(1024, 32) is None
    for g, by_N in ad.GEOMETRIES.items():
        for N, (q, baseR) in by_N.items():
            assert q & (q - 1) == 0 and 8 <= q <= 2 * N, (g, N)
            assert ad.classify(q, baseR) == ad.GEOMETRY_CLASS[g] and ad.digit_count(q, baseR) == ad.DR[g], (g, N)
            dR = ad.DR[g]
            assert baseR ** dR >= q > (baseR ** (dR - 1) if dR > 1 else 0)
            top = ad.digit_max(q, baseR, dR, dR - 1)
            assert ad.digits(q, baseR, dR, 1)[-1] == top                                   # -a = q - 1 shows it
            if g == "A" or g == "C":
                assert top == baseR - 1
            elif g == "B":
                assert top == q - 1 < baseR - 1
            else:
                assert top == 1 < baseR or baseR == 2
    assert ad.key_index(0, 1, 0, 32, 2) == 2 and ad.key_index(3, 31, 1, 32, 2) == ad.rgsw_count(4, 32, 2) - 1
    assert ad.bsk_words(503, 1024, 4, 32, 2) * 4 == 503 * (1 << 22)                           # STD128_OPT / AP: 4 MiB per coefficient


def test_cpu_table_hits_every_class_on_every_body_and_every_build():
    ctxs = ad.contexts()
    assert {x[0] for x in ctxs} == set(ad.SITES)
    for site in ad.SITES:
        assert {ad.GEOMETRY_CLASS[x[2]] for x in ctxs if x[0] == site} == set(ad.CLASSES), site
    for site, build, _, _, _, _, _, geoms in ad.BUILDS:
        drs = sorted(ad.DR[g] for g in geoms)
        assert drs[0] == 1 and drs[-1] >= 3, (site, build)
    assert sorted(ad.DR[g] for g in ad.DAG_BUILDS[0][7]) == [1, 10] and ad.DAG_BUILDS[1][7] == ("A",)
    # what the builds are: every (logN, dG) of the wave and integer bodies, every AP entry of the split and doubles tables
    shape = lambda site: sorted({(x[3], ad.gadget_digits(x[5], x[4])) for x in ctxs if x[0] == site})
    assert shape("wave32") == [(512, 3), (512, 4), (1024, 3), (1024, 4), (2048, 3)]
    assert shape("split") == [(1024, 4)]
    assert shape("int64") == [(512, 3), (512, 4), (1024, 3), (1024, 4), (2048, 3), (2048, 4)]
    assert shape("fp64") == [(512, 3), (512, 4), (1024, 3), (2048, 3)]
    envs = lambda site: {tuple(sorted(x[6].items())) for x in ctxs if x[0] == site}
    assert {(("BCE_OCCUPANCY", "2"),), (("BCE_VARIANT", "1"),)} < envs("wave32")
    assert envs("split") == {(("BCE_VARIANT", "2"),), (("BCE_FOLD", "0"), ("BCE_VARIANT", "2")), (("BCE_VARIANT", "3"),),
                             (("BCE_FOLD", "0"), ("BCE_VARIANT", "3")), (("BCE_FUSE_TAIL", "0"), ("BCE_VARIANT", "3"))}
    assert len([x for x in ctxs if x[0] == "fp64" and x[3] == 2048]) == 10
    for x in ctxs + ad.contexts(ad.DAG_BUILDS):
        n, q, baseR = x[8]
        assert 1 <= n <= (4 if x[3] == 2048 else 8)
        assert ad.bsk_words(n, x[3], ad.gadget_digits(x[5], x[4]), baseR, ad.digit_count(q, baseR)) * 8 <= ad.KEY_BYTES_MAX, x
    assert len(ROWS) == 2 * len(ad.BUILDS) == 52 and len(DAG_ROWS) == 3


@pytest.mark.parametrize("g,N", CPU_CONTEXTS)
def test_cpu_edge_ciphertexts_execute_the_steps_they_claim(orc, g, N):
    """on the oracle alone: dR and the key size are the restated ones; every edge ciphertext has the digits it is named
    after (worst_case.ap_digits, an independent loop) and executes the steps it claims; a = 0 leaves the test polynomial;
    the numpy blind rotation that reads the key through key_index() gives the oracle's accumulator word for word and reads
    exactly the indices of the non-zero digits (for baseR > q none at a0 >= q)"""
    q, baseR = ad.GEOMETRIES[g][N]
    gb = 9 if N != 1024 else 7
    n = ad.lwe_dimension(N, ad.gadget_digits("q27", gb), q, baseR)
    o = orc.Oracle(method=orc.AP, custom=base._custom(n, N, q, base._q27(orc.lib(), N), 1 << gb, baseR=baseR))
    p = o.params
    dR = p["dR"]
    assert dR == ad.digit_count(q, baseR) == ad.DR[g]
    assert o.bsk_words() == ad.bsk_words(n, N, p["dG"], baseR, dR) and ad.rgsw_count(n, baseR, dR) * 4 * p["dG"] * N == o.bsk_words()
    edge = ad.edge_a(q, baseR, dR, n)
    assert len(edge) == dR + 4 and edge[0][2] == 0
    seen_digits = [set() for _ in range(dR)]
    for name, a, steps in edge:
        prep = np.array(list(a) + [0], dtype=np.uint64)
        ds = wc.ap_digits(o, prep)
        assert ds == [ad.digits(q, baseR, dR, x) for x in a], name
        assert wc.executed_steps(o, prep) == steps, name
        assert all(wc._ap_value(q, baseR, dR, d) == x for d, x in zip(ds, a)), name
        for d in ds:
            for k in range(dR):
                seen_digits[k].add(d[k])
    for k in range(dR):
        only = [ds for ds in wc.ap_digits(o, np.array(edge[1 + k][1] + [0], dtype=np.uint64))]
        assert all(d[k] != 0 and sum(1 for x in d if x) == 1 for d in only), k
        assert {0, 1, ad.digit_max(q, baseR, dR, k)} <= seen_digits[k], (k, seen_digits[k])
    assert max(seen_digits[dR - 1]) == (q - 1) // baseR ** (dR - 1)
    if dR > 1:
        assert sum(1 for d in ad.digits(q, baseR, dR, edge[dR + 1][1][0]) if d) >= dR - 1      # the low digits all at baseR - 1
    assert ad.digits(q, baseR, dR, edge[-1][1][0]) == [1] + [0] * (dR - 1)
    o.keygen(4200)
    K = ad.IndexedKeys(o)
    o._xor_single_keys = K
    rng = np.random.default_rng(4201)
    for name, gate, prep, _ in ad.cases(o, rng):
        K.read.clear()
        m = xm.plain_poly(p, gate, int(prep[n]))
        acc = xm.blind_rotate(o, m, prep)
        assert np.array_equal(acc, o.blind_rotate(gate, prep)), name
        want = [ad.key_index(i, d, k, baseR, dR) for i, ds in enumerate(wc.ap_digits(o, prep)) for k, d in enumerate(ds) if d]
        assert K.read == want and all(0 <= x < ad.rgsw_count(n, baseR, dR) for x in want), name
        assert all((x // dR) % baseR < q for x in want)
        if name.startswith("a=0"):
            assert not want and not acc[:N].any() and np.array_equal(acc[N:], m)
    o.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _keys_equal(o, c, seed):
    o.keygen(seed)
    c.KeyGen(seed)
    s, z = c.export_sk()
    assert np.array_equal(s, o.sk()) and np.array_equal(z, o.z())
    R2N = 4 * o.params["dG"] * o.N
    for name, got, want, width in (("key-switching", c.export_ksk(), o.ksk(), o.n + 1), ("bootstrapping", c.export_bsk(), o.bsk(), R2N)):
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0])
            extra = ""
            if name == "bootstrapping":
                idx, dR, bR = k // R2N, o.params["dR"], o.params["baseR"]
                extra = " = RGSW ciphertext %d (coefficient %d, digit value %d, position %d)" % (idx, idx // (dR * bR), (idx // dR) % bR, idx % dR)
            pytest.fail("%s key: %d words differ, first at word %d (row %d, column %d%s): engine %d, oracle %d"
                        % (name, int((got != want).sum()), k, k // width, k % width, extra, int(got[k]), int(want[k])))


@gpu
@pytest.mark.parametrize("row", ids(ROWS))
def test_keygen_and_steps_at_every_digit_geometry(bce, orc, monkeypatch, row):
    o, c = base._pair(bce, orc, row, monkeypatch)
    assert o.params["dR"] == c.params["dR"] == ad.DR[row.geometry]
    _keys_equal(o, c, 4202)
    o._xor_single_keys = None
    rng = np.random.default_rng(4203)
    bad, _ = base._run_and_compare(o, c, ad.cases(o, rng), row.id)
    bad += ops._run_and_compare(o, c, ad.two_operand_cases(o, rng), row.id)[0]
    ops._finish(o, c, bad)


@gpu
@pytest.mark.parametrize("row", ids(DAG_ROWS))
def test_dataflow_kernel_at_digit_geometry(bce, orc, monkeypatch, row):
    """the persistent kernels (k_bootstrap_dag, k_bootstrap_dag64) share the step loop of their body: the edge ciphertexts
    as plain gates on two real operands, the BCE_XOR and the pair as one run; every output row equals the reference and the
    frontier path's"""
    o, c = base._pair(bce, orc, row, monkeypatch)
    assert c.dag_supported()
    _keys_equal(o, c, 4204)
    o._xor_single_keys = None
    rng = np.random.default_rng(4205)
    q = o.params["q"]
    cases = []
    for t, (name, gate, prep, _) in enumerate(ad.cases(o, rng)):
        n0, n1 = wc.NEGATIONS[t % 4]
        ct1, ct2 = wc.split_operands(q, prep, n0, n1)
        cases.append((name + " neg=%d%d" % (n0, n1), gate, ct1, ct2, n0, n1, prep))
    cases += ad.two_operand_cases(o, rng)
    nb = len(cases)
    descs = ops._load(c, cases, copies=2)
    c.EvalGates(descs)                                             # block 0: the frontier path
    dag = c.dag_create(descs, pairs=True)
    c.dag_run(dag, instances=1, slot_stride=4 * nb, slot_base=4 * nb)
    c.synchronize()
    last = c.dag_last_run()
    c.dag_destroy(dag)
    assert last["done"] == nb and last["abort"] == 0, last
    outs = np.arange(2 * nb, 4 * nb, dtype=np.uint32)
    stepped, flowed = c.lwe_read(outs), c.lwe_read(outs + 4 * nb)
    bad = []
    for i, case in enumerate(cases):
        for s, (_, _, want) in enumerate(ops._reference(o, case)[1]):
            for what, got in (("frontier path", stepped[2 * i + s]), ("dataflow kernel", flowed[2 * i + s])):
                if not np.array_equal(got, want):
                    k = int(np.flatnonzero(got != want)[0])
                    bad.append("%s | %s | output %d: first difference at %d: engine %d, reference %d" % (what, case[0], s, k, int(got[k]), int(want[k])))
    ops._finish(o, c, bad)
