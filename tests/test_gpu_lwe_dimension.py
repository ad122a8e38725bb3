"""LWE-dimension sweep: the key-switch tails, the prologue and the LWE row kernels at every row geometry n produces.

Every other parity test builds its custom contexts at n = 16 (one row at 24) or takes n from the parameter table.  n decides
how a key-switching row is read: 16-byte groups G = (n + VW) / VW, waves per row RW, row slices SL, the cap of the vector
pass and the scalar pass behind it, and through the launch size the number S of workgroups a bootstrap is spread over
(tests/lwe_dimension.py restates the rules and names the classes).  This file runs

  tail      bce_debug_tail (k_tail_gather / k_tail_finish) on the rounding-boundary accumulators of the worst-case suite and
            uniform ones, cycled to launch counts that give every S, under a uniform key-switching key and one of all qKS - 1
            (at S = 1 the bound of the u32 running sums), at every class and in-class edge of both row widths, on 32-bit and
            64-bit accumulator words and with sums folded every 8 rows (qKS = 2^29);
  fused     full bootstraps of the split-transform family under BCE_VARIANT=3 (the fused tail at any launch size): ciphertexts
            whose prepared a is non-zero only where a loop pass changes, keys uniform on those rows; plain gates under all
            negations, BCE_XOR and pairs; n = 1024 of each width also in one saturated launch of the default selection and as
            a small DAG on the dataflow kernel; both sides of fused_tail_fits;
  residency the LDS-bound residency of the split-transform family (context creation; one dataflow run on either side of the
            persistent kernel's own bound);
  rows      lwe_write / lwe_read and k_pool_pack in both directions (device gather and scatter), NOT / COPY, bce_check_slots
            with and without repair against numpy, on a random ternary secret;
  keygen    KeyGen(seed) against the oracle's at the tile edges of k_gen_ksk_rows.

Bar: bit for bit against the oracle at every stage.  Nothing is decrypted but in `rows`.  The CPU half (not marked gpu) asserts
that the lists hit every class, edge and S and that the sparse ciphertexts execute the steps they claim.
"""
import numpy as np
import pytest

import lwe_dimension as ld
import test_gpu_worst_case as base
import test_gpu_worst_case_ops as ops
import worst_case as wc

gpu = pytest.mark.gpu
Row = base.Row
LATER = base.STAGES[1:]


# ---- contexts ----------------------------------------------------------------------------------------------------------------
def _wave(n, width, qKS=None, baseKS=4):
    """N = 512, the 27-bit prime, base 2^9: the wave-per-transform family (the tail kernels take N at run time)"""
    return lambda L, b, o: base._custom(n, 512, 512, base._q27(L, 512), 1 << 9, qKS=qKS or ld.QKS[width], baseKS=baseKS)


def _fp64(n, width):
    return lambda L, b, o: base._custom(n, 512, 512, base._prime_below(L, 1 << 39, 512), 1 << 14, qKS=ld.QKS[width], baseKS=4)


def _split(n, width, baseKS=8):
    """N = 1024, base 2^7, the 27-bit prime: the split-transform family"""
    return lambda L, b, o: base._custom(n, 1024, 1024, base._q27(L, 1024), 1 << 7, qKS=ld.QKS[width], baseKS=baseKS)


TAIL_ROWS = [Row("tail_%s" % w, "n%d" % n, wc.GINX, _wave(n, w)) for w in ld.WIDTHS for n in ld.SEPARATE_N[w]]
TAIL_ROWS += [Row("tail_u32_qKS_2^29", "n256", wc.GINX, _wave(256, "u32", qKS=1 << 29)),
              Row("tail_fp64_u32", "n1025", wc.GINX, _fp64(1025, "u32")), Row("tail_fp64_u16", "n1024", wc.GINX, _fp64(1024, "u16")),
              Row("tail_split_shape_u32", "n512", wc.GINX, _split(512, "u32"))]
FUSED_ROWS = [Row("fused_%s" % w, "n%d" % n, wc.GINX, _split(n, w), {"BCE_VARIANT": "3"},
                  expect={"forward_units": 1, "forward_mfma": int(n <= 895)}) for w in ld.WIDTHS for n in ld.FUSED_N[w]]
SATURATED_ROWS = [Row("saturated_%s" % w, "n1024", wc.GINX, _split(1024, w), {}, 600, {"forward_units": 1, "forward_mfma": 0}) for w in ld.WIDTHS]
ROW_KERNEL_ROWS = [Row("rows_u32", "n%d" % n, wc.GINX, _wave(n, "u32")) for n in ld.ROW_KERNEL_N]
ids = lambda rows: [pytest.param(r, id=r.id) for r in rows]


# ---- CPU half ------------------------------------------------------------------------------------------------------------------
def test_cpu_geometry_is_the_table_and_the_lists_hit_every_class_and_edge():
    """the restated formulas give the class table for every n = 1 .. N_MAX; per row width and tail, the n lists of the sweep
    hit every class and every in-class edge the range holds (G = 1, a full last group and one element into a new one, every
    last wave with a single active lane), and both lengths of the scalar pass"""
    for w in ld.WIDTHS:
        vw = ld.VW[w]
        for table, cls, cap, chosen in ((ld.SEPARATE_TABLE[w], ld.separate_class, ld.SEPARATE_CAP, ld.SEPARATE_N[w]),
                                        (ld.FUSED_TABLE[w], ld.fused_class, ld.FUSED_CAP, ld.FUSED_N[w])):
            assert table[0][0] == 1 and table[-1][1] == ld.N_MAX and all(a[1] + 1 == b[0] for a, b in zip(table, table[1:]))
            for lo, hi, want in table:
                assert all(cls(n, vw) == want for n in range(lo, hi + 1)), (w, lo, hi, want)
                assert any(lo <= n <= hi for n in chosen), "%s: no n of %s in the class %d..%d %s" % (w, chosen, lo, hi, want)
            universe = set().union(*(ld.edges(n, vw, cap) for n in range(1, ld.N_MAX + 1)))
            hit = set().union(*(ld.edges(n, vw, cap) for n in chosen))
            assert hit == universe, "%s: %s misses the edges %s" % (w, chosen, sorted(universe - hit))
            assert {"G = 1", "n + 1 a multiple of VW", "one element into a new group"} < universe
    lanes = lambda w, cap: sorted(int(e.split("= ")[-1]) for e in set().union(*(ld.edges(n, ld.VW[w], cap) for n in range(1, ld.N_MAX + 1))) if "lane" in e)
    assert lanes("u16", ld.SEPARATE_CAP) == lanes("u16", ld.FUSED_CAP) == [65, 129]
    assert lanes("u32", ld.SEPARATE_CAP) == [65, 129, 193] and lanes("u32", ld.FUSED_CAP) == [65, 129, 193, 257]
    # the scalar pass of the separate tail: one element (the b column of n = 1024) and two; the fused tail never has one
    assert sorted(ld.tail_geometry(n, 4, ld.SEPARATE_CAP)[2] for n in ld.SEPARATE_N["u32"])[-2:] == [1, 2]
    assert not any(ld.tail_geometry(n, ld.VW[w], ld.FUSED_CAP)[2] for w in ld.WIDTHS for n in range(1, ld.N_MAX + 1))
    # idle trailing waves of the fused tail: 8 - RW SL
    assert [8 - rw * sl for rw, sl in (ld.fused_class(1024, 8), ld.fused_class(1024, 4), ld.fused_class(768, 4))] == [2, 3, 0]
    # the contexts beside the lists sit where they claim: u64 words on the capped class and on three waves per row
    assert ld.separate_class(1025, 4) == (4, 1, True) and ld.separate_class(1024, 8) == (3, 1, False) and ld.separate_class(512, 4) == (3, 1, False)
    assert set(ld.SEPARATE_N["u32"]) < set(ld.ROW_KERNEL_N) and {63, 64, 65, 127, 128, 129} < set(ld.ROW_KERNEL_N)
    assert len(TAIL_ROWS) == 6 + 11 + 4 and len(FUSED_ROWS) == 5 + 7


def test_cpu_launch_counts_hit_every_split():
    """the five launch counts give S = 16, 8, 4, 2, 1 at N = 1024 and 8, 8, 4, 2, 1 at N = 512 on 256 CUs, and every S of the
    shape on any CU count that is a multiple of 8"""
    assert ld.launch_counts(256) == [1, 65, 129, 257, 513]
    assert [ld.tail_split(256, 1024, k) for k in ld.launch_counts(256)] == [16, 8, 4, 2, 1]
    assert [ld.tail_split(256, 512, k) for k in ld.launch_counts(256)] == [8, 8, 4, 2, 1]
    for cu in (64, 104, 256, 304):
        assert {ld.tail_split(cu, 1024, k) for k in ld.launch_counts(cu)} == {16, 8, 4, 2, 1}
        assert {ld.tail_split(cu, 512, k) for k in ld.launch_counts(cu)} == {8, 4, 2, 1}
    # S = 1 at N = 512: one workgroup walks all N dKS rows; the key of all qKS - 1 keeps the u32 running sums below 2^32 only
    # because they are folded every floor(2^32 / qKS) rows: one chunk at qKS = 2^17, chunks of 8 rows at 2^29
    assert 512 * 9 * ((1 << 17) - 1) < 1 << 32 and 16 * ((1 << 29) - 1) >= 1 << 32


def test_cpu_fused_tail_rule_has_a_context_on_either_side():
    """fused_tail_fits at u16, n = 511, qKS = 2^14: baseKS = 8 (dKS = 5) needs 53,248 of the 55,296 bytes, baseKS = 4 (dKS = 7)
    does not fit; every context of the fused part fits"""
    assert ld.LAT_TAIL_BYTES == 55296
    assert ld.fused_tail_need(511, 1024, 5, 8) == 53248 and ld.fused_tail_fits(511, 1024, 5, 8)
    assert ld.fused_tail_need(511, 1024, 7, 8) > ld.LAT_TAIL_BYTES and not ld.fused_tail_fits(511, 1024, 7, 8)
    for w, dKS in (("u16", 5), ("u32", 6)):
        assert all(ld.fused_tail_fits(n, 1024, dKS, ld.VW[w]) for n in ld.FUSED_N[w])


def test_cpu_lds_residency_rule():
    """two workgroups of the matrix-pipe build fit a CU's 160 KiB up to n = 895, of the quarter-unit build up to n = 2431"""
    assert ld.lat_lds_bytes(True, 16) == (19584 + 20) * 4
    assert 2 * ld.lat_lds_bytes(True, 895) == ld.LDS_BYTES_PER_CU < 2 * ld.lat_lds_bytes(True, 896)
    assert 2 * ld.lat_lds_bytes(False, 2431) == ld.LDS_BYTES_PER_CU < 2 * ld.lat_lds_bytes(False, 2432)
    assert ld.lat_lds_bytes(False, 2432) <= ld.LDS_BYTES_PER_CU


ANCHORED = ("n3", "n7", "n512", "n1025")


@pytest.mark.parametrize("row", ids(FUSED_ROWS + SATURATED_ROWS))
def test_cpu_sparse_ciphertexts_execute_the_steps_they_claim(orc, row):
    """on the oracle alone, for EVERY context of the full-bootstrap part (the n = 1024 contexts of the saturated and dataflow
    ids among them): every sparse case prepares (through EvalNOT and gate_prep) to a vector that is non-zero exactly at its
    subset of loop_indices(n) and executes that many steps, and the cases together execute every loop index.  On the contexts
    of ANCHORED (the smallest n, a mid one of each width, the largest) also the key: its non-zero rows are exactly the loop
    indices, and the numpy blind rotation on it is the oracle's own word for word"""
    o = base._oracle(orc, row)
    q, n = o.params["q"], o.n
    idx = ld.loop_indices(n)
    assert idx == sorted(set(i for i in (0, 511, 512, 1023, n - 1) if i < n)) and idx[0] == 0 and idx[-1] == n - 1
    assert n != 1024 or idx == [0, 511, 512, 1023]              # the one n at which n - 1 is a pass boundary itself
    cases = ld.sparse_cases(o)
    assert len(cases) == 7 and set((x[4], x[5]) for x in cases) == set(wc.NEGATIONS)
    assert sum(1 for x in cases if x[1] == wc.XOR) == 1 and sum(1 for x in cases if wc.is_pair(x[1])) == 2
    executed = set()
    for name, op, ct1, ct2, n0, n1, prep, subset in cases:
        a, b = (o.eval_not(ct1) if n0 else ct1), (o.eval_not(ct2) if n1 else ct2)
        assert np.array_equal(o.gate_prep(wc.AND if op == wc.XOR else op & 0xFF, a, b), prep), name
        assert list(np.flatnonzero(prep[:n])) == subset and wc.executed_steps(o, prep) == len(subset), name
        assert np.count_nonzero(ct2) >= n // 2 and int(max(ct1.max(), ct2.max())) < q, name
        executed.update(subset)
    assert executed == set(idx) and any(not x[7] for x in cases)
    bs = [int(x[6][n]) for x in cases if x[1] in wc.PLAIN]
    edge = [b for b, x in zip(bs, [x for x in cases if x[1] in wc.PLAIN]) if b in wc.b_patterns(q, x[1])]
    assert 0 < len(edge) < len(bs), "b on a window edge and off it"
    if row.selector in ANCHORED:
        rng = np.random.default_rng(4002)
        bsk = ld.sparse_bsk(o, rng)
        assert sorted(set(int(i) for i in np.flatnonzero(bsk.reshape(n, -1).any(axis=1)))) == idx
        ld.install(o, None, bsk, wc.extreme_ksk(o, "0", rng))
        for case in cases[:1] + cases[5:6]:
            ld.reference(o, case, anchor=True)
    o.close()


# ---- GPU 1: the separate tail alone --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ids(TAIL_ROWS))
def test_separate_tail_at_every_row_geometry(bce, orc, monkeypatch, row):
    """part `tail`: every row of lweN, ks and the pool equals extract_modswitch, keyswitch and modswitch_final, at launch
    counts 1, cu/4 + 1, cu/2 + 1, cu + 1, 2 cu + 1 (every S the shape has), under a uniform key and one of all qKS - 1"""
    o, c = base._pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(4001)
    Q, N, n = o.params["Q"], o.N, o.n
    cu = c.launch_capacity()[0]
    counts = ld.launch_counts(cu)
    split = {k: c.debug_tail_split(k) for k in counts}           # launch_tail's own rule, not the restatement
    assert set(split.values()) == ({16, 8, 4, 2, 1} if N == 1024 else {8, 4, 2, 1}), (cu, split)
    assert split == {k: ld.tail_split(cu, N, k) for k in counts}, "tail_split of lwe_dimension.py is not the engine's"
    accs = np.concatenate([base._tail_accumulators(o, rng), rng.integers(0, Q, size=(4, 2, N), dtype=np.uint64)])
    r_lweN = np.stack([o.extract_modswitch(a.reshape(-1)) for a in accs])
    c.pool_reserve(counts[-1])
    bsk = np.zeros(wc.bsk_shape(o), dtype=np.uint64)           # the tail does not read it
    bad = []
    for kpat in ("uniform", "qKS-1"):
        base._install(o, c, bsk, wc.extreme_ksk(o, kpat, rng))
        r_ks = np.stack([o.keyswitch(l) for l in r_lweN])
        r_out = np.stack([o.modswitch_final(k) for k in r_ks])
        for count in counts:
            pick = np.arange(count) % len(accs)
            slots = np.arange(count, dtype=np.uint32)
            lweN, ks = c.debug_tail(accs[pick], slots)
            out = c.lwe_read(slots)
            for stage, got, want in zip(LATER, (lweN, ks, out), (r_lweN[pick], r_ks[pick], r_out[pick])):
                if not np.array_equal(got, want):
                    i, k = (int(v[0]) for v in np.nonzero(got != want))
                    bad.append("ksk %s | count %d (S = %d) | %s: %d words differ, first at row %d (accumulator %d) column %d: engine %d, oracle %d"
                               % (kpat, count, split[count], stage, int((got != want).sum()), i, i % len(accs), k, int(got[i, k]), int(want[i, k])))
                    break
    o.close()
    c.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))


# ---- GPU 2: the fused tail and the prologue ------------------------------------------------------------------------------------
def _sparse_pair(bce, orc, monkeypatch, row, seed, ksk="uniform"):
    o, c = base._pair(bce, orc, row, monkeypatch)
    rng = np.random.default_rng(seed)
    ld.install(o, c, ld.sparse_bsk(o, rng), wc.extreme_ksk(o, ksk, rng))
    cases = ld.sparse_cases(o)
    refs = [ld.reference(o, case, anchor=(i == 0)) for i, case in enumerate(cases)]
    return o, c, cases, refs


def _against(what, cases, got, refs):
    bad = []
    for case, g, r in zip(cases, got, refs):
        d = ops._first_difference(g, r)
        if d:
            bad.append("%s | %s | %s: first difference at %d: engine %d, reference %d" % ((what, case[0]) + d))
    return bad


@gpu
@pytest.mark.parametrize("row", ids(FUSED_ROWS))
def test_fused_tail_and_prologue_at_every_row_geometry(bce, orc, monkeypatch, row):
    """part `fused`, BCE_VARIANT=3: the sparse cases in one small launch that runs the tail in its epilogue; the accumulator,
    extract + ModSwitch, KeySwitch and the pool row of every output (a pair's second after the barrier) equal the reference"""
    o, c, cases, refs = _sparse_pair(bce, orc, monkeypatch, row, 4003)
    assert c.dag_supported()
    t0 = c.timing()["fused_tail_launches"]
    got = ops._engine_stages(c, ops._load(c, cases), 2 * len(cases))
    assert c.timing()["fused_tail_launches"] == t0 + 1, "the launch did not run the tail in its epilogue"
    ops._finish(o, c, _against(row.id, cases, got, refs))


def _saturated(o, c, cases, refs, replicas, what, fuses):
    """the cases in a small launch (separate tail kernels) and replicated into one saturated launch of the default selection:
    fused_tail_launches goes up by one iff `fuses`; every replica equals the small launch, the small launch the reference"""
    nb = len(cases)
    descs = ops._load(c, cases, extra=2 * replicas)
    t0 = c.timing()["fused_tail_launches"]
    small = ops._engine_stages(c, descs, 2 * nb)
    assert c.timing()["fused_tail_launches"] == t0, "the small launch was expected to run the separate tail kernels"
    big = [descs[i % nb][:3] + (4 * nb + 2 * i,) + descs[i % nb][4:] for i in range(replicas)]
    got = ops._engine_stages(c, big, 4 * nb)
    assert c.timing()["fused_tail_launches"] == t0 + int(fuses), "fused_tail_launches after the saturated launch (fuses = %d)" % fuses
    bad = _against(what + " | small launch", cases, small, refs)
    for i in range(replicas):
        d = ops._first_difference(got[i], small[i % nb])
        if d:
            bad.append("%s | replica %d of %s | %s differs from the small launch at %d" % (what, i, cases[i % nb][0], d[0], d[1]))
    return bad


@gpu
@pytest.mark.parametrize("row", ids(SATURATED_ROWS))
def test_saturated_default_launch_at_n_1024(bce, orc, monkeypatch, row):
    """the default selection at n = 1024 of each width: 600 bootstraps in one launch fuse the tail (three and five waves per
    row, trailing waves idle) on the quarter-unit body (the matrix-pipe build would leave a CU one workgroup)"""
    o, c, cases, refs = _sparse_pair(bce, orc, monkeypatch, row, 4004)
    cu = c.launch_capacity()
    assert cu[1] == 2 * cu[0] and row.fused > cu[1]
    ops._finish(o, c, _saturated(o, c, cases, refs, row.fused, row.id, True))


@gpu
@pytest.mark.parametrize("baseKS,fits", [(8, 1), (4, 0)])
def test_fused_tail_rule_both_sides(bce, orc, monkeypatch, baseKS, fits):
    """u16, n = 511, qKS = 2^14: with dKS = 5 the tail fits the dead LDS (the saturated launch fuses, the dataflow kernel
    exists), with dKS = 7 it does not (no dataflow kernel; the saturated launch keeps the separate tail and still equals the
    reference)"""
    row = Row("rule_u16", "n511_baseKS%d" % baseKS, wc.GINX, _split(511, "u16", baseKS), {}, 600, {"forward_mfma": 1})
    o, c, cases, refs = _sparse_pair(bce, orc, monkeypatch, row, 4005)
    assert o.params["dKS"] == (5 if fits else 7)
    assert int(c.dag_supported()) == fits == int(ld.fused_tail_fits(511, 1024, o.params["dKS"], 8))
    ops._finish(o, c, _saturated(o, c, cases, refs, row.fused, row.id, bool(fits)))


@gpu
@pytest.mark.parametrize("row", ids(SATURATED_ROWS))
def test_dataflow_kernel_at_n_1024(bce, orc, monkeypatch, row):
    """a small DAG on the persistent kernel at n = 1024 of each width: a chain of three (the second and third read refreshed,
    dense ciphertexts: all n steps, the prologue's three passes), a pair task and a BCE_XOR; every register equals the frontier
    path's and the reference's (plain gates on dense inputs: the oracle's EvalBinGate)"""
    o, c, cases, refs = _sparse_pair(bce, orc, monkeypatch, row, 4006)
    assert c.dag_supported()
    first, pair, xor = cases[0], cases[5], cases[4]
    ins = np.stack([first[2], first[3], pair[2], pair[3], xor[2], xor[3]])
    tasks = [(first[1], 0, 1, 6, first[4], first[5]), (wc.OR, 6, 2, 7, 0, 1), (wc.NAND, 7, 6, 8, 1, 0),
             (pair[1], 2, 3, 9, pair[4], pair[5]), (xor[1], 4, 5, 11, xor[4], xor[5])]
    want = {6: refs[0][1][0][2], 9: refs[5][1][0][2], 10: refs[5][1][1][2], 11: refs[4][1][0][2]}
    want[7] = o.eval_bingate(wc.OR, want[6], o.eval_not(ins[2]))
    want[8] = o.eval_bingate(wc.NAND, o.eval_not(want[7]), want[6])
    stride, regs = 12, np.arange(6, 12, dtype=np.uint32)
    c.pool_reserve(2 * stride)
    for k in range(2):
        c.lwe_write(np.arange(6, dtype=np.uint32) + k * stride, ins)
        c.lwe_write(regs + k * stride, np.zeros((6, o.n + 1), dtype=np.uint64))
    for level in ([tasks[0], tasks[3], tasks[4]], [tasks[1]], [tasks[2]]):
        c.EvalGates(level)                                        # block 0: the frontier path
    dag = c.dag_create(tasks, pairs=True)
    c.dag_run(dag, instances=1, slot_stride=stride, slot_base=stride)
    c.synchronize()
    last = c.dag_last_run()
    assert last["done"] == len(tasks) and last["abort"] == 0, last
    stepped, flowed = c.lwe_read(regs), c.lwe_read(regs + stride)
    c.dag_destroy(dag)
    bad = []
    for j, r in enumerate(regs):
        for what, got in (("frontier path", stepped[j]), ("dataflow kernel", flowed[j])):
            if not np.array_equal(got, want[int(r)]):
                k = int(np.flatnonzero(got != want[int(r)])[0])
                bad.append("%s | register %d: first difference at %d: engine %d, reference %d" % (what, r, k, int(got[k]), int(want[int(r)][k])))
    ops._finish(o, c, bad)


# ---- GPU 3: LDS residency of the split-transform family ------------------------------------------------------------------------
def _split_ctx(bce, orc, monkeypatch, n, env=None):
    for k in ("BCE_VARIANT", "BCE_FWD_MFMA", "BCE_FWD_UNITS", "BCE_FOLD", "BCE_FUSE_TAIL", "BCE_OCCUPANCY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return bce.BinFHEContext(method=bce.GINX, custom=_split(n, "u16")(orc.lib(), bce, orc))


@gpu
def test_matrix_pipe_build_is_granted_only_where_two_workgroups_fit(bce, orc, monkeypatch):
    """n = 895: two workgroups of the matrix-pipe build fill a CU's LDS exactly; n = 896: the quarter-unit body stays; the
    saturated capacity is two workgroups per CU on both sides"""
    seen = []
    for n in (895, 896):
        c = _split_ctx(bce, orc, monkeypatch, n)
        cu, full = c.launch_capacity()
        seen.append((c.forward_mfma(), c.forward_units(), full == 2 * cu))
        c.close()
    assert seen == [(1, 1, True), (0, 1, True)], seen
    assert 2 * ld.lat_lds_bytes(True, 895) <= ld.LDS_BYTES_PER_CU < 2 * ld.lat_lds_bytes(True, 896)


@gpu
def test_saturated_capacity_is_bounded_by_lds(bce, orc, monkeypatch):
    """the quarter-unit build at n = 2431 / 2432 (BCE_FWD_MFMA=0): two workgroups per CU, then one"""
    seen = []
    for n in (2431, 2432):
        c = _split_ctx(bce, orc, monkeypatch, n, {"BCE_FWD_MFMA": "0"})
        cu, full = c.launch_capacity()
        seen.append((c.forward_mfma(), full // cu, full % cu))
        c.close()
    assert seen == [(0, 2, 0), (0, 1, 0)], seen


@gpu
@pytest.mark.parametrize("n,per_cu", [(887, 2), (888, 1)])
def test_dataflow_grid_follows_the_persistent_kernels_own_lds(bce, orc, monkeypatch, n, per_cu):
    """the persistent kernel keeps a 32-byte mailbox in front of the LDS layout, so two of ITS workgroups (matrix-pipe build)
    fit a CU up to n = 887 while two of the per-frontier kernel fit up to 895: asked for two workgroups per CU, bce_dag_run
    grants two at n = 887 and one at n = 888 (the grid never exceeds the resident count), and the registers equal the
    reference either way.  The same rule gives the quarter-unit build's band n = 2424 .. 2431 (not run: its keys exceed a GiB)"""
    assert 2 * (ld.lat_lds_bytes(True, 887) + 32) <= ld.LDS_BYTES_PER_CU < 2 * (ld.lat_lds_bytes(True, 888) + 32)
    assert 2 * (ld.lat_lds_bytes(False, 2423) + 32) <= ld.LDS_BYTES_PER_CU < 2 * (ld.lat_lds_bytes(False, 2424) + 32)
    row = Row("dag_residency_u16", "n%d" % n, wc.GINX, _split(n, "u16"), {}, expect={"forward_mfma": 1})
    o, c, cases, refs = _sparse_pair(bce, orc, monkeypatch, row, 4009)
    cu, full = c.launch_capacity()
    assert full == 2 * cu and c.dag_supported()
    picked = [0, 4, 5]                                             # a plain gate, the BCE_XOR, a pair
    ins = np.concatenate([np.stack([cases[i][2], cases[i][3]]) for i in picked])
    tasks = [(cases[i][1], 2 * k, 2 * k + 1, 6 + 2 * k, cases[i][4], cases[i][5]) for k, i in enumerate(picked)]
    c.pool_reserve(12)
    c.lwe_write(np.arange(6, dtype=np.uint32), ins)
    c.dag_set_limits(workgroups_per_cu=2)
    dag = c.dag_create(tasks, pairs=True)
    c.dag_run(dag)
    c.synchronize()
    last = c.dag_last_run()
    got = c.lwe_read(np.arange(6, 12, dtype=np.uint32))
    c.dag_destroy(dag)
    assert last["done"] == len(tasks) and last["abort"] == 0, last
    assert last["workgroups_per_cu"] == per_cu, last
    bad = []
    for k, i in enumerate(picked):
        for s, (_, _, want) in enumerate(refs[i][1]):
            if not np.array_equal(got[2 * k + s], want):
                j = int(np.flatnonzero(got[2 * k + s] != want)[0])
                bad.append("%s | output %d: first difference at %d: engine %d, reference %d" % (cases[i][0], s, j, int(got[2 * k + s][j]), int(want[j])))
    ops._finish(o, c, bad)


class _DeviceWords:
    """a device buffer of u32 words for bce_pool_gather / bce_pool_scatter, from the HIP runtime the engine itself loaded"""

    def __init__(self, words):
        import ctypes as C
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.hip, self.C, self.words, self.ptr = C.CDLL(path), C, words, C.c_void_p()

    def __enter__(self):
        assert self.hip.hipMalloc(self.C.byref(self.ptr), self.C.c_size_t(4 * self.words)) == 0
        return self

    def __exit__(self, *exc):
        self.hip.hipFree(self.ptr)

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        assert a.size <= self.words
        assert self.hip.hipMemcpy(self.ptr, a.ctypes.data_as(self.C.c_void_p), self.C.c_size_t(4 * a.size), 1) == 0      # host to device
        assert self.hip.hipDeviceSynchronize() == 0

    def download(self):
        out = np.zeros(self.words, dtype=np.uint32)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.ptr, self.C.c_size_t(4 * self.words), 2) == 0  # device to host
        return out


# ---- GPU 4: LWE row kernels and key generation -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("row", ids(ROW_KERNEL_ROWS))
def test_lwe_row_kernels_at_every_n(bce, orc, monkeypatch, row):
    """lwe_write / lwe_read round trip with k_pool_pack in both directions (the device gather of lwe_read and bce_pool_gather;
    bce_pool_scatter), nothing written past the rows; NOT and COPY (with and without the folded negation) over three instances at a slot
    stride of 7; bce_check_slots without and with repair against numpy on rows that sit on every rounding boundary of the
    decision, under a random ternary secret"""
    o, c = base._pair(bce, orc, row, monkeypatch)
    q, n = o.params["q"], o.n
    rng = np.random.default_rng(4007 + n)
    s = rng.integers(-1, 2, n).astype(np.int32)
    c.import_keys_eval(s, np.zeros(o.N, dtype=np.int32), np.zeros(o.bsk_words(), dtype=np.uint64),
                       np.zeros(int(np.prod(wc.ksk_shape(o))), dtype=np.uint32))
    assert np.array_equal(c.export_sk()[0], s)
    named = ld.check_rows(q, s, rng)
    rows = np.stack([r for _, r in named])
    nr, K, STRIDE = len(rows), 3, 7
    assert STRIDE % 4 and int(rows[-1].sum()) == n % 64 + 1 and rows[-1][n] == 1      # b is the last of the n % 64 + 1 ones
    # round trip.  lwe_write is a host copy per run of slots, lwe_read one bulk copy while the slots span at most 4 count + 64
    # rows; beyond that it gathers on the device.  k_pool_pack therefore runs here in both directions: to_pool = 0 through
    # lwe_read of slots 17 apart and through bce_pool_gather into a device buffer, to_pool = 1 through bce_pool_scatter
    POOL = 256
    c.pool_reserve(POOL)
    every = np.arange(POOL, dtype=np.uint32)
    fill = rng.integers(0, q, size=(POOL, n + 1), dtype=np.uint64)
    slots = np.arange(nr, dtype=np.uint32) * 17 + 5
    assert int(slots[-1]) < POOL and int(slots[-1] - slots[0]) + 1 > 4 * nr + 64, "lwe_read would take the bulk copy"
    c.lwe_write(every, fill)
    c.lwe_write(slots, rows)
    held = fill.copy()
    held[slots] = rows
    assert np.array_equal(c.lwe_read(every), held)                                     # bulk copy: what the pool holds
    assert np.array_equal(c.lwe_read(slots), rows) and np.array_equal(c.lwe_read(slots[::-1]), rows[::-1])   # k_pool_pack, to_pool = 0
    L, W = bce._bind_circuit(), n + 1
    with _DeviceWords((nr + 1) * W) as dev:                                            # one row of sentinels behind the rows
        dev.upload(np.full((nr + 1) * W, 0xFFFFFFFF, dtype=np.uint32))
        assert L.bce_pool_gather(c.h, slots.ctypes.data, nr, dev.ptr) == 0
        c.synchronize()
        packed = dev.download().reshape(nr + 1, W)
        assert np.array_equal(packed[:nr], rows.astype(np.uint32)), "bce_pool_gather: first difference at %s" % (np.argwhere(packed[:nr] != rows)[:1],)
        assert (packed[nr] == 0xFFFFFFFF).all(), "bce_pool_gather wrote past count rows of n + 1 words"
        dev.upload(np.ascontiguousarray(rows[::-1]).astype(np.uint32).reshape(-1))      # to_pool = 1: other rows into the same slots
        assert L.bce_pool_scatter(c.h, slots.ctypes.data, nr, dev.ptr) == 0
        c.synchronize()
    held[slots] = rows[::-1]
    after = c.lwe_read(every)
    assert np.array_equal(after[slots], rows[::-1]), "bce_pool_scatter: first difference at %s" % (np.argwhere(after[slots] != rows[::-1])[:1],)
    assert np.array_equal(after, held), "bce_pool_scatter changed a row it was not given"
    # NOT / COPY: instance k reads slots 0, 1 (+ 7 k) and writes 2 .. 5 (+ 7 k)
    src = np.stack([rows[(2 * k + j) % nr] for k in range(K) for j in range(2)])
    c.lwe_write(np.array([k * STRIDE + j for k in range(K) for j in range(2)], dtype=np.uint32), src)
    c.EvalGates([(bce.OP_NOT, 0, 0, 2), (bce.OP_COPY, 1, 1, 3), (bce.OP_NOT, 1, 1, 4, 1, 0), (bce.OP_COPY, 0, 0, 5, 1, 0)], instances=K, slot_stride=STRIDE)
    got = c.lwe_read(np.arange(K * STRIDE, dtype=np.uint32)).reshape(K, STRIDE, n + 1)
    for k in range(K):
        a, b = src[2 * k], src[2 * k + 1]
        assert np.array_equal(o.eval_not(a), wc.lwe_not(q, a))
        for j, want in enumerate((a, b, wc.lwe_not(q, a), b, b, wc.lwe_not(q, a))):      # NOT with neg0 copies, COPY with neg0 negates
            assert np.array_equal(got[k, j], want), "instance %d slot %d: first difference at %d" % (k, j, int(np.flatnonzero(got[k, j] != want)[0]))
    # decrypt / compare / repair
    base_slot = 64
    cslots = np.arange(base_slot, base_slot + nr, dtype=np.uint32)
    c.lwe_write(cslots, rows)
    ph = [ld.phase(q, s, r) for r in rows]
    msg = [ld.decision(q, p) for p in ph]
    assert set(msg) == {0, 1, 2, 3}
    for shift, repair in ((0, False), (1, False), (1, True)):
        expect = np.array([(m + shift * (1 + i % 3)) % 4 for i, m in enumerate(msg)], dtype=np.uint8)
        err = [ld.centred_error(q, p, int(e)) for p, e in zip(ph, expect)]
        wrong = [i for i in range(nr) if msg[i] != expect[i]]
        assert len(wrong) == (nr if shift else 0)
        c.check_reset()
        c.check_slots(cslots, expect, repair=repair, tag=40 + shift)
        rep, log = c.check_get()
        want = {"checked": nr, "mismatches": len(wrong), "repaired": len(wrong) if repair else 0, "sum_err": sum(err),
                "sum_sq_err": sum(e * e for e in err), "max_abs_err": max(abs(e) for e in err)}
        assert {k: rep[k] for k in want} == want, (shift, repair, rep, want, [nm for nm, _ in named])
        assert {(x["tag"], x["index"], x["slot"], x["got"], x["expect"], x["err"]) for x in log} == \
               {(40 + shift, i, base_slot + i, msg[i], int(expect[i]), err[i]) for i in wrong}
        after = c.lwe_read(cslots)
        if repair:
            fixed = np.zeros_like(rows)
            fixed[:, n] = expect.astype(np.uint64) * (q // 4)
            assert np.array_equal(after, fixed), "repair: every mismatching row becomes (0, ..., 0, expect q/4)"
        else:
            assert np.array_equal(after, rows), "repair = 0 changed the pool"
    o.close()
    c.close()


@gpu
@pytest.mark.parametrize("width", ld.WIDTHS)
@pytest.mark.parametrize("n", ld.KEYGEN_N)
def test_keygen_at_the_tile_edges(bce, orc, monkeypatch, n, width):
    """KeyGen(seed) against the oracle's keygen(seed) at N = 512: secret, key-switching key (64-wide tiles of
    k_gen_ksk_rows: n + 1 = 64, 65, 66, 129 elements per row) and bootstrapping key, word for word"""
    row = Row("keygen_%s" % width, "n%d" % n, wc.GINX, _wave(n, width, baseKS=32))
    o, c = base._pair(bce, orc, row, monkeypatch)
    o.keygen(4008 + n)
    c.KeyGen(4008 + n)
    s, z = c.export_sk()
    assert np.array_equal(s, o.sk()) and np.array_equal(z, o.z())
    for name, got, want in (("key-switching", c.export_ksk(), o.ksk()), ("bootstrapping", c.export_bsk(), o.bsk())):
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0])
            width_ = (n + 1) if name == "key-switching" else o.N
            pytest.fail("%s key: %d words differ, first at word %d (row %d, column %d): engine %d, oracle %d"
                        % (name, int((got != want).sum()), k, k // width_, k % width_, int(got[k]), int(want[k])))
    o.close()
    c.close()
