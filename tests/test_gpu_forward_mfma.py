"""Forward stages on position bits 9..4 of the quarter units as i8 matrix products (kernels.hip, ntt_forward_quarter3<true>;
default where the host conditions of csrc/fwd_mfma.hpp hold), against the quarter-unit body it replaces (BCE_FWD_MFMA=0, same
binary) and against the oracle.

Bar: every compared stage word for word.  The two bodies compute the same residues mod Q -- M6 (d - 64) on the matrix pipe
against six lazy butterflies on d - 64 + Q -- but different lazy representatives inside the forward phase; the MAC tail
returns canonical accumulator words, so accumulator, extract + ModSwitch, KeySwitch and final ciphertext are equal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x0FE5EED
OPS = ("OR", "AND", "NOR", "NAND", "XOR_FAST", "XNOR_FAST", "OP_REFRESH")


def _context(bce, monkeypatch, mfma, seed):
    monkeypatch.setenv("BCE_VARIANT", "3")            # the two-workgroups-per-CU build whatever the launch size
    monkeypatch.setenv("BCE_FWD_MFMA", "1" if mfma else "0")
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    assert c.forward_units() == 1 and c.forward_mfma() == (1 if mfma else 0) and c.forward_transforms_per_step() == 6
    c.KeyGen(seed)
    return c


def test_multi_round_launch_every_stage_equals_quarter_units_and_oracle(bce, orc, monkeypatch):
    """One launch of 1,150 bootstraps of DISTINCT gates (every operation, folded EvalNOTs, refreshes; more than two rounds
    of 512 workgroups): accumulator, extract + ModSwitch, KeySwitch and final ciphertext of every bootstrap equal between
    the matrix-pipe body and the quarter-unit body, and equal to the oracle's on the first / last workgroup of
    every round and the first gates (the samples of the saturated-launch and multi-round tests of test_gpu_engine.py)."""
    o = orc.Oracle(orc.STD128_OPT, orc.GINX)
    o.keygen(SEED)
    nb = 1150
    rng = np.random.default_rng(20261)
    bits = rng.integers(0, 2, size=2 * nb)
    cts = np.stack([o.encrypt(int(bits[i]), 70000 + i) for i in range(2 * nb)])
    ops = [getattr(bce, name) for name in OPS]
    descs = []
    for i in range(nb):
        op = ops[int(rng.integers(0, len(ops)))]
        n0, n1 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        descs.append((op, 2 * i, 2 * i + 1, 2 * nb + i, n0, n1 if op != bce.OP_REFRESH else 0))
    res = []
    for mfma in (1, 0):
        c = _context(bce, monkeypatch, mfma, SEED)
        c.pool_reserve(3 * nb)
        c.lwe_write(np.arange(2 * nb, dtype=np.uint32), cts)
        t0 = c.timing()["fused_tail_launches"]
        acc, lweN, ks = c.debug_eval_stages(descs)
        assert c.timing()["fused_tail_launches"] == t0 + 1            # one launch, tail in the epilogue
        out = c.lwe_read(np.arange(2 * nb, 3 * nb, dtype=np.uint32))
        res.append((np.array(acc), np.array(lweN), np.array(ks), out))
        c.close()
    for name, a, b in zip(("accumulator", "extract + ModSwitch", "KeySwitch", "final ciphertext"), res[0], res[1]):
        bad = np.flatnonzero((a != b).reshape(nb, -1).any(axis=1))
        print("%s: %d of %d bootstraps differ between the bodies" % (name, bad.size, nb))
        assert bad.size == 0, "%s differs, first bootstraps %s" % (name, bad[:8])
    acc, lweN, ks, out = res[0]
    for i in (0, 1, 2, 511, 512, 1023, 1024, nb - 1):
        op, i0, i1, _, n0, n1 = descs[i]
        ca = o.eval_not(cts[i0]) if n0 else cts[i0]
        cb = o.eval_not(cts[i1]) if n1 else cts[i1]
        a, b = int(bits[i0]) ^ n0, int(bits[i1]) ^ n1
        if op == bce.OP_REFRESH:
            pool = np.zeros((3 * nb, o.params["n"] + 1), dtype=np.uint64)
            pool[:2 * nb] = cts
            o.eval_gates(pool, [descs[i]])
            assert np.array_equal(out[i], pool[2 * nb + i]), "final ciphertext (refresh), bootstrap %d" % i
            assert o.decrypt(out[i]) == a
            continue
        r_acc = o.blind_rotate(op, o.gate_prep(op, ca, cb))
        assert np.array_equal(acc[i], r_acc), "accumulator differs from the oracle, bootstrap %d" % i
        r_lweN = o.extract_modswitch(r_acc)
        assert np.array_equal(lweN[i], r_lweN), "extract + ModSwitch, bootstrap %d" % i
        r_ks = o.keyswitch(r_lweN)
        assert np.array_equal(ks[i], r_ks), "KeySwitch, bootstrap %d" % i
        assert np.array_equal(out[i], o.modswitch_final(r_ks)), "final ciphertext, bootstrap %d" % i
        assert o.decrypt(out[i]) == [a | b, a & b, 1 - (a | b), 1 - (a & b), a ^ b, 1 - (a ^ b)][op]
    o.close()


def test_small_dag_through_the_persistent_kernel(bce, orc, monkeypatch):
    """The dependency-driven kernel shares the bootstrap body: 120 dependent gates x 2 instances through bce_dag_run at two
    workgroups per CU leave the same registers with either forward body (k_bootstrap_dag takes the same LatVariant), and a gate deep in the DAG replays on the oracle."""
    o = orc.Oracle(orc.STD128_OPT, orc.GINX)
    o.keygen(SEED)
    rng = np.random.default_rng(12)
    n_in, n_tasks, K = 12, 120, 2
    stride = n_in + n_tasks
    tasks = []
    for i in range(n_tasks):
        hi = n_in + i
        a, b = rng.integers(max(0, hi - 30), hi, 2)
        op = int(rng.choice([bce.AND, bce.OR, bce.NAND, bce.NOR]))
        tasks.append((op, int(a), int(b), hi, int(rng.integers(0, 2)), int(rng.integers(0, 2))))
    bits = rng.integers(0, 2, K * n_in).astype(np.uint8)
    slots = np.array([k * stride + i for k in range(K) for i in range(n_in)], dtype=np.uint32)
    regs = []
    for mfma in (1, 0):
        c = _context(bce, monkeypatch, mfma, SEED)
        assert c.dag_supported()
        c.pool_reserve(K * stride)
        c.set_encrypt_seed(SEED)
        c.Encrypt(bits, slots, enc_index_base=900)
        c.dag_set_limits(workgroups_per_cu=2)
        dag = c.dag_create(tasks)
        c.dag_run(dag, K, stride, 0)
        c.synchronize()
        last = c.dag_last_run()
        assert last["done"] == K * n_tasks and last["abort"] == 0 and last["workgroups_per_cu"] == 2
        regs.append(c.lwe_read(np.arange(0, K * stride, dtype=np.uint32)))
        c.dag_destroy(dag)
        c.close()
    assert np.array_equal(regs[0], regs[1])
    got = regs[0]
    for t in (tasks[0], tasks[-1]):
        op, a, b, out, n0, n1 = t
        ca, cb = got[stride + a], got[stride + b]
        ca = o.eval_not(ca) if n0 else ca
        cb = o.eval_not(cb) if n1 else cb
        assert np.array_equal(got[stride + out], o.eval_bingate(op, ca, cb))
    o.close()


def test_host_check_refuses_the_body_and_the_quarter_units_or_older_bodies_run(bce, orc, monkeypatch):
    """Contexts of the same kernel class in which the body must not be selected: q = 2N (factor 1: no quarter units at all,
    the whole-row + half-row bodies and the general MAC tail run), BCE_FWD_UNITS=0, and AP.  The first one is evaluated and
    compared with the oracle stage by stage."""
    monkeypatch.setenv("BCE_VARIANT", "3")
    monkeypatch.delenv("BCE_FWD_MFMA", raising=False)
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    assert c.forward_units() == 1 and c.forward_mfma() == 1          # the default where the conditions hold
    c.close()
    c = bce.BinFHEContext(bce.STD128_AP, bce.AP)
    assert c.forward_mfma() == 0
    c.close()
    monkeypatch.setenv("BCE_FWD_UNITS", "0")
    c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    assert c.forward_units() == 0 and c.forward_mfma() == 0
    c.close()
    monkeypatch.delenv("BCE_FWD_UNITS")
    L = orc.lib()
    N = 1024
    Q = L.bo_previous_prime(L.bo_first_prime(27, 2 * N), 2 * N)
    #         n   N  q      Q  qKS      baseKS baseG   baseR
    params = (24, N, 2 * N, Q, 1 << 14, 32,    1 << 7, 32)
    o = orc.Oracle(method=orc.GINX, custom=params)
    o.keygen(2024)
    c = bce.BinFHEContext(method=bce.GINX, custom=params)
    assert o.params == c.params and o.params["dG"] == 4 and o.params["q"] == 2 * N
    assert bce.forward_mfma_tables(Q, N, 7, 4)[0] == 1               # the arithmetic would allow it: the odd factor refuses
    assert c.forward_transforms_per_step() == 6 and c.forward_units() == 0 and c.forward_mfma() == 0
    c.KeyGen(2024)
    cases, idx = [], 40
    for gate in range(6):
        for a in (0, 1):
            for b in (0, 1):
                cases.append((gate, a, b, o.encrypt(a, idx), o.encrypt(b, idx + 1)))
                idx += 2
    nb = len(cases)
    c.pool_reserve(3 * nb)
    c.lwe_write(np.arange(2 * nb, dtype=np.uint32), np.concatenate([np.stack([ca, cb]) for (_, _, _, ca, cb) in cases]))
    descs = [(g, 2 * i, 2 * i + 1, 2 * nb + i) for i, (g, _, _, _, _) in enumerate(cases)]
    acc, lweN, ks = c.debug_eval_stages(descs)
    out = c.lwe_read(np.arange(2 * nb, 3 * nb, dtype=np.uint32))
    for i, (g, a, b, ca, cb) in enumerate(cases):
        r_acc = o.blind_rotate(g, o.gate_prep(g, ca, cb))
        assert np.array_equal(acc[i], r_acc), "accumulator differs, case %d" % i
        r_lweN = o.extract_modswitch(r_acc)
        assert np.array_equal(lweN[i], r_lweN)
        r_ks = o.keyswitch(r_lweN)
        assert np.array_equal(ks[i], r_ks)
        assert np.array_equal(out[i], o.modswitch_final(r_ks))
        assert o.decrypt(out[i]) == [a | b, a & b, 1 - (a | b), 1 - (a & b), a ^ b, 1 - (a ^ b)][g]
    o.close()
    c.close()
