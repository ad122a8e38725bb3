"""AP key addressing of the split-transform family at 2 GiB and 4 GiB.

k_blind_rotate_lat and k_bootstrap_dag read the AP key through ONE buffer resource of 0x7FFFFFFF records with a wave-uniform
32-bit byte offset ((i baseR + a0) dR + k) * 64 KiB per step; the wave-per-transform family (BCE_VARIANT=1) adds the same
index to a 64-bit pointer.  No tabulated set comes near 2 GiB on that shape (N = 1024, four digits), bce_ctx_create_custom
takes any n.  Here n is chosen from bce_bsk_words() so that the key is just below 2^31 bytes, exactly 2^31, exactly 2^32 and one
LWE coefficient past 2^32 (n = 511, 512, 1024, 1025 at q = 1024, baseR = 32).  Keys come from the device KeyGen(seed) alone (no
oracle key, no export: 4 GiB of words), so the contexts of one size hold the same key.  The ciphertexts have a trivial mask
but for coefficients 0, n - 2 and n - 1, whose digits are at their maxima at n - 2 and n - 1: the steps read the lowest and the
highest RGSW ciphertexts of the key.

Asserted: every pool word of every output is the same under BCE_VARIANT=1, 2, 3 and on the persistent kernel (where the
context has one), and every output decrypts to the truth table.  kernel_class grants the split-transform family to an AP
context only while its key stays below SPLIT_AP_KEY_BYTES = 2^31; from there on every BCE_VARIANT runs the wave-per-transform
kernel and there is no persistent kernel, which is asserted from timing()["by_kernel"] and bce_dag_supported().

What the split-transform kernels did with these keys before that rule (MI355X, one run per size): below 2^31 every word
agreed; at exactly 2^31 the 16 b words of the outputs differed and no gate decrypted (the wave-uniform offset takes part in
the range check of the buffer load, so the last 16 bytes of the key read as zeros); at 2^32 and past it 16,392 and 16,404 of
the 16,416 words differed.

No run here can fault: the per-thread offset stays below 16 KiB under a record count of 2 GiB, and every wrapped 32-bit
offset lands inside the allocation.  A wrong offset shows as wrong words.
"""
import numpy as np
import pytest

import test_gpu_worst_case as base
import worst_case as wc

gpu = pytest.mark.gpu
SPLIT_AP_KEY_BYTES = 1 << 31              # kSplitApKeyBytes (csrc/kernels.hpp): the split-transform family takes AP keys below it
SIZES = ("below 2^31", "2^31", "2^32", "past 2^32")
SELECTORS = ("BCE_VARIANT", "BCE_FWD_MFMA", "BCE_FWD_UNITS", "BCE_FOLD", "BCE_FP64", "BCE_FUSE_TAIL", "BCE_OCCUPANCY")
WAVE = 0                                  # BCE_BR_WAVE_PER_TRANSFORM


def _params(orc, n):
    return base._custom(n, 1024, 1024, base._q27(orc.lib(), 1024), 1 << 7, qKS=1 << 14, baseKS=32, baseR=32)


def _context(bce, orc, monkeypatch, n, env):
    for k in SELECTORS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return bce.BinFHEContext(method=bce.AP, custom=_params(orc, n))


def _key_bytes(bce, c):
    return int(bce.lib().bce_bsk_words(c.h)) * 4


def _sizes(bce, orc, monkeypatch, env=None):
    """{size name: n}, derived from bce_bsk_words of a context of one coefficient: the key grows by the same amount per
    coefficient"""
    c = _context(bce, orc, monkeypatch, 1, env or {})
    per = _key_bytes(bce, c)
    c.close()
    assert (1 << 31) % per == 0
    n31, n32 = (1 << 31) // per, (1 << 32) // per
    return {"below 2^31": n31 - 1, "2^31": n31, "2^32": n32, "past 2^32": n32 + 1}, per


def _inputs(q, s, n):
    """[(gate, bit0, bit1, ct1, ct2)]: ct1 encrypts bit0 without noise under s with a mask that is zero but for coefficient 0
    (-a = 1: digit 1 at position 0, the lowest key row that is ever read) and coefficients n - 2 and n - 1 (-a = q - 1: both
    digits 31, the highest rows); ct2 is the trivial encryption of bit1"""
    a = np.zeros(n, dtype=np.int64)
    a[0], a[n - 2], a[n - 1] = q - 1, 1, 1
    out = []
    for gate in wc.PLAIN:
        for b0 in (0, 1):
            for b1 in (0, 1):
                ct1 = np.zeros(n + 1, dtype=np.uint64)
                ct1[:n] = a
                ct1[n] = (int(np.dot(a, s.astype(np.int64))) + b0 * (q // 4)) % q
                ct2 = np.zeros(n + 1, dtype=np.uint64)
                ct2[n] = b1 * (q // 4)
                out.append((gate, b0, b1, ct1, ct2))
    return out


def _truth(gate, a, b):
    return [a | b, a & b, 1 - (a | b), 1 - (a & b)][gate]


def _run(bce, orc, monkeypatch, n, env, seed, dag=False):
    """KeyGen(seed) on a fresh context under `env`, the 16 gates in one launch (dag: as one run of the persistent kernel):
    {"pool": output rows, "bits": decryptions, "wave": launches counted for the wave-per-transform kernel, "launches": all
    blind-rotation launches, "dag_supported", "key_bytes", "transforms": forward transforms per step}"""
    c = _context(bce, orc, monkeypatch, n, env)
    try:
        res = {"dag_supported": int(c.dag_supported()), "key_bytes": _key_bytes(bce, c), "transforms": c.forward_transforms_per_step()}
        if dag and not res["dag_supported"]:
            return res
        c.KeyGen(seed)
        s, _ = c.export_sk()
        q = c.params["q"]
        cases = _inputs(q, s, n)
        nb = len(cases)
        c.pool_reserve(3 * nb)
        c.lwe_write(np.arange(2 * nb, dtype=np.uint32), np.concatenate([np.stack([x[3], x[4]]) for x in cases]))
        descs = [(x[0], 2 * i, 2 * i + 1, 2 * nb + i) for i, x in enumerate(cases)]
        before = [k["launches"] for k in c.timing()["by_kernel"]]
        if dag:
            g = c.dag_create(descs)
            c.dag_run(g)
            c.synchronize()
            last = c.dag_last_run()
            c.dag_destroy(g)
            assert last["done"] == nb and last["abort"] == 0, last
        else:
            c.EvalGates(descs)
            c.synchronize()
        after = [k["launches"] for k in c.timing()["by_kernel"]]
        outs = np.arange(2 * nb, 3 * nb, dtype=np.uint32)
        res.update(pool=c.lwe_read(outs), bits=[int(v) for v in c.Decrypt(outs)], wave=after[WAVE] - before[WAVE],
                   launches=sum(after) - sum(before), want=[_truth(x[0], x[1], x[2]) for x in cases])
        return res
    finally:
        c.close()


FAMILIES = (("BCE_VARIANT=2", {"BCE_VARIANT": "2"}, False), ("BCE_VARIANT=3", {"BCE_VARIANT": "3"}, False),
            ("default selection", {}, False), ("persistent kernel", {}, True))


def compare_families(bce, orc, monkeypatch, size, seed=4101):
    """(n, key bytes, reference run under BCE_VARIANT=1, [(family, run, words that differ from the reference)])"""
    n = _sizes(bce, orc, monkeypatch)[0][size]
    ref = _run(bce, orc, monkeypatch, n, {"BCE_VARIANT": "1"}, seed)
    rows = []
    for name, env, dag in FAMILIES:
        r = _run(bce, orc, monkeypatch, n, env, seed, dag)
        rows.append((name, r, int((r["pool"] != ref["pool"]).sum()) if "pool" in r else None))
    return n, ref["key_bytes"], ref, rows


@gpu
def test_sizes_are_derived_from_the_key_word_count(bce, orc, monkeypatch):
    """an RGSW ciphertext of the shape is 64 KiB, folded key or plain: n = 511, 512, 1024, 1025"""
    for env in ({}, {"BCE_FOLD": "0"}):
        sizes, per = _sizes(bce, orc, monkeypatch, env)
        assert per == 32 * 2 * 65536 and sizes == {"below 2^31": 511, "2^31": 512, "2^32": 1024, "past 2^32": 1025}, (env, per, sizes)


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_ap_key_addressing_at_2_and_4_gib(bce, orc, monkeypatch, size):
    n, key_bytes, ref, rows = compare_families(bce, orc, monkeypatch, size)
    split = key_bytes < SPLIT_AP_KEY_BYTES
    print("n = %d, key %d bytes (%s the bound): BCE_VARIANT=1 decrypts %s" % (n, key_bytes, "below" if split else "not below", ref["bits"] == ref["want"]))
    assert ref["wave"] == ref["launches"] == 1 and ref["bits"] == ref["want"], ("BCE_VARIANT=1", ref["bits"], ref["want"])
    bad = []
    for name, r, differ in rows:
        print("  %s: dag_supported %d, transforms per step %d, launches %s (wave-per-transform %s), words that differ %s"
              % (name, r["dag_supported"], r["transforms"], r.get("launches"), r.get("wave"), differ))
        if r["dag_supported"] != int(split):
            bad.append("%s: bce_dag_supported() = %d for a key of %d bytes" % (name, r["dag_supported"], key_bytes))
        if "pool" not in r:
            continue                                # the persistent kernel from the bound on: there is none, asserted above
        if differ:
            bad.append("%s: %d pool words differ from BCE_VARIANT=1" % (name, differ))
        if r["bits"] != r["want"]:
            bad.append("%s: decrypts to %s, truth table %s" % (name, r["bits"], r["want"]))
        if name != "persistent kernel" and (r["wave"] == r["launches"]) == split:
            bad.append("%s: %d of %d launches on the wave-per-transform kernel for a key of %d bytes" % (name, r["wave"], r["launches"], key_bytes))
    assert not bad, "\n".join(bad)


@gpu
def test_split_family_is_granted_up_to_the_key_bound_only(bce, orc, monkeypatch):
    """both sides of the bound, creation only: one coefficient below it the split-transform family (folded key: 6 forward
    transforms per step; a persistent kernel), at the bound the wave-per-transform family (plain key: 8; none) under every
    selector; GINX keys of the same n stay far below the bound and keep the split family"""
    sizes, per = _sizes(bce, orc, monkeypatch)
    at = SPLIT_AP_KEY_BYTES // per - 1
    seen = {}
    for n in (at, at + 1):
        for v in ("0", "1", "2", "3"):
            c = _context(bce, orc, monkeypatch, n, {"BCE_VARIANT": v})
            seen[(n, v)] = (int(c.dag_supported()), c.forward_transforms_per_step(), c.lazy_arithmetic())
            c.close()
    for v in ("0", "2", "3"):
        assert seen[(at, v)] == (1, 6, 1) and seen[(at + 1, v)] == (0, 8, 1), seen
    assert seen[(at, "1")] == seen[(at + 1, "1")] == (0, 8, 1), seen
    monkeypatch.delenv("BCE_VARIANT")
    g = bce.BinFHEContext(method=bce.GINX, custom=_params(orc, at + 1))
    assert (int(g.dag_supported()), g.forward_transforms_per_step()) == (1, 6)
    g.close()
