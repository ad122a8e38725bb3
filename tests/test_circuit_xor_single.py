"""setXorSingle on the host circuit runtime, without an engine: every XOR gate as one BCE_XOR descriptor (one bootstrap of
ct1 + ct2).  Plaintext runs are untouched by the option; n_bootstraps, the step sizes and the plan hash reflect it; it is refused
together with setXorFast / setXorShared and after SetInput."""
import os

import pytest

import kat
from kat import CIRCUITS


def _read(bce, name):
    c = bce.Circuit()
    if name.endswith(".out"):
        c.ReadFile(os.path.join(CIRCUITS, name))
    else:
        c.ReadBristol(os.path.join(CIRCUITS, name))
    return c


def parity_vectors(count=16):
    """inputs and outputs of parity.out in the shape of kat.parity_case (8 bits + bit8 = 0), for more vectors than it has"""
    out = []
    for t in range(count):
        bits = [((37 * t + 11) >> i) & 1 for i in range(8)] + [0]
        odd = sum(bits) & 1
        out.append(([bits], [1 - odd, odd]))
    return out


def _plain(c, inputs):
    c.Reset()
    c.setPlaintext(True)
    c.setEncrypted(False)
    c.SetInput(inputs)
    return c.Clock()[0]


def test_plaintext_runs_are_unchanged_by_the_option(bce):
    c = _read(bce, "adder_2bit.out")
    assert not c.getXorSingle()
    c.setXorSingle(True)
    assert c.getXorSingle()
    for a in range(4):
        for b in range(4):
            o = _plain(c, [[a & 1, a >> 1], [b & 1, b >> 1]])
            assert o[0] + 2 * o[1] + 4 * o[2] == a + b
    c.close()
    p = _read(bce, "parity.out")
    p.setXorSingle(True)
    for ins, want in parity_vectors(16):
        assert _plain(p, ins) == want
    p.close()
    m = _read(bce, "AES-expanded.txt")
    m.setXorSingle(True)
    for v in [x for x in kat.AES_VECTORS if x["circuit"] == "AES-expanded"]:
        assert _plain(m, kat.aes_case(v)[0]) == kat.aes_case(v)[1]
    m.close()


@pytest.mark.parametrize("name,ref,single", [("adder_2bit.out", 13, 7), ("parity.out", None, None), ("AES-expanded.txt", 66415, 25765),
                                             ("adder_64bit.txt", 610, 380)])
def test_one_bootstrap_per_xor(bce, name, ref, single):
    c = _read(bce, name)
    c.Reset(); c.setPlaintext(True); c.setEncrypted(False)
    c.SetInput([[0] * w for w in c.buses()[0]])
    c.Clock()
    n = c.counts()
    c.Reset()
    ref_info, ref_steps, ref_hash = c.info(), c.relevel_steps(), c.plan_hash()
    assert ref_info["n_bootstraps"] == sum(ref_steps) == n["and"] + n["or"] + 3 * n["xor"] and ref in (None, ref_info["n_bootstraps"])
    c.setXorSingle(True)
    info, steps = c.info(), c.relevel_steps()
    assert info["n_bootstraps"] == sum(steps) == n["and"] + n["or"] + n["xor"] and single in (None, info["n_bootstraps"])
    assert len(steps) == info["n_relevel_steps"] <= ref_info["n_relevel_steps"]    # an XOR is one step deep, not two
    assert len(steps) < len(ref_steps) or name == "adder_64bit.txt"                # (its critical path is the AND / OR carry chain)
    assert info["slot_stride"] <= ref_info["slot_stride"]
    c.check_relevel()
    assert c.plan_hash() != ref_hash
    descs = [d for st in c.relevel_plan() for d in st]
    assert sum(1 for d in descs if d[0] == bce.XOR) == n["xor"] and all(d[0] in (bce.XOR, bce.AND, bce.OR) for d in descs)
    # the same shape as the XOR_FAST lowering: one unit per gate
    c.setXorSingle(False)
    assert c.relevel_steps() == ref_steps and c.plan_hash() == ref_hash
    c.setXorFast(True)
    assert c.relevel_steps() == steps and c.plan_hash() != ref_hash
    fast_hash = c.plan_hash()
    c.setXorFast(False)
    c.setXorSingle(True)
    assert c.plan_hash() != fast_hash
    c.setDataflow(True)
    tasks, prio = c.dataflow_plan()                    # the dataflow schedule: one task per gate, no temporaries
    assert len(tasks) == len(prio) == info["n_bootstraps"] and sum(1 for t in tasks if t[0] == bce.XOR) == n["xor"]
    assert max(max(t[1:4]) for t in tasks) < info["n_wires"]
    c.close()


def test_parity_keeps_the_negations_of_its_not_gates(bce):
    """parity.out has NOT gates in front of XORs: on the bootstrap-depth schedule they are the descriptor's flags"""
    c = _read(bce, "parity.out")
    c.setXorSingle(True)
    descs = [d for st in c.relevel_plan() for d in st]
    assert any(d[0] == bce.XOR and (d[4] or d[5]) for d in descs) or c.counts()["not"] == 0
    assert all(d[0] != bce.XNOR_FAST and d[0] != bce.XOR_FAST for d in descs)
    c.close()


def test_option_rules(bce):
    c = _read(bce, "adder_2bit.out")
    c.setXorSingle(True)
    for other in (c.setXorFast, c.setXorShared):
        with pytest.raises(bce.BceError) as e:
            other(True)
        assert e.value.code == bce.ERR_ARG
        assert c.getXorSingle() and sum(c.relevel_steps()) == 7
    c.setXorSingle(False)
    for other in (c.setXorFast, c.setXorShared):
        other(True)
        with pytest.raises(bce.BceError) as e:
            c.setXorSingle(True)
        assert e.value.code == bce.ERR_ARG and not c.getXorSingle()
        other(False)
    assert sum(c.relevel_steps()) == 13
    # not after SetInput: the slot stride depends on the lowering
    o = _plain(c, [[1, 1], [0, 1]])
    assert o[0] + 2 * o[1] + 4 * o[2] == 5
    with pytest.raises(bce.BceError) as e:
        c.setXorSingle(True)
    assert e.value.code == bce.ERR_STATE and not c.getXorSingle() and sum(c.relevel_steps()) == 13
    c.setXorSingle(False)                    # no change: accepted
    c.Reset()
    c.setXorSingle(True)
    _plain_keep = c.relevel_steps()
    c.setPlaintext(True); c.setEncrypted(False)
    c.SetInput([[1, 0], [1, 1]])
    with pytest.raises(bce.BceError) as e:
        c.setXorSingle(False)
    assert e.value.code == bce.ERR_STATE and c.getXorSingle() and c.relevel_steps() == _plain_keep
    # gate-level rounds and per-gate evaluation count the same
    c.Reset()
    c.setRelevel(False)
    assert c.info()["n_bootstraps"] == 7
    c.setBatched(False)
    assert c.info()["n_bootstraps"] == 7
    c.close()
