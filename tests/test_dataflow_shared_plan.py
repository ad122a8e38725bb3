"""Host side of setDataflowShared without a GPU: with setXorShared + setDataflow + setDataflowShared the task list (what
bce_dag_create_pairs receives) holds a PAIR(OR, NAND) task and an AND per XOR.  It must be a valid SSA DAG in topological
order in which a pair writes two adjacent temporaries, and executed in plaintext in random dependency-respecting orders --
whatever order the device's workgroups pick -- every gate register must hold the netlist's value.  Pair semantics:
tests/pair_model.py.  Without the new setter the two options together keep giving the step schedule."""
import os
import random

import pytest

import pair_model as pm
from conftest import CIRCUITS
from test_random_circuits import random_netlist

PAIR_WORD = pm.PAIR(pm.OR, pm.NAND)


def _writes(t):
    return (t[3], t[3] + 1) if t[0] >> 8 else (t[3],)


def _check_ssa_and_run(tasks, prio, live, n_wires, stride, rnd):
    """validates the list, then executes it in a random topological order; live: slot -> bit of inputs and constants"""
    assert len(tasks) == len(prio) and all(0 <= p < 4 for p in prio)
    writer = {}
    for i, t in enumerate(tasks):
        op, a, b = t[0], t[1], t[2]
        if op >> 8:
            assert op == PAIR_WORD and t[3] >= n_wires and t[3] + 1 < stride, "a pair writes two adjacent temporaries"
        else:
            assert op in (pm.AND, pm.OR)
        for x in (a, b):
            assert x in writer or x in live, "task %d reads slot %d nobody defines before it" % (i, x)
        for o in _writes(t):
            assert o not in writer and o not in live, "slot %d written twice" % o
            writer[o] = i
    deps = [{writer[x] for x in (t[1], t[2]) if x in writer} for t in tasks]
    assert all(j < i for i, d in enumerate(deps) for j in d), "not in topological order"
    cons = [[] for _ in tasks]
    for i, d in enumerate(deps):
        for j in d:
            cons[j].append(i)           # a consumer of both outputs of a pair depends on it once
    val = dict(live)
    left = [len(d) for d in deps]
    ready = [i for i, n in enumerate(left) if n == 0]
    done = 0
    while ready:
        i = ready.pop(rnd.randrange(len(ready)))
        op, a, b, out, n0, n1 = tasks[i]
        x, y = val[a] ^ n0, val[b] ^ n1
        val[out] = pm.truth(op & 0xFF, x, y)
        if op >> 8:
            val[out + 1] = pm.truth((op >> 8) - 1, x, y)
        done += 1
        for c in cons[i]:
            left[c] -= 1
            if left[c] == 0:
                ready.append(c)
    assert done == len(tasks), "dependency cycle or unreachable task"
    return val


def _register_values(text, flat):
    """value of every REGISTER of a random_netlist text (one register per EQ / gate output, in file order; EQW aliases)"""
    wire = {i: (i, b) for i, b in enumerate(flat)}
    reg, regval, consts = len(flat), dict(enumerate(flat)), {}
    for l in text.splitlines()[4:]:
        tk = l.split()
        if not tk:
            continue
        op = tk[-1]
        if op in ("XOR", "AND"):
            a, b, o = int(tk[2]), int(tk[3]), int(tk[4])
            v = wire[a][1] ^ wire[b][1] if op == "XOR" else wire[a][1] & wire[b][1]
            wire[o] = (reg, v); regval[reg] = v; reg += 1
        elif op == "INV":
            wire[int(tk[3])] = (reg, 1 - wire[int(tk[2])][1]); regval[reg] = 1 - wire[int(tk[2])][1]; reg += 1
        elif op == "EQ":
            wire[int(tk[3])] = (reg, int(tk[2])); regval[reg] = consts[reg] = int(tk[2]); reg += 1
        elif op == "EQW":
            wire[int(tk[3])] = wire[int(tk[2])]
        else:
            m = int(tk[1])
            a = [int(x) for x in tk[2:2 + 2 * m]]
            for k in range(m):
                v = wire[a[k]][1] & wire[a[m + k]][1]
                wire[int(tk[2 + 2 * m + k])] = (reg, v); regval[reg] = v; reg += 1
    return reg, regval, consts


def _shared_dataflow(bce, path, new_flag=True):
    c = bce.Circuit()
    c.ReadBristol(path, new_flag=new_flag)
    c.setXorShared(True)
    c.setDataflow(True)
    return c


@pytest.mark.parametrize("seed", range(10))
def test_pair_task_list_is_a_valid_ssa_dag_and_order_independent(bce, tmp_path, seed):
    rnd = random.Random(4200 + seed)
    text, in_w, out_w, evaluate = random_netlist(rnd, rnd.randint(10, 150))
    path = tmp_path / "rand.txt"
    path.write_text(text)
    n_xor = sum(1 for l in text.splitlines() if l.endswith(" XOR"))
    c = _shared_dataflow(bce, str(path))
    assert c.xorSharedActive() and c.dataflow_plan() == ([], [])          # without the setter: the step schedule, as ever
    ref_hash = c.plan_hash()
    c.setDataflowShared(True)
    assert c.xorSharedActive() and not c.dataflowActive()                 # no engine: the plan exists, the GPU path cannot run
    assert c.plan_hash() != ref_hash
    tasks, prio = c.dataflow_plan()
    info = c.info()
    W, stride = info["n_wires"], info["slot_stride"]
    pairs = [t for t in tasks if t[0] >> 8]
    assert len(pairs) == n_xor and len(tasks) == info["n_bootstraps"] == sum(c.relevel_steps())
    assert sorted(t[3] for t in pairs) == [W + 2 * x for x in range(n_xor)] and stride >= W + 2 * n_xor
    for t in pairs:                                                       # each pair is followed by the AND of its two outputs
        ands = [u for u in tasks if not u[0] >> 8 and {u[1], u[2]} == {t[3], t[3] + 1}]
        assert len(ands) == 1 and ands[0][0] == pm.AND and ands[0][3] < W and ands[0][4:] == (0, 0)
        assert prio[tasks.index(ands[0])] == prio[tasks.index(t)]
    ins = [[rnd.randint(0, 1) for _ in range(w)] for w in in_w]
    flat = [b for bus in ins for b in bus]
    n_regs, regval, consts = _register_values(text, flat)
    assert n_regs == W
    live = dict(enumerate(flat))
    live.update(consts)
    gate_regs = [t[3] for t in tasks if t[3] < W]
    assert len(gate_regs) == len(tasks) - n_xor
    for trial in range(3):
        val = _check_ssa_and_run(tasks, prio, live, W, stride, random.Random(seed * 10 + trial))
        for r in gate_regs:
            assert val[r] == regval[r], "register %d: dataflow order gives %d, netlist says %d" % (r, val[r], regval[r])
    c.Reset(); c.setPlaintext(True); c.setEncrypted(False); c.SetInput(ins)
    assert c.Clock() == evaluate(ins)
    c.close()


def test_pair_task_list_of_aes_expanded(bce):
    c = _shared_dataflow(bce, os.path.join(CIRCUITS, "AES-expanded.txt"), new_flag=False)
    assert c.xorSharedActive() and c.dataflow_plan()[0] == [] and c.info()["n_bootstraps"] == 46090
    c.setDataflowShared(True)
    tasks, prio = c.dataflow_plan()
    info = c.info()
    assert len(tasks) == 46090 == info["n_bootstraps"] and sum(1 for t in tasks if t[0] >> 8) == 20325
    assert all(t[0] == PAIR_WORD for t in tasks if t[0] >> 8)
    assert info["slot_stride"] == info["n_wires"] + 2 * 20325
    written = [o for t in tasks for o in _writes(t)]
    assert len(set(written)) == len(written) == 46090 + 20325 and max(written) < info["slot_stride"]
    level = {}
    for t in tasks:
        l = 1 + max(level.get(t[1], 0), level.get(t[2], 0))
        for o in _writes(t):
            level[o] = l
    deepest = max(level.values())
    assert deepest == 416 == info["n_relevel_steps"]
    assert 0 in prio and max(prio) <= 3 and any(p == 0 and level[t[3]] == deepest for t, p in zip(tasks, prio))
    c.setDataflowShared(False)
    assert c.dataflow_plan() == ([], []) and c.xorSharedActive()
    c.close()


def test_the_setter_is_an_opt_in_and_fixed_at_setinput(bce):
    c = bce.Circuit()
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setDataflowShared(True)                       # alone it changes nothing
    assert c.dataflow_plan() == ([], []) and sum(c.relevel_steps()) == 13
    c.setDataflow(True)
    assert len(c.dataflow_plan()[0]) == 13 and not any(t[0] >> 8 for t in c.dataflow_plan()[0])
    c.setXorShared(True)
    tasks, _ = c.dataflow_plan()
    assert len(tasks) == 10 == sum(c.relevel_steps()) and sum(1 for t in tasks if t[0] >> 8) == 3
    c.setVerify(True)                               # a host-side verify pass: the reference lowering, on both schedules
    assert not c.xorSharedActive() and len(c.dataflow_plan()[0]) == 13
    c.setVerify(False)
    assert c.xorSharedActive() and len(c.dataflow_plan()[0]) == 10
    c.Reset()
    c.setPlaintext(True)
    c.SetInput([[1, 1], [0, 1]])
    with pytest.raises(bce.BceError) as e:
        c.setDataflowShared(False)
    assert e.value.code == bce.ERR_STATE and "before SetInput" in str(e.value)
    c.setDataflowShared(True)                       # no change: accepted
    assert len(c.dataflow_plan()[0]) == 10
    o = c.Clock()[0]
    assert o[0] + 2 * o[1] + 4 * o[2] == 5
    c.Reset()
    c.setDataflowShared(False)                      # Reset() lifts it
    assert c.dataflow_plan() == ([], []) and c.xorSharedActive()
    c.close()
