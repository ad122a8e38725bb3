"""Writes tests/golden/schedule_pins.json: digests of the host schedules of a PARENT commit's library, which
tests/test_schedule_pins.py recomputes with this tree's library.  No GPU: circuits without an engine, explicit capacities.

    python tests/golden/make_schedule_pins.py <checkout of the parent commit, built>

Never run it against this tree's own library: the fixture would then pin nothing.

A case is (circuit, xor_fast, dataflow, balance, K, locality, world, rank) under gate sharding.  Its record holds
plan_hash(), info()["slot_stride"], info()["n_relevel_steps"] and the SHA-256 of relevel_steps(), of relevel_publications()
and of dataflow_plan().  The 28 (locality, world, rank) records of one (circuit, xor_fast, dataflow, balance, K) group are
hashed together, and the fixture stores that one digest per group, so that it stays a few tens of KB for 11,088 cases.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
import hashlib
import importlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
CIRCUITS = os.path.join(HERE, "circuits")
PKG = "openfhe-boolean-circuit-evaluator_amd"
FIXTURE = os.path.join(HERE, "schedule_pins.json")

FILES = [("adder_2bit.out", "file"), ("parity.out", "file"), ("adder_64bit.txt", "bristol"), ("md5.txt", "bristol"),
         ("sha256_new.txt", "bristol_new"), ("AES-expanded.txt", "bristol")]
RANDOM_SEEDS = range(5)
KS = (1, 3, 32)
BALANCES = ((False, 256, 512), (True, 256, 512), (True, 1, 1))      # capacities always explicit: no device is asked
WORLDS = (1, 2, 3, 8)


def circuits(tmp_dir):
    """(name, loader) of every pinned circuit; random netlists are written under tmp_dir"""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    from test_random_circuits import random_netlist
    out = []
    for name, kind in FILES:
        path = os.path.join(CIRCUITS, name)
        if kind == "file":
            out.append((name, lambda c, p=path: c.ReadFile(p)))
        else:
            out.append((name, lambda c, p=path, nf=(kind == "bristol_new"): c.ReadBristol(p, new_flag=nf)))
    for seed in RANDOM_SEEDS:
        rnd = random.Random(7100 + seed)
        text = random_netlist(rnd, rnd.randint(10, 150))[0]
        path = os.path.join(tmp_dir, "random_%d.txt" % seed)
        with open(path, "w") as f:
            f.write(text)
        out.append(("random_%d" % seed, lambda c, p=path: c.ReadBristol(p, new_flag=True)))
    return out


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def _raw(fn, h, ctype, *more):
    """SHA-256 of what a two-call C accessor (count, then fill) returns: the buffers' bytes, not Python lists (the task
    list of AES-expanded has 66 k descriptors and there are a thousand cases of it)"""
    n = C.c_uint32(0)
    assert fn(h, *([None] * (1 + len(more))), 0, C.byref(n)) == 0
    bufs = [(t * max(1, n.value))() for t in (ctype,) + more]
    assert fn(h, *bufs, n.value, C.byref(n)) == 0
    d = hashlib.sha256(str(n.value).encode())
    for t, b in zip((ctype,) + more, bufs):
        d.update(bytes(b)[:n.value * C.sizeof(t)])
    return d.hexdigest()


def case_record(bce, c):
    """what relevel_steps(), relevel_publications() and dataflow_plan() return, read through the same C accessors"""
    info = c.info()
    L = c._L
    return [c.plan_hash(), info["slot_stride"], info["n_relevel_steps"],
            _raw(L.bce_circuit_relevel_steps, c.h, C.c_uint32), _raw(L.bce_circuit_relevel_publications, c.h, C.c_uint32),
            _raw(L.bce_circuit_dataflow_plan, c.h, bce.GateDesc, C.c_uint8)]


def _unit(bce, load, name, xor_fast, dataflow, check):
    """the groups of one (circuit, xor_fast, dataflow): [(key, digest, cases)]"""
    out = []
    c = bce.Circuit()      # fresh: a task list is held only while the dataflow schedule is chosen
    load(c)
    c.setXorFast(xor_fast)
    c.setDataflow(dataflow)
    for bi, (on, lone, full) in enumerate(BALANCES):
        c.setBalance(on, lone, full)
        for K in KS:
            c.setInstances(K)
            records = []
            for locality in (True, False):
                c.setShardLocality(locality)
                for world in WORLDS:
                    for rank in range(world):
                        c.set_exchange(rank, world, 1, lambda nbytes, on_dev: 0, None, None, None, None, 0)
                        if check:
                            c.check_relevel()
                        records.append(case_record(bce, c))
            out.append(("%s|xor_fast=%d|dataflow=%d|balance=%d|K=%d" % (name, xor_fast, dataflow, bi, K), _sha(records), len(records)))
    c.close()
    return out


def groups(bce, check=False):
    """yields (key, digest, cases) per group; check=True also asserts check_relevel() for every case.  The 44 (circuit,
    xor_fast, dataflow) units are independent circuits and run on a few threads (the library calls release the GIL)."""
    bce.Circuit().close()   # loads and binds the library once, before any thread does
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        units = [(load, name, xf, df) for name, load in circuits(tmp) for xf in (False, True) for df in (False, True)]
        units.sort(key=lambda u: -os.path.getsize(os.path.join(CIRCUITS, u[1])) if os.path.exists(os.path.join(CIRCUITS, u[1])) else 0)
        for res in pool.map(lambda u: _unit(bce, *u, check), units):
            yield from res


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    sys.path.insert(0, parent)
    bce = importlib.import_module(PKG)
    if not os.path.abspath(bce.__file__).startswith(parent + os.sep):
        sys.exit("the package was not imported from %s" % parent)
    pins, n = {}, 0
    for key, digest, cases in groups(bce):
        pins[key] = digest
        n += cases
    with open(FIXTURE, "w") as f:
        json.dump({"cases": n, "groups": pins}, f, indent=0, sort_keys=True)
    print("%d cases in %d groups -> %s" % (n, len(pins), FIXTURE))
