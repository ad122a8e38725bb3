"""What a Clock() runs is decided by ONE rule, resolve_mode() of csrc/run_mode.hpp, and that rule answers what the commit
before it answered: no GPU.

tests/golden/circuit_mode_pins.json was written by tests/golden/make_circuit_mode_pins.py against that commit's library:
one row per combination of the mode setters (plaintext x encrypted x verify x batched x relevel x XOR choice x dataflow x
dataflow-shared x graph x device-verify x gate sharding x engine), with the four ...Active() answers, the slot stride, the
number of steps and the number of dataflow tasks.  Here every row, the ones recorded with an engine included, goes through
the pure function (bce_circuit_resolve_mode), and the rows without an engine are replayed on a real Circuit."""
import importlib.util
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_circuit_mode_pins", os.path.join(GOLDEN, "make_circuit_mode_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def resolve_inputs(gen, r):
    """the argument of bce_circuit_resolve_mode for a recorded row: the flags the circuit reported, the requested choices,
    and the four facts (engine, bce_dag_supported, gate sharding, a task list exists)"""
    engine = gen.ENGINES[r["engine"]]
    return (r["inputs"] & ~7 | r["plaintext"] | r["encrypted"] << 1 | r["verify"] << 2 | (engine != "none") << 11
            | (engine == "dag") << 12 | r["sharded"] << 13 | (r["n_tasks"] > 0) << 14)


def test_the_rule_answers_every_recorded_row(bce, gen):
    pins = gen.load()
    assert pins["columns"] == gen.COLUMNS
    rows = pins["table_host"] + pins["table_gpu"]
    # no axis may drop out: the full product, every point once
    assert len(rows) >= gen.AXES * len(gen.ENGINES) == 12288
    assert {(r[0], r[1], r[2]) for r in rows} == {(i, e, s) for e in range(len(gen.ENGINES)) for i, s in gen.points()}
    differ = []
    for row in rows:
        r = dict(zip(gen.COLUMNS, row))
        out = bce.circuit_resolve_mode(resolve_inputs(gen, r))
        got = (int(out >> 2 & 3 == 2), out >> 6 & 1, out >> 5 & 1, out >> 4 & 1)
        want = (r["xor_shared_active"], r["dataflow_active"], r["graph_active"], r["device_verify_active"])
        if got != want or gen.mode_key(row)[:2] != (out & 3, out >> 2 & 3):
            differ.append((row, got, out))
    assert not differ, "%d of %d rows differ, first: %s" % (len(differ), len(rows), differ[:3])


def test_a_circuit_without_engine_answers_the_recorded_rows(bce, gen):
    pins = gen.load()
    assert len(pins["table_host"]) == gen.AXES
    got = gen.table(bce, "none")
    differ = [(w, g) for w, g in zip(pins["table_host"], got) if w != g]
    assert len(got) == len(pins["table_host"]) and not differ, "%d rows differ, first (recorded, now): %s" % (len(differ), differ[:3])


def test_every_mode_of_the_table_has_a_clock_record(bce, gen):
    """the Clock() records (tests/test_gpu_circuit_modes.py replays them) cover every mode the rule reaches with an engine"""
    pins = gen.load()
    points = gen.clock_points(pins["table_gpu"])
    assert [p[1] for p in points] == [c["inputs"] for c in pins["clocks"]]
    rows = {(r[0], r[1], r[2]): r for r in pins["table_gpu"]}
    modes = {bce.circuit_resolve_mode(resolve_inputs(gen, dict(zip(gen.COLUMNS, r)))) for r in pins["table_gpu"] if r[1] == gen.ENGINES.index("dag")}
    clocked = {bce.circuit_resolve_mode(resolve_inputs(gen, dict(zip(gen.COLUMNS, rows[(i, gen.ENGINES.index("dag"), 0)])))) for _, i in points}
    assert clocked == modes and len(modes) == len({k for k, _ in points}) == 36
