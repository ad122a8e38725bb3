"""The mode table and the Clock() of every mode, on real contexts, against the commit before csrc/run_mode.hpp.

tests/golden/circuit_mode_pins.json (tests/golden/make_circuit_mode_pins.py, tests/test_circuit_modes.py): the rows recorded
with an engine are replayed on Circuits of the same two contexts -- no keys, no Clock() -- and the Clock() records are run
again: adder_2bit.out, K = 2, STD128_OPT / GINX, fixed key seed, encryption seed and inputs, one wrong input ciphertext
where verify is on; one Clock() and one Rearm() + Clock() per mode.  Outputs, statistics, counts, the device's check
report, the "Bad ..." lines and every register of the pool (SHA-256) must be the recorded ones: no tolerance."""
import importlib.util
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_circuit_mode_pins", os.path.join(GOLDEN, "make_circuit_mode_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("engine", ["dag", "nodag"])
def test_circuits_with_an_engine_answer_the_recorded_rows(bce, gen, engine):
    want = [r for r in gen.load()["table_gpu"] if r[1] == gen.ENGINES.index(engine)]
    assert len(want) == gen.AXES
    cc = gen.context(bce, engine)
    try:
        got = gen.table(bce, engine, cc)
    finally:
        cc.close()
    differ = [(w, g) for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not differ, "%d rows differ, first (recorded, now): %s" % (len(differ), differ[:3])


def test_clock_of_every_mode_is_the_recorded_one(bce, gen):
    pins = gen.load()
    assert [p[1] for p in gen.clock_points(pins["table_gpu"])] == [c["inputs"] for c in pins["clocks"]]
    cc = gen.context(bce, "dag", keys=True)      # one keyed context for all records
    differ = []
    try:
        for want in pins["clocks"]:
            got = gen.clock_record(bce, cc, want["inputs"])
            if got != want:
                differ.append((want, got))
                print(want["inputs"], [(k, w[k], g[k]) for w, g in zip(want["clocks"], got["clocks"]) for k in w if w[k] != g[k]])
    finally:
        cc.close()
    assert not differ, "%d of %d records differ, first (recorded, now): %s" % (len(differ), len(pins["clocks"]), differ[:1])
