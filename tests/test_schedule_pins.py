"""The host schedules are pinned to the ones the commit before the schedule module (csrc/schedule.cpp) built: no GPU.

tests/golden/schedule_pins.json was written by tests/golden/make_schedule_pins.py against that commit's library.  For every
case of the cross product (circuit x K x balance x xor_fast x dataflow x locality x world x rank, gate sharding, explicit
capacities) it covers plan_hash(), the slot stride, the number of steps and the SHA-256 of relevel_steps(), of
relevel_publications() and of dataflow_plan(); one digest per (circuit, K, balance, xor_fast, dataflow) group holds the 28
(locality, world, rank) cases of the group.  Here the same digests are recomputed with this tree's library, and every case
must also pass check_relevel()."""
import importlib.util
import json
import os

from conftest import GOLDEN


def test_schedules_equal_the_pinned_ones(bce):
    spec = importlib.util.spec_from_file_location("make_schedule_pins", os.path.join(GOLDEN, "make_schedule_pins.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.FIXTURE) as f:
        pinned = json.load(f)
    seen, cases, differ = set(), 0, []
    for key, digest, n in gen.groups(bce, check=True):
        seen.add(key)
        cases += n
        if pinned["groups"].get(key) != digest:
            differ.append(key)
    assert not differ, "%d of %d groups differ from the pinned schedules, first: %s" % (len(differ), len(seen), differ[:5])
    assert seen == set(pinned["groups"]) and cases == pinned["cases"] == 11088
