#!/usr/bin/env python3
"""What two gates from one blind rotation buy: wall time of Circuit.Clock() with

    reference   XOR = (a AND !b) OR (!a AND b): three blind rotations (the default)
    shared      setXorShared: XOR = AND(OR(a, b), NAND(a, b)), the OR and the NAND from one blind rotation (a BCE_PAIR
                descriptor, whose tail runs twice): two blind rotations

for AES-expanded at STD128_OPT GINX K = 32 and adder_64bit at K = 64, on the bootstrap-depth schedule, step by step.  The
lowering is chosen before SetInput, so each leg has a Circuit and a context of its own (same key seed, same inputs) in ONE
process on one device, and the two alternate round by round (a warm-up round first, then --reps timed rounds).  Every Clock()
ends in a device synchronise; outputs are compared with the known answers after every run.  Per leg: steps, blind rotations
and the per-kernel device times of timing() of the last round.

    python3 tools/xor_shared_cost.py [--reps 3] [--out profiles/xor_shared_cost.json] [--aes-k 32] [--adder-k 64]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
bce = importlib.import_module("openfhe-boolean-circuit-evaluator_amd")
import kat  # noqa: E402

LEGS = ("reference", "shared")


def measure(ccs, name, path, K, cases, reps):
    circ = {}
    for leg in LEGS:
        c = bce.Circuit(ccs[leg])
        c.ReadBristol(path)
        c.setInstances(K)
        c.setXorShared(leg == "shared")
        c.Reset()
        c.setEncrypted(True)
        assert c.xorSharedActive() == (leg == "shared")
        for k in range(K):
            c.SetInput(cases[k % len(cases)][0], instance=k)
        circ[leg] = c
    wall = {leg: [] for leg in LEGS}
    per_leg = {}
    for rnd in range(reps + 1):       # round 0 warms up (plan upload, first launches)
        for leg in LEGS:
            c, cc = circ[leg], ccs[leg]
            if rnd:
                c.Rearm()
            cc.timing_reset()
            t0 = time.perf_counter()
            c.Clock()
            dt = time.perf_counter() - t0
            for k in range(K):
                assert c.Outputs(k)[0] == cases[k % len(cases)][1], "%s, %s: instance %d is wrong" % (name, leg, k)
            st, t = c.stats(), cc.timing()
            if rnd:
                wall[leg].append(dt)
            per_leg[leg] = {"steps": st["levels"], "launches": st["sublaunches"], "blind_rotations": st["bootstraps"],
                            "blind_rotations_per_instance": st["bootstraps"] // K,
                            "blind_rotate_ms": t["blind_rotate_ms"], "tail_ms": t["tail_ms"], "fused_tail_launches": t["fused_tail_launches"],
                            "by_kernel": [k for k in t["by_kernel"] if k["launches"]]}
            print("%-12s round %d %-9s %8.3f s  (%d steps, %d blind rotations)" % (name, rnd, leg, dt, st["levels"], st["bootstraps"]), flush=True)
    med = {leg: statistics.median(wall[leg]) for leg in LEGS}
    res = {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps, "wall_s": wall,
           "median_wall_s": med, "spread_s": {leg: max(wall[leg]) - min(wall[leg]) for leg in LEGS}, "per_leg": per_leg,
           "clock_ratio_shared_over_reference": med["shared"] / med["reference"],
           "blind_rotation_ratio_shared_over_reference": per_leg["shared"]["blind_rotations"] / per_leg["reference"]["blind_rotations"],
           "device_ms_ratio_shared_over_reference": (per_leg["shared"]["blind_rotate_ms"] + per_leg["shared"]["tail_ms"])
                                                    / (per_leg["reference"]["blind_rotate_ms"] + per_leg["reference"]["tail_ms"])}
    assert per_leg["shared"]["steps"] == per_leg["reference"]["steps"]
    for c in circ.values():
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--aes-k", type=int, default=32)
    ap.add_argument("--adder-k", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xor_shared_cost.json"))
    args = ap.parse_args()
    ccs = {}
    for leg in LEGS:
        ccs[leg] = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
        ccs[leg].KeyGen(0x0FE5EED)
    results = []
    if args.adder_k:
        results.append(measure(ccs, "adder_64bit", os.path.join(kat.CIRCUITS, "adder_64bit.txt"), args.adder_k,
                               [kat.adder_case(t, 64) for t in range(8)], args.reps))
    if args.aes_k:
        vecs = [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]
        results.append(measure(ccs, "AES-expanded", os.path.join(kat.CIRCUITS, "AES-expanded.txt"), args.aes_k, vecs, args.reps))
    doc = {"what": "wall time of Circuit.Clock() with the reference XOR lowering and with setXorShared, the two alternating round by "
                   "round in one process on one device (tools/xor_shared_cost.py); medians over `reps` timed rounds after one "
                   "warm-up round; per-kernel device times of the last round",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        print("%s K=%d: reference %.3f s, shared %.3f s: Clock() x%.4f, blind rotations x%.4f, device kernel time x%.4f" % (
            r["circuit"], r["instances"], r["median_wall_s"]["reference"], r["median_wall_s"]["shared"],
            r["clock_ratio_shared_over_reference"], r["blind_rotation_ratio_shared_over_reference"], r["device_ms_ratio_shared_over_reference"]))


if __name__ == "__main__":
    main()
