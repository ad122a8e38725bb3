#!/usr/bin/env python3
"""What XOR in one bootstrap buys: wall time of Circuit.Clock() with

    reference   XOR = (a AND !b) OR (!a AND b): three blind rotations in two steps (the default)
    shared      setXorShared: XOR = AND(OR(a, b), NAND(a, b)), the OR and the NAND from one blind rotation: two, in two steps
    single      setXorSingle: one BCE_XOR bootstrap of ct1 + ct2 (three-level test polynomial): one, in one step

for AES-expanded at STD128_OPT GINX K = 32 and adder_64bit at K = 64, on the bootstrap-depth schedule, step by step.  The
lowering is chosen before SetInput, so each leg has a Circuit and a context of its own (same key seed, same inputs) in ONE
process on one device, and the three alternate round by round (a warm-up round first, then --reps timed rounds).  Every Clock()
ends in a device synchronise; outputs are compared with the known answers after every run.  Per leg: steps, blind rotations
and the per-kernel device times of timing() of the last round.

The plain lowering must pay nothing for the new branch in the prologues and tails: with --parent-root DIR (a checkout of the
parent commit with its library built) the reference leg of THIS build runs against the same leg of the parent's.  One library per
process, so the two builds alternate as child processes (parent, this, parent, this, ...: --ab-rounds of each); the margin is
the spread between the parent's own repeated legs (the method of parent_comparison in profiles/dataflow_shared_cost.json).

    python3 tools/xor_single_cost.py [--reps 3] [--parent-root DIR] [--ab-rounds 2] [--only legs|parent]
                                     [--out profiles/xor_single_cost.json] [--aes-k 32] [--adder-k 64]

--only runs one half and merges it into an existing --out file (the two halves fit separate time limits).
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("reference", "shared", "single")


def load(root):
    """the package of the build under `root`; the known answers are this tree's"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import kat
    return importlib.import_module("openfhe-boolean-circuit-evaluator_amd"), kat


def measure(bce, ccs, legs, name, path, K, cases, reps):
    circ = {}
    for leg in legs:
        c = bce.Circuit(ccs[leg])
        c.ReadBristol(path)
        c.setInstances(K)
        if leg == "shared":
            c.setXorShared(True)
        if leg == "single":
            c.setXorSingle(True)
        c.Reset()
        c.setEncrypted(True)
        for k in range(K):
            c.SetInput(cases[k % len(cases)][0], instance=k)
        circ[leg] = c
    wall = {leg: [] for leg in legs}
    per_leg = {}
    for rnd in range(reps + 1):       # round 0 warms up (plan upload, first launches)
        for leg in legs:
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
    med = {leg: statistics.median(wall[leg]) for leg in legs}
    res = {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps, "wall_s": wall,
           "median_wall_s": med, "spread_s": {leg: max(wall[leg]) - min(wall[leg]) for leg in legs}, "per_leg": per_leg}
    for leg in legs:
        if leg != "reference":
            res["clock_ratio_%s_over_reference" % leg] = med[leg] / med["reference"]
            res["blind_rotation_ratio_%s_over_reference" % leg] = per_leg[leg]["blind_rotations"] / per_leg["reference"]["blind_rotations"]
            res["device_ms_ratio_%s_over_reference" % leg] = ((per_leg[leg]["blind_rotate_ms"] + per_leg[leg]["tail_ms"])
                                                              / (per_leg["reference"]["blind_rotate_ms"] + per_leg["reference"]["tail_ms"]))
    for c in circ.values():
        c.close()
    return res


def run_legs(args, root, legs):
    bce, kat = load(root)
    ccs = {}
    for leg in legs:
        ccs[leg] = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
        ccs[leg].KeyGen(0x0FE5EED)
    results = []
    if args.adder_k:
        results.append(measure(bce, ccs, legs, "adder_64bit", os.path.join(kat.CIRCUITS, "adder_64bit.txt"), args.adder_k,
                               [kat.adder_case(t, 64) for t in range(8)], args.reps))
    if args.aes_k:
        vecs = [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]
        results.append(measure(bce, ccs, legs, "AES-expanded", os.path.join(kat.CIRCUITS, "AES-expanded.txt"), args.aes_k, vecs, args.reps))
    return results


def run_parent_ab(args):
    """children alternate parent, this, parent, this, ...; nothing of the GPU is touched by this process"""
    runs = {"parent": [], "this": []}
    for rnd in range(args.ab_rounds):
        for who, root in (("parent", args.parent_root), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root), "--reps", str(args.reps),
                   "--aes-k", str(args.aes_k), "--adder-k", str(args.adder_k)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                raise RuntimeError("child (%s) failed with status %d: %s" % (who, out.returncode, out.stderr[-2000:]))
            runs[who].append(json.loads(lines[-1][7:]))
            for r in runs[who][-1]:
                print("A/B round %d %-6s %-12s K=%d reference %.4f s" % (rnd, who, r["circuit"], r["instances"], r["median_wall_s"]["reference"]), flush=True)
    res = []
    for i in range(len(runs["this"][0])):
        p = [run[i]["median_wall_s"]["reference"] for run in runs["parent"]]
        t = [run[i]["median_wall_s"]["reference"] for run in runs["this"]]
        mp, mt = statistics.median(p), statistics.median(t)
        margin = max(p) - min(p)
        res.append({"circuit": runs["this"][0][i]["circuit"], "instances": runs["this"][0][i]["instances"], "leg": "reference",
                    "reps_per_process": args.reps, "processes_per_build": args.ab_rounds,
                    "parent_median_wall_s_per_process": p, "this_median_wall_s_per_process": t,
                    "parent_wall_s": [run[i]["wall_s"]["reference"] for run in runs["parent"]],
                    "this_wall_s": [run[i]["wall_s"]["reference"] for run in runs["this"]],
                    "parent_median_s": mp, "this_median_s": mt, "this_over_parent": mt / mp,
                    "margin_s": margin, "margin_is": "spread between the parent's own repeated legs (max - min of its per-process medians)",
                    "slower_than_parent_beyond_margin": bool(mt - mp > margin)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--aes-k", type=int, default=32)
    ap.add_argument("--adder-k", type=int, default=64)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its library built: runs the parent comparison")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--only", choices=("legs", "parent"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xor_single_cost.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:       # one build, the reference leg alone (the parent has no other to compare)
        print("RESULT " + json.dumps(run_legs(args, args.root, ("reference",))), flush=True)
        return
    doc = json.load(open(args.out)) if args.only and os.path.exists(args.out) else {}
    doc["what"] = ("wall time of Circuit.Clock() with the reference XOR lowering, with setXorShared and with setXorSingle, the three "
                   "alternating round by round in one process on one device (tools/xor_single_cost.py); medians over `reps` timed "
                   "rounds after one warm-up round; per-kernel device times of the last round.  parent_comparison: the reference leg "
                   "of this build against a build of the parent commit, alternating processes on the same device")
    if args.only != "parent":
        doc["results"] = run_legs(args, ROOT, LEGS)
    if args.only != "legs" and args.parent_root:
        doc["parent_comparison"] = run_parent_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc.get("results", []):
        m, p = r["median_wall_s"], r["per_leg"]
        print("%s K=%d: reference %.3f s / %d steps / %d rotations, shared %.3f s / %d / %d, single %.3f s / %d / %d: Clock() x%.4f (shared), x%.4f (single)" % (
            r["circuit"], r["instances"], m["reference"], p["reference"]["steps"], p["reference"]["blind_rotations"], m["shared"], p["shared"]["steps"],
            p["shared"]["blind_rotations"], m["single"], p["single"]["steps"], p["single"]["blind_rotations"],
            r["clock_ratio_shared_over_reference"], r["clock_ratio_single_over_reference"]))
    for r in doc.get("parent_comparison", []):
        print("%s K=%d reference lowering: parent %.4f s, this %.4f s (x%.4f), margin %.4f s" % (
            r["circuit"], r["instances"], r["parent_median_s"], r["this_median_s"], r["this_over_parent"], r["margin_s"]))


if __name__ == "__main__":
    main()
