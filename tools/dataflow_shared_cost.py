#!/usr/bin/env python3
"""What setDataflowShared buys: wall time of Circuit.Clock() on the four combinations of schedule and XOR lowering

    steps + reference      the bootstrap-depth schedule, XOR = three blind rotations (the default)
    steps + shared         setXorShared: XOR = AND(OR, NAND), the OR and the NAND from one blind rotation
    dataflow + reference   setDataflow: the whole bootstrap DAG in one persistent launch
    dataflow + shared      setXorShared + setDataflow + setDataflowShared: pair tasks in the persistent kernel

for AES-expanded at K = 32 and adder_64bit at K = 256, STD128_OPT GINX.  The lowering and the schedule are chosen before
SetInput, so each leg has a Circuit and a context of its own (ONE key seed: the same keys; the same inputs) in ONE process on
one device, and the legs alternate round by round: a warm-up round first, then --reps timed rounds (at least 5); a leg's
figure is the median of its timed rounds.  Every Clock() ends in a device synchronise; outputs are compared with the known
answers after every run.  Per leg also: blind rotations, and for the dataflow legs busy / wait milliseconds per bootstrap of
dag_last_run().

Two numbers decide how the documents describe the option:
  (a) plain dataflow must not get slower from the branch the pair tasks add to the persistent kernel: the dataflow +
      reference leg of THIS build against the same leg of a build of the PARENT commit (--parent-root DIR: a checkout of the
      parent with its library built).  One library per process, so the two builds alternate as child processes (parent,
      this, parent, this, ...: --ab-rounds of each); the margin is the spread between the parent's own repeated legs.
  (b) dataflow + shared against steps + shared, the best the parent offers: the ratio at both shapes.

    python3 tools/dataflow_shared_cost.py [--reps 5] [--parent-root DIR] [--ab-rounds 2] [--only legs|parent]
                                          [--out profiles/dataflow_shared_cost.json]

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
SEED = 0x0FE5EED
LEGS = ("steps_reference", "steps_shared", "dataflow_reference", "dataflow_shared")
SHAPES = (("adder_64bit", "adder_64bit.txt", "adder_k"), ("AES-expanded", "AES-expanded.txt", "aes_k"))


def load(root):
    """the package of the tree at `root` (this tree's own by default), the test vectors of THIS tree"""
    sys.path.insert(0, os.path.abspath(root))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    return importlib.import_module("openfhe-boolean-circuit-evaluator_amd"), importlib.import_module("kat")


def cases_of(kat, name):
    if name == "adder_64bit":
        return [kat.adder_case(t, 64) for t in range(8)]
    return [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]


def make_circuit(bce, cc, leg, path, K, cases):
    dataflow, shared = leg.startswith("dataflow"), leg.endswith("shared")
    c = bce.Circuit(cc)
    c.ReadBristol(path)
    c.setInstances(K)
    c.setXorShared(shared)
    c.setDataflow(dataflow)
    if dataflow and shared:
        c.setDataflowShared(True)
    c.Reset()
    c.setEncrypted(True)
    assert c.xorSharedActive() == shared and c.dataflowActive() == dataflow, leg
    for k in range(K):
        c.SetInput(cases[k % len(cases)][0], instance=k)
    return c


def clock(c, cc, K, cases, what, rearm):
    if rearm:
        c.Rearm()
    t0 = time.perf_counter()
    c.Clock()
    dt = time.perf_counter() - t0
    for k in range(K):
        assert c.Outputs(k)[0] == cases[k % len(cases)][1], "%s: instance %d is wrong" % (what, k)
    st = c.stats()
    rec = {"blind_rotations": st["bootstraps"], "blind_rotations_per_instance": st["bootstraps"] // K, "launches": st["sublaunches"]}
    if c.dataflowActive():
        last = cc.dag_last_run()
        assert last["done"] == st["bootstraps"] and last["abort"] == 0, last
        rec.update(busy_ms_per_bootstrap=last.get("ms_per_bootstrap"), wait_ms_per_bootstrap=last.get("wait_ms_per_bootstrap"),
                   workgroups_per_cu=last["workgroups_per_cu"])
    return dt, rec


def measure(bce, kat, ccs, legs, name, path, K, reps):
    cases = cases_of(kat, name)
    circ = {leg: make_circuit(bce, ccs[leg], leg, path, K, cases) for leg in legs}
    wall = {leg: [] for leg in legs}
    per_leg = {}
    for rnd in range(reps + 1):       # round 0 warms up (plan / DAG upload, first launches)
        for leg in legs:
            dt, per_leg[leg] = clock(circ[leg], ccs[leg], K, cases, "%s, %s" % (name, leg), rnd > 0)
            if rnd:
                wall[leg].append(dt)
            print("%-12s K=%-3d round %d %-19s %8.3f s  (%d blind rotations)" % (name, K, rnd, leg, dt, per_leg[leg]["blind_rotations"]), flush=True)
    for c in circ.values():
        c.close()
    med = {leg: statistics.median(wall[leg]) for leg in legs}
    for leg in legs:
        per_leg[leg]["gate_bootstraps_per_s"] = per_leg[leg]["blind_rotations"] / med[leg]
    return {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps, "wall_s": wall,
            "median_wall_s": med, "spread_s": {leg: max(wall[leg]) - min(wall[leg]) for leg in legs}, "per_leg": per_leg}


def contexts(bce, legs):
    ccs = {}
    for leg in legs:
        ccs[leg] = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
        ccs[leg].KeyGen(SEED)
    return ccs


def run_legs(args, legs):
    bce, kat = load(args.root)
    ccs = contexts(bce, legs)
    results = []
    for name, fname, karg in SHAPES:
        K = getattr(args, karg)
        if K:
            results.append(measure(bce, kat, ccs, legs, name, os.path.join(kat.CIRCUITS, fname), K, args.reps))
    for cc in ccs.values():
        cc.close()
    return results


def child(args):
    """one build's dataflow + reference leg, as a process of its own: prints one JSON line"""
    print("RESULT " + json.dumps(run_legs(args, ("dataflow_reference",))), flush=True)


def run_parent_ab(args):
    """(a): children alternate parent, this, parent, this, ...; nothing of the GPU is touched by this process"""
    runs = {"parent": [], "this": []}
    for rnd in range(args.ab_rounds):
        for who, root in (("parent", args.parent_root), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(args.reps),
                   "--aes-k", str(args.aes_k), "--adder-k", str(args.adder_k)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.exit("child (%s) failed with status %d:\n%s\n%s" % (who, out.returncode, out.stdout[-2000:], out.stderr[-2000:]))
            runs[who].append(json.loads(lines[-1][7:]))
            for r in runs[who][-1]:
                print("A/B round %d %-6s %-12s K=%-3d dataflow + reference: median %.4f s" % (
                    rnd, who, r["circuit"], r["instances"], r["median_wall_s"]["dataflow_reference"]), flush=True)
    res = []
    for i in range(len(runs["this"][0])):
        p = [run[i]["median_wall_s"]["dataflow_reference"] for run in runs["parent"]]
        t = [run[i]["median_wall_s"]["dataflow_reference"] for run in runs["this"]]
        mp, mt = statistics.median(p), statistics.median(t)
        margin = max(p) - min(p)
        res.append({"circuit": runs["this"][0][i]["circuit"], "instances": runs["this"][0][i]["instances"], "leg": "dataflow_reference",
                    "reps_per_process": args.reps, "processes_per_build": args.ab_rounds,
                    "parent_median_wall_s_per_process": p, "this_median_wall_s_per_process": t,
                    "parent_wall_s": [run[i]["wall_s"]["dataflow_reference"] for run in runs["parent"]],
                    "this_wall_s": [run[i]["wall_s"]["dataflow_reference"] for run in runs["this"]],
                    "parent_median_s": mp, "this_median_s": mt, "this_over_parent": mt / mp,
                    "margin_s": margin, "margin_is": "spread between the parent's own repeated legs (max - min of its per-process medians)",
                    "slower_than_parent_beyond_margin": bool(mt - mp > margin)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--aes-k", type=int, default=32)
    ap.add_argument("--adder-k", type=int, default=256)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its library built: runs comparison (a)")
    ap.add_argument("--ab-rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--only", choices=("legs", "parent"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataflow_shared_cost.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("a leg reports the median of at least 5 Clock() calls")
    if args.child:
        return child(args)
    doc = {}
    if args.only and os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc["what"] = ("wall time of Circuit.Clock() on steps / dataflow x reference / shared XOR lowering, the four legs alternating round by "
                   "round in one process on one device (tools/dataflow_shared_cost.py); medians over `reps` timed rounds after one "
                   "warm-up round; busy / wait ms per bootstrap of dag_last_run() for the dataflow legs (last round).  "
                   "parent_comparison: the dataflow + reference leg of this build against a build of the parent commit, alternating "
                   "processes on the same device")
    if args.only != "parent":
        results = run_legs(args, LEGS)
        for r in results:
            m = r["median_wall_s"]
            r["dataflow_shared_over_steps_shared"] = m["dataflow_shared"] / m["steps_shared"]
            r["dataflow_shared_over_dataflow_reference"] = m["dataflow_shared"] / m["dataflow_reference"]
            r["dataflow_reference_over_steps_reference"] = m["dataflow_reference"] / m["steps_reference"]
        doc["results"] = results
    if args.only != "legs" and args.parent_root:
        doc["parent_comparison"] = run_parent_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc.get("results", []):
        m = r["median_wall_s"]
        print("%s K=%d: steps %.3f / %.3f s, dataflow %.3f / %.3f s (reference / shared); dataflow + shared over steps + shared x%.4f" % (
            r["circuit"], r["instances"], m["steps_reference"], m["steps_shared"], m["dataflow_reference"], m["dataflow_shared"],
            r["dataflow_shared_over_steps_shared"]))
    for r in doc.get("parent_comparison", []):
        print("%s K=%d dataflow + reference: parent %.4f s, this %.4f s (x%.4f), margin %.4f s" % (
            r["circuit"], r["instances"], r["parent_median_s"], r["this_median_s"], r["this_over_parent"], r["margin_s"]))


if __name__ == "__main__":
    main()
