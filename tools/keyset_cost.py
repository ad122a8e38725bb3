#!/usr/bin/env python3
"""What key sets cost and buy: wall time of Circuit.Clock() on AES-expanded at STD128_OPT / GINX with

    a   K = 32 instances under ONE key set (no setInstanceKeys: what every caller had before key sets)
    b   K = 32 instances under 32 key sets (setInstanceKeys(range(32))): 32 clients in one launch per step
    c   K = 32 instances under 4 key sets of 8 instances each
    d   K = 1, measured once and multiplied by 32: what a server with 32 clients could do before key sets

on the bootstrap-depth schedule, step by step.  The pool belongs to the context, so each leg has a context and a Circuit of its
own (set k from KeyGen(seed + k), the same inputs) in ONE process on one device; a, b and c alternate round by round (a warm-up
round first, then --reps timed rounds, the median counts), d runs once after its own warm-up.  Every Clock() ends in a device
synchronise; the outputs of every instance are compared with the known answers after every run.  Reported: b / a, c / a,
d / b, and for a - c the kernel time per blind rotation (blind-rotation + tail device time of timing() over the rotations).

Existing callers must pay nothing: with --parent-root DIR (a checkout of the parent commit with its library built) leg a of
THIS build (AES-expanded K = 32 and adder_64bit K = 64, unkeyed) runs against the same leg of the parent's.  One library per
process, so the two builds alternate as child processes (parent, this, parent, this, ...: --ab-rounds of each); the margin is
the spread between the parent's own repeated legs (the method of parent_comparison in profiles/xor_single_cost.json).

    python3 tools/keyset_cost.py [--reps 3] [--parent-root DIR] [--ab-rounds 2] [--only legs|parent]
                                 [--out profiles/keyset_cost.json] [--aes-k 32] [--adder-k 64]

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


def load(root):
    """the package of the build under `root`; the known answers are this tree's"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import kat
    return importlib.import_module("openfhe-boolean-circuit-evaluator_amd"), kat


def context(bce, nsets):
    """a context with `nsets` key sets, set k from KeyGen(SEED + k); the parent's build has one set and no key-set calls"""
    cc = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    cc.KeyGen(SEED)
    for k in range(1, nsets):
        assert cc.keyset_add() == k
        cc.keyset_select(k)
        cc.KeyGen(SEED + k)
    if nsets > 1:
        cc.keyset_select(0)
    return cc


def circuit(bce, cc, path, K, cases, keys=None):
    c = bce.Circuit(cc)
    c.ReadBristol(path)
    c.setInstances(K)
    if keys is not None:
        c.setInstanceKeys(keys)
    c.Reset()
    c.setEncrypted(True)
    for k in range(K):
        c.SetInput(cases[k % len(cases)][0], instance=k)
    return c


def clock(c, cc, K, cases, what, rearm):
    if rearm:
        c.Rearm()
    cc.timing_reset()
    t0 = time.perf_counter()
    c.Clock()
    dt = time.perf_counter() - t0
    for k in range(K):
        assert c.Outputs(k)[0] == cases[k % len(cases)][1], "%s: instance %d is wrong" % (what, k)
    st, t = c.stats(), cc.timing()
    dev_ms = t["blind_rotate_ms"] + t["tail_ms"]
    return dt, {"steps": st["levels"], "launches": st["sublaunches"], "blind_rotations": st["bootstraps"], "blind_rotate_ms": t["blind_rotate_ms"],
                "tail_ms": t["tail_ms"], "fused_tail_launches": t["fused_tail_launches"],
                "kernel_us_per_blind_rotation": 1e3 * dev_ms / max(1, st["bootstraps"]),
                "by_kernel": [k for k in t["by_kernel"] if k["launches"]]}


def measure(name, legs, K, cases, reps):
    """legs: {leg: (circuit, context)}, alternating round by round; round 0 warms up (plan upload, first launches)"""
    wall = {leg: [] for leg in legs}
    per_leg = {}
    for rnd in range(reps + 1):
        for leg, (c, cc) in legs.items():
            dt, per_leg[leg] = clock(c, cc, K, cases, "%s, leg %s" % (name, leg), rnd > 0)
            if rnd:
                wall[leg].append(dt)
            print("%-12s round %d leg %-2s %8.3f s  (%d steps, %d blind rotations, %.3f us of kernel time each)" % (
                name, rnd, leg, dt, per_leg[leg]["steps"], per_leg[leg]["blind_rotations"], per_leg[leg]["kernel_us_per_blind_rotation"]), flush=True)
    return {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps, "wall_s": wall,
            "median_wall_s": {leg: statistics.median(wall[leg]) for leg in legs},
            "spread_s": {leg: max(wall[leg]) - min(wall[leg]) for leg in legs}, "per_leg": per_leg}


def run_unkeyed(args, root):
    """leg a alone, on any build: AES-expanded and adder_64bit under one key set"""
    bce, kat = load(root)
    results = []
    for name, file, K, cases in (("adder_64bit", "adder_64bit.txt", args.adder_k, [kat.adder_case(t, 64) for t in range(8)]),
                                 ("AES-expanded", "AES-expanded.txt", args.aes_k, [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"])):
        if not K:
            continue
        cc = context(bce, 1)
        c = circuit(bce, cc, os.path.join(kat.CIRCUITS, file), K, cases)
        results.append(measure(name, {"a": (c, cc)}, K, cases, args.reps))
        c.close()
        cc.close()
    return results


def run_legs(args):
    bce, kat = load(ROOT)
    K = args.aes_k
    path = os.path.join(kat.CIRCUITS, "AES-expanded.txt")
    cases = [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]
    groups = 4
    maps = {"a": None, "b": list(range(K)), "c": [k * groups // K for k in range(K)]}
    legs = {}
    for leg, keys in maps.items():
        cc = context(bce, 1 if keys is None else max(keys) + 1)
        legs[leg] = (circuit(bce, cc, path, K, cases, keys), cc)
    res = measure("AES-expanded", legs, K, cases, args.reps)
    res["key_sets"] = {"a": 1, "b": K, "c": groups}
    # d: one block alone, once after a warm-up run; 32 of them one after another is what 32 clients cost without key sets
    cc1 = context(bce, 1)
    c1 = circuit(bce, cc1, path, 1, cases)
    clock(c1, cc1, 1, cases, "AES-expanded, leg d (warm-up)", False)
    d_s, d_leg = clock(c1, cc1, 1, cases, "AES-expanded, leg d", True)
    print("AES-expanded leg d  %8.3f s for K = 1 (x %d = %.3f s)" % (d_s, K, d_s * K), flush=True)
    med = res["median_wall_s"]
    res["leg_d"] = {"instances": 1, "wall_s_once": d_s, "times": K, "wall_s_for_all": d_s * K, "per_leg": d_leg}
    res["ratio_b_over_a"] = med["b"] / med["a"]
    res["ratio_c_over_a"] = med["c"] / med["a"]
    res["ratio_d_over_b"] = d_s * K / med["b"]
    res["kernel_us_per_blind_rotation"] = {leg: res["per_leg"][leg]["kernel_us_per_blind_rotation"] for leg in legs}
    for c, cc in list(legs.values()) + [(c1, cc1)]:
        c.close()
        cc.close()
    return [res]


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
                print("A/B round %d %-6s %-12s K=%d unkeyed %.4f s" % (rnd, who, r["circuit"], r["instances"], r["median_wall_s"]["a"]), flush=True)
    res = []
    for i in range(len(runs["this"][0])):
        p = [run[i]["median_wall_s"]["a"] for run in runs["parent"]]
        t = [run[i]["median_wall_s"]["a"] for run in runs["this"]]
        mp, mt = statistics.median(p), statistics.median(t)
        margin = max(p) - min(p)
        res.append({"circuit": runs["this"][0][i]["circuit"], "instances": runs["this"][0][i]["instances"], "leg": "a (unkeyed, one key set)",
                    "reps_per_process": args.reps, "processes_per_build": args.ab_rounds,
                    "parent_median_wall_s_per_process": p, "this_median_wall_s_per_process": t,
                    "parent_wall_s": [run[i]["wall_s"]["a"] for run in runs["parent"]],
                    "this_wall_s": [run[i]["wall_s"]["a"] for run in runs["this"]],
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyset_cost.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:       # one build, the unkeyed leg alone (the parent has no other)
        print("RESULT " + json.dumps(run_unkeyed(args, args.root)), flush=True)
        return
    doc = json.load(open(args.out)) if args.only and os.path.exists(args.out) else {}
    doc["what"] = ("wall time of Circuit.Clock() on AES-expanded, STD128_OPT / GINX, with K instances under one key set (a), under K key sets "
                   "(b), under 4 key sets (c), the three alternating round by round in one process on one device, and K = 1 once, times K "
                   "(d) (tools/keyset_cost.py); medians over `reps` timed rounds after one warm-up round; kernel time per blind rotation "
                   "from the per-kernel device times of the last round.  parent_comparison: leg a of this build against a build of the "
                   "parent commit, alternating processes on the same device")
    if args.only != "parent":
        doc["results"] = run_legs(args)
    if args.only != "legs" and args.parent_root:
        doc["parent_comparison"] = run_parent_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc.get("results", []):
        m, u = r["median_wall_s"], r["kernel_us_per_blind_rotation"]
        print("%s K=%d: a %.3f s (%.3f us / rotation), b %.3f s (%.3f us), c %.3f s (%.3f us), d %.3f s x %d = %.3f s: b / a x%.4f, c / a x%.4f, d / b x%.4f" % (
            r["circuit"], r["instances"], m["a"], u["a"], m["b"], u["b"], m["c"], u["c"], r["leg_d"]["wall_s_once"], r["leg_d"]["times"],
            r["leg_d"]["wall_s_for_all"], r["ratio_b_over_a"], r["ratio_c_over_a"], r["ratio_d_over_b"]))
    for r in doc.get("parent_comparison", []):
        print("%s K=%d unkeyed: parent %.4f s, this %.4f s (x%.4f), margin %.4f s" % (
            r["circuit"], r["instances"], r["parent_median_s"], r["this_median_s"], r["this_over_parent"], r["margin_s"]))


if __name__ == "__main__":
    main()
