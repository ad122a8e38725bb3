#!/usr/bin/env python3
"""What verify mode costs: wall time of Circuit.Clock() under

    off           verify off, bootstrap-depth schedule (the engine's default path)
    device        setVerify + setDeviceVerify: checks on the device between the schedule's steps, step by step
    device_graph  the same under setGraph (one hipGraph launch per Clock)
    host          setVerify alone: gate-level rounds, every level's outputs decrypted on the host (today's default)

for AES-expanded at STD128_OPT GINX K = 32 and adder_64bit at K = 64.  One process, one context, one Circuit per netlist:
the input ciphertexts are encrypted once and every setting is a Rearm() + Clock() on them, so the settings alternate
round by round on the same device (a warm-up round first, then --reps timed rounds).  Every Clock() ends in a device
synchronise; outputs are compared with the known answers after every run.

    python3 tools/verify_cost.py [--reps 2] [--out profiles/verify_device_cost.json] [--aes-k 32] [--adder-k 64]
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

SETTINGS = ("off", "device", "device_graph", "host")


def select(c, setting):
    verify = setting != "off"
    c.setVerify(verify)               # on: also sets plaintext + encrypted
    c.setPlaintext(verify)
    c.setEncrypted(True)
    c.setDeviceVerify(setting.startswith("device"))
    c.setGraph(setting == "device_graph")
    assert c.deviceVerifyActive() == setting.startswith("device") and c.graphActive() == (setting == "device_graph")


def measure(cc, name, path, K, cases, reps):
    c = bce.Circuit(cc)
    c.ReadBristol(path)
    c.setInstances(K)
    c.Reset()
    c.setVerify(True)                 # SetInput keeps the plaintext bits and encrypts
    for k in range(K):
        c.SetInput(cases[k % len(cases)][0], instance=k)
    wall = {s: [] for s in SETTINGS}
    stats, report = {}, None
    for rnd in range(reps + 1):       # round 0 warms up (plan upload, graph capture, first launches)
        for s in SETTINGS:
            c.Rearm()
            select(c, s)
            t0 = time.perf_counter()
            c.Clock()
            dt = time.perf_counter() - t0
            for k in range(K):
                assert c.Outputs(k)[0] == cases[k % len(cases)][1], "%s, %s: instance %d is wrong" % (name, s, k)
            st = c.stats()
            assert st["verify_fixes"] == 0, "%s, %s: %d fixes in a fault-free run" % (name, s, st["verify_fixes"])
            if rnd:
                wall[s].append(dt)
            stats[s] = {"levels": st["levels"], "sublaunches": st["sublaunches"], "bootstraps": st["bootstraps"]}
            if s == "device":
                report = c.check_report()
            print("%-12s round %d %-13s %8.3f s  (%d dependent rounds)" % (name, rnd, s, dt, st["levels"]), flush=True)
    med = {s: statistics.median(wall[s]) for s in SETTINGS}
    n, q = cc.n, cc.params["q"]
    res = {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps,
           "wall_s": wall, "median_wall_s": med, "per_setting": stats,
           "device_over_off": med["device"] / med["off"], "device_graph_over_off": med["device_graph"] / med["off"],
           "host_over_off": med["host"] / med["off"], "host_over_device": med["host"] / med["device"],
           "check_report": report,
           "checked_bytes_per_clock": report["checked"] * (n + 1) * 4,
           "checked_bytes_per_step": report["checked"] * (n + 1) * 4 / max(1, stats["device"]["levels"]),
           "q": q}
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--aes-k", type=int, default=32)
    ap.add_argument("--adder-k", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_device_cost.json"))
    args = ap.parse_args()
    cc = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    cc.KeyGen(0x0FE5EED)
    results = []
    if args.adder_k:
        results.append(measure(cc, "adder_64bit", os.path.join(kat.CIRCUITS, "adder_64bit.txt"), args.adder_k,
                               [kat.adder_case(t, 64) for t in range(8)], args.reps))
    if args.aes_k:
        vecs = [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]
        results.append(measure(cc, "AES-expanded", os.path.join(kat.CIRCUITS, "AES-expanded.txt"), args.aes_k,
                               vecs, args.reps))
    doc = {"what": "wall time of Circuit.Clock() per verify setting, settings alternating round by round in one process "
                   "on one device (tools/verify_cost.py); medians over `reps` timed rounds after one warm-up round",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        print("%s K=%d: off %.3f s, device %.3f s (x%.3f), device+graph %.3f s (x%.3f), host %.3f s (x%.3f); host / device = %.2f"
              % (r["circuit"], r["instances"], r["median_wall_s"]["off"], r["median_wall_s"]["device"], r["device_over_off"],
                 r["median_wall_s"]["device_graph"], r["device_graph_over_off"], r["median_wall_s"]["host"], r["host_over_off"],
                 r["host_over_device"]))
        assert r["median_wall_s"]["device"] < r["median_wall_s"]["host"], "device verify is not faster than host verify on " + r["circuit"]
        assert r["median_wall_s"]["device_graph"] < r["median_wall_s"]["host"], "device verify (graph) is not faster than host verify on " + r["circuit"]


if __name__ == "__main__":
    main()
