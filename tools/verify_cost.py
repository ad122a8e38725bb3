#!/usr/bin/env python3
"""What verify mode costs: wall time of Circuit.Clock() under

    off           verify off, bootstrap-depth schedule (the engine's default path)
    device        setVerify + setDeviceVerify: checks on the device between the schedule's steps, step by step
    device_graph  the same under setGraph (one hipGraph launch per Clock)
    host          setVerify alone: gate-level rounds, every level's outputs decrypted on the host (today's default)
    dataflow          verify off on the dataflow schedule: one persistent launch per Clock (setDataflow)
    device-dataflow   setDataflow + setDeviceVerify + setVerify: the checks inside the persistent kernel, between a
                      bootstrap and the release of its consumers

for AES-expanded at STD128_OPT GINX K = 32 and adder_64bit at K = 64.  One process, one context, one Circuit per netlist:
the input ciphertexts are encrypted once and every setting is a Rearm() + Clock() on them, so the settings alternate
round by round on the same device (a warm-up round first, then --reps timed rounds).  Every Clock() ends in a device
synchronise; outputs are compared with the known answers after every run.

    python3 tools/verify_cost.py [--reps 2] [--out profiles/verify_dataflow_cost.json] [--aes-k 32] [--adder-k 64]
                                 [--settings off,device,...]
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

SETTINGS = ("off", "device", "device_graph", "host", "dataflow", "device-dataflow")


def select(c, setting):
    verify = setting not in ("off", "dataflow")
    flow = setting.endswith("dataflow")
    c.setVerify(verify)               # on: also sets plaintext + encrypted
    c.setPlaintext(verify)
    c.setEncrypted(True)
    c.setDataflow(flow)               # chosen before SetInput (measure()): switching it afterwards keeps the pool layout
    c.setDeviceVerify(setting.startswith("device"))
    c.setGraph(setting == "device_graph")
    assert c.deviceVerifyActive() == setting.startswith("device") and c.graphActive() == (setting == "device_graph")
    assert c.dataflowActive() == flow


def measure(cc, name, path, K, cases, reps, settings):
    c = bce.Circuit(cc)
    c.ReadBristol(path)
    c.setInstances(K)
    c.setDataflow(True)               # the pool is laid out with the dataflow schedule's temporaries too
    c.Reset()
    c.setVerify(True)                 # SetInput keeps the plaintext bits and encrypts
    for k in range(K):
        c.SetInput(cases[k % len(cases)][0], instance=k)
    wall = {s: [] for s in settings}
    stats, reports = {}, {}
    for rnd in range(reps + 1):       # round 0 warms up (plan upload, graph capture, first launches)
        for s in settings:
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
            if s.startswith("device"):
                reports[s] = c.check_report()
            print("%-12s round %d %-13s %8.3f s  (%d dependent rounds)" % (name, rnd, s, dt, st["levels"]), flush=True)
    med = {s: statistics.median(wall[s]) for s in settings}
    n, q = cc.n, cc.params["q"]
    res = {"circuit": name, "paramset": "STD128_OPT", "method": "GINX", "instances": K, "reps": reps,
           "wall_s": wall, "median_wall_s": med, "spread_s": {s: max(wall[s]) - min(wall[s]) for s in settings},
           "per_setting": stats, "check_reports": reports, "q": q}

    def ratio(key, a, b):
        if a in med and b in med:
            res[key] = med[a] / med[b]

    ratio("device_over_off", "device", "off")
    ratio("device_graph_over_off", "device_graph", "off")
    ratio("host_over_off", "host", "off")
    ratio("host_over_device", "host", "device")
    ratio("device_dataflow_over_dataflow", "device-dataflow", "dataflow")
    ratio("dataflow_over_off", "dataflow", "off")
    if "device" in reports:
        res["check_report"] = reports["device"]
        res["checked_bytes_per_clock"] = reports["device"]["checked"] * (n + 1) * 4
        res["checked_bytes_per_step"] = reports["device"]["checked"] * (n + 1) * 4 / max(1, stats["device"]["levels"])
    if "device" in reports and "device-dataflow" in reports:   # integer sums over the same ciphertexts
        for f in ("checked", "mismatches", "repaired", "sum_err", "sum_sq_err", "max_abs_err"):
            assert reports["device"][f] == reports["device-dataflow"][f], "%s: the two schedules report different %s" % (name, f)
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--aes-k", type=int, default=32)
    ap.add_argument("--adder-k", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_dataflow_cost.json"))
    ap.add_argument("--settings", default=",".join(SETTINGS), help="comma-separated subset of " + ", ".join(SETTINGS))
    args = ap.parse_args()
    settings = tuple(args.settings.split(","))
    assert settings and all(s in SETTINGS for s in settings), settings
    cc = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
    cc.KeyGen(0x0FE5EED)
    results = []
    if args.adder_k:
        results.append(measure(cc, "adder_64bit", os.path.join(kat.CIRCUITS, "adder_64bit.txt"), args.adder_k,
                               [kat.adder_case(t, 64) for t in range(8)], args.reps, settings))
    if args.aes_k:
        vecs = [kat.aes_case(v) for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"]
        results.append(measure(cc, "AES-expanded", os.path.join(kat.CIRCUITS, "AES-expanded.txt"), args.aes_k,
                               vecs, args.reps, settings))
    doc = {"what": "wall time of Circuit.Clock() per verify setting, settings alternating round by round in one process "
                   "on one device (tools/verify_cost.py); medians over `reps` timed rounds after one warm-up round",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in results:
        m = r["median_wall_s"]
        print("%s K=%d: " % (r["circuit"], r["instances"]) + ", ".join("%s %.3f s" % (k, v) for k, v in m.items()))
        for k in ("device_over_off", "device_graph_over_off", "host_over_off", "device_dataflow_over_dataflow", "dataflow_over_off"):
            if k in r:
                print("    %-30s x%.4f" % (k, r[k]))
        for dev in ("device", "device_graph"):    # same schedule as `off`: the checks must not cost what the host path costs
            if dev in m and "host" in m:
                assert m[dev] < m["host"], "%s is not faster than host verify on %s" % (dev, r["circuit"])


if __name__ == "__main__":
    main()
