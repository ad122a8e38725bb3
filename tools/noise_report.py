"""Noise model against measurement, per stage, on the GPU: the analytic model of tests/noise_model.py (DESIGN.md "Noise") next
to what debug_eval_stages (8192 bootstraps) and two dependent EvalGates levels (2 x 32768, device-side check) give.

usage: noise_report.py [PARAMSET [METHOD]]          one tabulated set (default STD128_OPT GINX), keys from a fixed seed
       noise_report.py --profile OUT.json           STD128_OPT GINX and every shape of tests/test_gpu_noise.py -> the committed
                                                    profiles/noise_model_ratios.json (ratio per stage, M, max |e| in sigma)
"""
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_model as nm  # noqa: E402
import noise_run  # noqa: E402

bce = importlib.import_module("openfhe-boolean-circuit-evaluator_amd")
NOTE = ("ratio = measured second moment / the model's for the key at hand (V - V_bias + mean^2, tests/noise_model.py); "
        "against_key_averaged_V = the same second moment / V, the average over keys")


def measure(c, name):
    s, z = c.export_sk()
    V = nm.model(c.params, s, z)
    row = {"case": name, "model": {k: round(V["V_" + k], 3) for k in ("N", "ks", "out")}, "stages": {}}
    err, wrong = noise_run.stage_run(c, np.random.default_rng(21))
    for tag in ("N", "ks", "out"):
        ratio, raw, mean, bar, mx, _ = nm.stage_stats(err[tag], V["V_" + tag], V["B_" + tag])
        row["stages"][tag] = {"M": int(err[tag].size), "ratio": round(ratio, 4), "against_key_averaged_V": round(raw, 4), "mean": round(mean, 3),
                              "mean_bar": round(bar, 3), "max_abs_err_sigma": round(mx, 2)}
    row["stages"]["out"]["wrong_bits"] = wrong
    for lvl, rep in enumerate(noise_run.end_run(c, bce.GateDesc, np.random.default_rng(22)), 1):
        ratio, mean, bar, mx = nm.report_stats(rep, V["V_out"], V["B_out"])
        row["stages"]["level%d" % lvl] = {"M": rep["checked"], "ratio": round(ratio, 4),
                                          "against_key_averaged_V": round(rep["sum_sq_err"] / rep["checked"] / V["V_out"], 4), "mean": round(mean, 3), "mean_bar": round(bar, 3),
                                          "max_abs_err_sigma": round(mx, 2), "mismatches": rep["mismatches"]}
    print("%-22s model V_N %.1f V_ks %.1f V_out %.2f (sigma %.2f)" % (name, V["V_N"], V["V_ks"], V["V_out"], math.sqrt(V["V_out"])))
    for tag, st in row["stages"].items():
        print("    %-7s M %6d  measured / model %.3f  mean %+.3f (bar %.3f)  max |e| %.2f sigma" % (
            tag, st["M"], st["ratio"], st["mean"], st["mean_bar"], st["max_abs_err_sigma"]), flush=True)
    return row


def main(argv):
    if argv and argv[0] == "--profile":
        from oracle import oracle as O        # the prime search of the custom shapes
        rows = []
        c = bce.BinFHEContext(bce.STD128_OPT, bce.GINX)
        c.KeyGen(0x0FE5EED)
        rows.append(measure(c, "STD128_OPT GINX"))
        c.close()
        for shape, (paramset, custom, methods) in noise_run.shapes(O.lib(), bce.TOY).items():
            for m in methods:
                c = bce.BinFHEContext(paramset, getattr(bce, m)) if custom is None else bce.BinFHEContext(method=getattr(bce, m), custom=custom)
                c.KeyGen(None)
                rows.append(measure(c, "%s %s" % (shape, m)))
                c.close()
        with open(argv[1], "w") as f:
            json.dump({"band": list(nm.BAND), "sigma": nm.SIGMA, "rows": rows, "note": NOTE}, f, indent=1)
            f.write("\n")
        return
    ps = argv[0] if argv else "STD128_OPT"
    method = argv[1] if len(argv) > 1 else "GINX"
    c = bce.BinFHEContext(getattr(bce, ps), getattr(bce, method))
    c.KeyGen(0x0FE5EED)
    measure(c, "%s %s" % (ps, method))
    c.close()


if __name__ == "__main__":
    main(sys.argv[1:])
