"""Writes tests/golden/ctx_params_pins.json: what a PARENT commit's derive_ctx() decides for a list of shapes and context
knobs, which tests/test_ctx_params.py holds derive_params() of this tree to.  Needs no GPU -- and must run without one.

    python tests/golden/make_ctx_params_pins.py <checkout of the parent commit, built> [output file]

Never run it against this tree: the fixture would then pin nothing.  It refuses a parent whose library exports
bce_params_derive.  It compiles tests/golden/ctx_params_probe.cpp (which includes the parent's engine.cpp) with the flags of
the parent's build.py, links it with the parent's _obj/*.o except engine.cpp.o, and runs the probe once per knob setting,
the cases on its standard input and the knobs in its environment.

The file: "names" (the order of a row's values), "cases" (id -> the probe's arguments, the knobs, cu_count) and "rows":
id -> [status, message, values], values in the order of "names" for status 0.  A case with knobs holds, instead of its values,
{name: value} of what differs from the same case without knobs.
"""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "openfhe-boolean-circuit-evaluator_amd"
FIXTURE = os.path.join(HERE, "ctx_params_pins.json")
PROBE = os.path.join(HERE, "ctx_params_probe.cpp")

SETS = ["TOY", "MEDIUM", "STD128_AP", "STD128_APOPT", "STD128", "STD128_OPT", "STD192", "STD192_OPT", "STD256", "STD256_OPT"]
AP, GINX = 1, 2
METHODS = {"AP": AP, "GINX": GINX}
KNOB_SETTINGS = [{"BCE_VARIANT": "1"}, {"BCE_VARIANT": "2"}, {"BCE_VARIANT": "3"}, {"BCE_OCCUPANCY": "2"}, {"BCE_XCD_GATE_US": "50"},
                 {"BCE_FUSE_TAIL": "0"}, {"BCE_FP64": "0"}, {"BCE_XCD_GATE": "0"}, {"BCE_FOLD": "0"}, {"BCE_FWD_UNITS": "0"},
                 {"BCE_FWD_MFMA": "0"}]
KNOB_NAMES = sorted({k for s in KNOB_SETTINGS for k in s})
KNOB_CASES = ["STD128_OPT/GINX", "STD128_OPT/AP", "STD192_OPT/GINX"]


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_near(bound, m, above):
    """the nearest prime = 1 mod m above (>=) or below (<) `bound`"""
    q = bound - bound % m + 1
    if above and q < bound:
        q += m
    if not above and q >= bound:
        q -= m
    while not is_prime(q):
        q += m if above else -m
    return q


def tabulated_Q(bits, cyclo):
    """PreviousPrime(FirstPrime(bits, cyclo), cyclo)"""
    return prime_near(prime_near((1 << bits) + 1, cyclo, True), cyclo, False)


def cases():
    """id -> {"set": [paramset, method]} or {"custom": [n, N, q, Q, qKS, baseKS, baseG, baseR, method]}, and "cu" """
    out = {}
    for p, name in enumerate(SETS):
        for m in METHODS:
            out["%s/%s" % (name, m)] = {"set": [p, METHODS[m]], "cu": 256}
    out["STD128_OPT/GINX@64"] = {"set": [SETS.index("STD128_OPT"), GINX], "cu": 64}
    out["STD192_OPT/AP@64"] = {"set": [SETS.index("STD192_OPT"), AP], "cu": 64}
    Q27 = tabulated_Q(27, 2048)

    def custom(name, n=502, N=1024, q=1024, Q=Q27, qKS=1 << 14, baseKS=1 << 7, baseG=1 << 7, baseR=32, method=GINX, cu=256):
        out[name] = {"custom": [n, N, q, Q, qKS, baseKS, baseG, baseR, method], "cu": cu}

    # the STD128_OPT ring at the LWE dimensions where an LDS layout stops fitting
    for n in (887, 888, 895, 896, 2423, 2424, 2431, 2432):
        custom("n=%d" % n, n=n)
    # the other ring dimensions, three and four gadget digits
    custom("N=512", n=64, N=512, q=512, Q=tabulated_Q(27, 1024), qKS=0, baseKS=25, baseG=1 << 9, baseR=23)
    custom("N=2048,27bit,3digits", N=2048, q=2048, Q=tabulated_Q(27, 4096), baseG=1 << 9, baseR=46)
    custom("N=2048,30bit,4digits", N=2048, q=2048, Q=prime_near(1 << 30, 4096, False), baseG=1 << 8, baseR=46)
    custom("N=2048,30bit,3digits", N=2048, q=2048, Q=prime_near(1 << 30, 4096, False), baseG=1 << 10, baseR=46)
    custom("N=1024,3digits", baseG=1 << 9)
    custom("N=1024,4digits", baseG=1 << 7)
    # the ring modulus either side of the width classes
    custom("Q<2^28", Q=prime_near(1 << 28, 2048, False))
    custom("Q>2^28", Q=prime_near(1 << 28, 2048, True), baseG=1 << 8)
    custom("Q<2^31", N=2048, q=2048, Q=prime_near(1 << 31, 4096, False), baseG=1 << 8, baseR=46)
    custom("Q>2^31", N=2048, q=2048, Q=prime_near(1 << 31, 4096, True), baseG=1 << 8, baseR=46)   # (no kernel: pinned as rejected)
    custom("Q<2^31,N=1024", Q=prime_near(1 << 31, 2048, False), baseG=1 << 8)
    custom("Q>2^31,N=1024", Q=prime_near(1 << 31, 2048, True), baseG=1 << 8)
    for m in METHODS:
        custom("Q<2^39/%s" % m, Q=prime_near(1 << 39, 2048, False), baseG=1 << 13, method=METHODS[m])
        custom("Q>2^39/%s" % m, Q=prime_near(1 << 39, 2048, True), baseG=1 << 14, method=METHODS[m])
    # the doubles family at N = 2048 has a folded build: three digits of 14 bits fold, three of 16 bits decompose exactly as
    # well but digit x twiddle is no longer exact in a double; N = 2048, 30 bits, base 2^10 (above) fails the exact decomposition
    custom("N=2048,Q<2^39,B=2^14", N=2048, q=2048, Q=prime_near(1 << 39, 4096, False), baseG=1 << 14, baseR=46)
    custom("N=2048,Q<2^39,B=2^16", N=2048, q=2048, Q=prime_near(1 << 39, 4096, False), baseG=1 << 16, baseR=46)
    custom("Q<2^40", Q=prime_near(1 << 40, 2048, False), baseG=1 << 14)
    custom("odd-factor", q=2048)
    # AP keys either side of 2^31 bytes (n * baseR * dR * 2 dG * 2 N * 4 bytes = n * 2^22)
    custom("AP,n=511", n=511, method=AP)
    custom("AP,n=512", n=512, method=AP)
    custom("AP,n=513", n=513, method=AP)
    for qKS in (65536, 65537, 1 << 29, (1 << 29) + 1):
        custom("qKS=%d" % qKS, qKS=qKS)
    # every rejected argument
    custom("reject:method", method=3)
    for N in (256, 1000, 4096):
        custom("reject:N=%d" % N, N=N, Q=prime_near(1 << 27, 2 * N, False) if N != 1000 else Q27)
    for q in (1000, 4096, 4):
        custom("reject:q=%d" % q, q=q)
    custom("reject:Q-composite", Q=next(Q27 + 2048 * k for k in range(1, 99) if not is_prime(Q27 + 2048 * k)))
    custom("reject:Q-not-1-mod-2N", Q=(1 << 27) - 39)
    custom("reject:Q>=2^40", Q=prime_near(1 << 40, 2048, True), baseG=1 << 14)
    for baseG in (0, 1, 96):
        custom("reject:baseG=%d" % baseG, baseG=baseG)
    custom("reject:n=0", n=0)
    for baseKS in (0, 1):
        custom("reject:baseKS=%d" % baseKS, baseKS=baseKS)
    for baseR in (0, 1):
        custom("reject:AP,baseR=%d" % baseR, baseR=baseR, method=AP)
    custom("GINX,baseR=0", baseR=0)
    custom("reject:qKS=2^32", qKS=1 << 32)
    custom("reject:qKS>2^32,digits", qKS=1 << 33, baseG=1 << 5)     # two reasons: the kernel class speaks first
    custom("reject:6digits", baseG=1 << 5)
    custom("reject:N=2048,27bit,4digits", N=2048, q=2048, Q=tabulated_Q(27, 4096), baseG=1 << 7, baseR=46)
    custom("reject:N=2048,37bit,4digits", N=2048, q=2048, Q=prime_near(1 << 37, 4096, False), baseG=1 << 10, baseR=46)
    # the STD192 ring at LWE dimensions either side of what the doubles kernel's LDS layout holds
    for n in (2040, 2048, 2100):
        custom("STD192,n=%d" % n, n=n, N=2048, Q=tabulated_Q(37, 4096), qKS=1 << 19, baseKS=28, baseG=1 << 13)
    assert is_prime((1 << 27) - 39) and ((1 << 27) - 40) % 2048
    return out


def probe_line(cid, case):
    if "set" in case:
        return "%s set %d %d %d" % (cid.replace(" ", "_"), case["set"][0], case["set"][1], case["cu"])
    return "%s custom %s %d" % (cid.replace(" ", "_"), " ".join(str(v) for v in case["custom"]), case["cu"])


def build_probe(parent, workdir):
    pkg = os.path.join(parent, PKG)
    spec = importlib.util.spec_from_file_location("parent_build", os.path.join(pkg, "build.py"))
    pb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pb)
    objs = [os.path.join(pb.OBJ, s + ".o") for s in pb.SOURCES if s != "engine.cpp"]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        sys.exit("the parent is not built (no %s)" % missing[0])
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj, exe = os.path.join(workdir, "probe.o"), os.path.join(workdir, "ctx_params_probe")
    subprocess.check_call([hipcc] + pb.FLAGS + ["-x", "hip", "-I" + pb.CSRC, "-c", PROBE, "-o", obj])
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-o", exe, obj] + objs + ["-lpthread", "-ldl"])
    return exe


def run_probe(exe, lines, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BCE_")}
    env.update(env_extra)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.exit("probe failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    rows = {}
    for ln in r.stdout.splitlines():
        cid, status, message, values = ln.split("\t")
        rows[cid] = (int(status), message, [kv.split("=") for kv in values.split()])
    return rows


def load(path=FIXTURE):
    """[(id, case, knobs, status, message, {name: value} or None)] with the knob rows' values filled in from their base"""
    with open(path) as f:
        fx = json.load(f)
    out = []
    for cid, (status, message, values) in fx["rows"].items():
        case = fx["cases"][cid]
        if status == 0 and isinstance(values, dict):
            base = dict(zip(fx["names"], fx["rows"][case["base"]][2]))
            base.update(values)
            values = base
        elif status == 0:
            values = dict(zip(fx["names"], values))
        else:
            values = None
        out.append((cid, case, case.get("env", {}), status, message, values))
    return out


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    so = os.path.join(parent, PKG, "libbce_amd.so")
    if os.path.exists(so) and hasattr(ctypes.CDLL(so), "bce_params_derive"):
        sys.exit("%s is this tree, not its parent: its library exports bce_params_derive" % parent)
    target = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    all_cases = cases()
    ids = {cid.replace(" ", "_"): cid for cid in all_cases}
    with tempfile.TemporaryDirectory() as work:
        exe = build_probe(parent, work)
        plain = run_probe(exe, [probe_line(c, all_cases[c]) for c in all_cases], {})
        names = [k for k, _ in plain[KNOB_CASES[0]][2]]
        assert "MIRROR_MISMATCH" not in " ".join(names)
        fixture = {"names": names, "cases": {}, "rows": {}}
        for pid, (status, message, kv) in plain.items():
            assert status != 0 or [k for k, _ in kv] == names, pid
            fixture["cases"][ids[pid]] = all_cases[ids[pid]]
            fixture["rows"][ids[pid]] = [status, message, [int(v) for _, v in kv]]
        for setting in KNOB_SETTINGS:
            got = run_probe(exe, [probe_line(c, all_cases[c]) for c in KNOB_CASES], setting)
            for cid in KNOB_CASES:
                status, message, kv = got[cid]
                base = dict(zip(names, fixture["rows"][cid][2]))
                assert status != 0 or [k for k, _ in kv] == names
                diff = {k: int(v) for k, v in kv if int(v) != base[k]}
                kid = "%s %s" % (cid, ",".join("%s=%s" % i for i in setting.items()))
                fixture["cases"][kid] = dict(all_cases[cid], env=setting, base=cid)
                fixture["rows"][kid] = [status, message, diff if status == 0 else []]
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(target, "w") as f:
        f.write('{\n"names": %s,\n"cases": {\n%s\n},\n"rows": {\n%s\n}\n}\n' % (
            one(fixture["names"]),
            ",\n".join("%s: %s" % (one(k), one(v)) for k, v in fixture["cases"].items()),
            ",\n".join("%s: %s" % (one(k), one(v)) for k, v in fixture["rows"].items())))
    print("%d rows (%d rejected) -> %s, %d bytes" % (len(fixture["rows"]), sum(r[0] != 0 for r in fixture["rows"].values()),
                                                      target, os.path.getsize(target)))
