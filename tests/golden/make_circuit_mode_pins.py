"""Writes tests/golden/circuit_mode_pins.json: what a PARENT commit's Circuit answers and runs for every combination of its
mode setters, which tests/test_circuit_modes.py and tests/test_gpu_circuit_modes.py hold this tree to.

    python tests/golden/make_circuit_mode_pins.py <checkout of the parent commit, built> host|gpu [output file]

Never run it against this tree's own library: the fixture would then pin nothing.  It refuses a library that exports
bce_circuit_resolve_mode (the parent has no such entry).  `host` writes the rows without an engine (no GPU needed) and
keeps the other groups of an existing fixture; `gpu` writes the rows with an engine and the Clock() records and keeps
the host rows.

Group "table": one row per point of
    plaintext x encrypted x verify x batched x relevel x XOR choice (none, fast, shared, single) x dataflow x
    dataflow-shared x graph x device-verify x gate sharding (off, world 2) x engine (ENGINES)
on parity.out, set on a fresh circuit before SetInput in the fixed order of apply().  A row is
    [inputs, engine, sharded, error, plaintext, encrypted, verify, xor_shared_active, dataflow_active, graph_active,
     device_verify_active, slot_stride, n_relevel_steps, n_tasks]
where `inputs` packs the REQUESTED choices as bits 0-10 of bce_circuit_resolve_mode's argument (bce_circuit.h), `error` is
"" or "<setter>:<code>" of the first setter that raised, plaintext / encrypted / verify are the flags the circuit then
reports (setVerify forces the other two on) and n_tasks is the length of dataflow_plan().  The file holds a row as three hex digits at its
position in that order (pack(), load()): 60 KB for 12,288 rows.

Group "clocks": for every distinct (path of Clock(), XOR mode, the four predicates) the table reaches on the context with
the persistent kernel, the first and the last row reaching it without gate sharding and with plaintext or encrypted on
(the first has the fewest options on, the last the most), run on adder_2bit.out with K = 2, fixed key seed, encryption seed and inputs, and -- where verify is on -- input register R0 of
instance 0 re-encrypted with the wrong bit: one Clock(), then Rearm() + Clock().  Per Clock(): outputs of both instances,
stats() without the three times, counts(), check_report(), the SHA-256 of lwe_read over every pool slot of both instances
and the "Bad ..." lines of stderr -- in the order written on the host path, sorted where the device checked (the device's
log holds the mismatches of one step in the order its workgroups found them, which differs from run to run).
"""
import hashlib
import importlib
import itertools
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CIRCUITS = os.path.join(HERE, "circuits")
PKG = "openfhe-boolean-circuit-evaluator_amd"
FIXTURE = os.path.join(HERE, "circuit_mode_pins.json")

# engine axis: no engine; STD128_OPT / GINX (split-transform kernels with the fused tail: dag_supported() == 1); TOY / GINX
# (three gadget digits: the one-wave-per-transform family, which has no persistent kernel: dag_supported() == 0)
ENGINES = ("none", "dag", "nodag")
ENGINE_PARAMS = {"dag": ("STD128_OPT", "GINX", 1), "nodag": ("TOY", "GINX", 0)}
XOR_SETTERS = (None, "setXorFast", "setXorShared", "setXorSingle")
AXES = 8 * 2 * 2 * 4 * 2 * 2 * 2 * 2 * 2      # rows per engine
SEED = 0x0FE5EED
K = 2
INPUTS = ([[1, 0], [1, 1]], [[1, 1], [0, 1]])  # a = 1, b = 3; a = 3, b = 2
COLUMNS = ["inputs", "engine", "sharded", "error", "plaintext", "encrypted", "verify", "xor_shared_active", "dataflow_active",
           "graph_active", "device_verify_active", "slot_stride", "n_relevel_steps", "n_tasks"]


def points():
    """(inputs bits, sharded) of every point of the table, in a fixed order"""
    for sharded, xor, rest in itertools.product((0, 1), range(4), range(1 << 9)):
        yield rest | xor << 9, sharded


def apply(bce, c, inputs, sharded):
    """the setters of one point on a freshly loaded circuit, in the fixed order; returns "" or "<setter>:<code>" """
    bit = lambda k: bool(inputs >> k & 1)
    xor = XOR_SETTERS[inputs >> 9 & 3]
    calls = [("Reset",)]
    if sharded:
        calls.append(("set_exchange", 0, 2, 1, lambda nbytes, on_dev: 0, None, None, None, None, 0))
    calls += [("setBatched", bit(3)), ("setRelevel", bit(4))]
    if xor:
        calls.append((xor, True))
    calls += [("setDataflowShared", bit(8)), ("setDataflow", bit(7)), ("setGraph", bit(5)), ("setDeviceVerify", bit(6)),
              ("setPlaintext", bit(0)), ("setEncrypted", bit(1)), ("setVerify", bit(2))]
    for name, *args in calls:
        try:
            getattr(c, name)(*args)
        except bce.BceError as e:
            return "%s:%d" % (name, e.code)
    return ""


def table_row(bce, c, inputs, engine, sharded):
    err = apply(bce, c, inputs, sharded)
    info = c.info()
    return [inputs, engine, sharded, err, int(c.getPlaintext()), int(c.getEncrypted()), int(c.getVerify()),
            int(c.xorSharedActive()), int(c.dataflowActive()), int(c.graphActive()), int(c.deviceVerifyActive()),
            info["slot_stride"], info["n_relevel_steps"], len(c.dataflow_plan()[0])]


def table(bce, engine, cc=None):
    """the rows of one engine kind (cc: its context, None without an engine)"""
    path = os.path.join(CIRCUITS, "parity.out")
    rows = []
    for inputs, sharded in points():
        c = bce.Circuit(cc)
        c.ReadFile(path)
        rows.append(table_row(bce, c, inputs, ENGINES.index(engine), sharded))
        c.close()
    return rows


def context(bce, engine, keys=False):
    paramset, method, dag = ENGINE_PARAMS[engine]
    cc = bce.BinFHEContext(getattr(bce, paramset), getattr(bce, method))
    assert int(bool(cc.dag_supported())) == dag, "%s / %s answers dag_supported() = %d" % (paramset, method, cc.dag_supported())
    if keys:
        cc.KeyGen(SEED)
    return cc


def mode_key(row):
    """(path of Clock(), XOR mode, the four predicates) of a table row with an engine.  The path is the branch Clock() takes:
    0 gate-level rounds, 1 step schedule, 2 dataflow kernel; the XOR mode as bce_circuit_resolve_mode numbers it."""
    r = dict(zip(COLUMNS, row))
    i = r["inputs"]
    batched, relevel, dataflow, xor = i >> 3 & 1, i >> 4 & 1, i >> 7 & 1, i >> 9 & 3
    scheduled = ((relevel or dataflow) and r["encrypted"] and not r["plaintext"] and batched) or r["device_verify_active"]
    path = 0 if not scheduled else 2 if r["dataflow_active"] else 1
    xor_mode = xor if xor in (1, 3) else 2 if r["xor_shared_active"] else 0
    return (path, xor_mode, r["xor_shared_active"], r["dataflow_active"], r["graph_active"], r["device_verify_active"])


def clock_points(rows):
    """the first and the last clockable row (no gate sharding, plaintext or encrypted on, no setter error) of every
    mode_key() the rows of the context with the persistent kernel reach: [(key, inputs)]; every key must have one"""
    first, last, keys = {}, {}, []
    for row in rows:
        r = dict(zip(COLUMNS, row))
        if r["engine"] != ENGINES.index("dag"):
            continue
        k = mode_key(row)
        if k not in keys:
            keys.append(k)
        if not r["sharded"] and not r["error"] and (r["plaintext"] or r["encrypted"]):
            first.setdefault(k, r["inputs"])
            last[k] = r["inputs"]
    assert all(k in first for k in keys), "a mode is reached only by rows that cannot be clocked"
    return [(k, i) for k in keys for i in sorted({first[k], last[k]})]


class _BadLines:
    """collects the lines beginning "Bad " that the library writes to file descriptor 2"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        self.lines = []
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.lines = [ln for ln in self.tmp.read().decode().splitlines() if ln.startswith("Bad ")]
        self.tmp.close()


def clock_record(bce, cc, inputs):
    """one Clock() and one Rearm() + Clock() of a point on adder_2bit.out, K = 2 (cc: the keyed STD128_OPT / GINX context)"""
    import numpy as np
    c = bce.Circuit(cc)
    c.ReadFile(os.path.join(CIRCUITS, "adder_2bit.out"))
    c.setInstances(K)
    err = apply(bce, c, inputs, 0)
    assert not err, err
    stride = c.info()["slot_stride"]
    slots = np.arange(K * stride, dtype=np.uint32)
    encrypted, verify = c.getEncrypted(), c.getVerify()
    cc.set_encrypt_seed(SEED)
    out = {"inputs": inputs, "clocks": []}
    try:
        if encrypted:
            cc.pool_reserve(K * stride)
            cc.lwe_write(slots, np.zeros((K * stride, cc.n + 1), dtype=np.uint64))
        for k in range(K):
            c.SetInput(INPUTS[k], instance=k)
        if encrypted and verify:
            cc.Encrypt([0], [0], enc_index_base=123456)     # R0 of instance 0 (a bit 0) now encrypts 0 instead of 1
        for rep in range(2):
            if rep:
                c.Rearm()
            with _BadLines() as bad:
                try:
                    c.Clock()
                    error = ""
                except bce.BceError as e:
                    error = "Clock:%d" % e.code
            stats, report = c.stats(), c.check_report()
            rec = {"error": error, "outputs": [c.Outputs(k) for k in range(K)],
                   "stats": {f: stats[f] for f in sorted(stats) if not f.endswith("_ms")},
                   "counts": c.counts(), "check_report": report, "bad": sorted(bad.lines) if report["checked"] else bad.lines,
                   "pool_sha256": hashlib.sha256(np.ascontiguousarray(cc.lwe_read(slots)).tobytes()).hexdigest() if encrypted else ""}
            out["clocks"].append(rec)
    finally:
        cc.set_encrypt_seed(None)
        c.close()
    return json.loads(json.dumps(out))     # as the fixture holds it: tuples are lists, keys are strings


BLOCK = 1 << 9                                 # rows per line of the file: one (gate sharding, XOR choice) block of points()
ANSWERS = COLUMNS[4:11]                        # one bit each, in this order


def pack(fixture):
    """the file's form of {"table_host", "table_gpu", "clocks"}.  A row's inputs, engine and sharding are its position (the
    order of points(), per engine); its code is two hex digits for the ANSWERS bits and one for its entry in "shapes", the
    distinct (error, slot_stride, n_relevel_steps, n_tasks).  "records" holds each distinct Clock() record once and "clocks"
    is [inputs, record of the first Clock(), record of the second]."""
    rows = fixture.get("table_host", []) + fixture.get("table_gpu", [])
    shapes = sorted({(r[3], r[11], r[12], r[13]) for r in rows})
    assert len(shapes) <= 16
    tables = {}
    for e, engine in enumerate(ENGINES):
        mine = [r for r in rows if r[1] == e]
        assert [(r[0], r[2]) for r in mine] == list(points())[:len(mine)], "rows out of the order of points()"
        codes = ["%02x%x" % (sum(r[4 + b] << b for b in range(7)), shapes.index((r[3], r[11], r[12], r[13]))) for r in mine]
        tables[engine] = ["".join(codes[at:at + BLOCK]) for at in range(0, len(codes), BLOCK)]
    records = []
    for c in fixture.get("clocks", []):
        records += [k for k in c["clocks"] if k not in records]
    return {"columns": COLUMNS, "shapes": shapes, "tables": tables, "records": records,
            "clocks": [[c["inputs"]] + [records.index(k) for k in c["clocks"]] for c in fixture.get("clocks", [])]}


def dumps(packed):
    """one line per block of rows, per record and per clocked point"""
    one = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)
    lines = lambda v: "[\n" + ",\n".join(one(x) for x in v) + "\n]"
    tables = "{\n" + ",\n".join('"%s": %s' % (e, lines(packed["tables"][e])) for e in ENGINES) + "\n}"
    return ('{\n"columns": %s,\n"shapes": %s,\n"tables": %s,\n"records": %s,\n"clocks": %s\n}\n'
            % (one(packed["columns"]), one(packed["shapes"]), tables, lines(packed["records"]), one(packed["clocks"])))


def load(path=FIXTURE):
    """the fixture as {"columns", "table_host", "table_gpu", "clocks"}: rows as lists in the order of COLUMNS, Clock()
    records as clock_record() returns them"""
    with open(path) as f:
        packed = json.load(f)
    rows = {}
    for e, engine in enumerate(ENGINES):
        codes = "".join(packed["tables"].get(engine, []))
        rows[engine] = []
        for (inputs, sharded), at in zip(points(), range(0, len(codes), 3)):
            bits, (error, stride, steps, tasks) = int(codes[at:at + 2], 16), packed["shapes"][int(codes[at + 2], 16)]
            rows[engine].append([inputs, e, sharded, error] + [bits >> b & 1 for b in range(7)] + [stride, steps, tasks])
    return {"columns": packed["columns"], "table_host": rows["none"], "table_gpu": rows["dag"] + rows["nodag"],
            "clocks": [{"inputs": i, "clocks": [packed["records"][a], packed["records"][b]]} for i, a, b in packed["clocks"]]}


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4) or sys.argv[2] not in ("host", "gpu"):
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    sys.path.insert(0, parent)
    bce = importlib.import_module(PKG)
    if not os.path.abspath(bce.__file__).startswith(parent + os.sep):
        sys.exit("the package was not imported from %s" % parent)
    if hasattr(bce.lib(), "bce_circuit_resolve_mode"):
        sys.exit("%s is this tree, not its parent: its library exports bce_circuit_resolve_mode" % parent)
    target = sys.argv[3] if len(sys.argv) > 3 else FIXTURE     # the groups it does not write are taken from FIXTURE
    fixture = load() if os.path.exists(FIXTURE) else {}
    fixture["columns"] = COLUMNS
    if sys.argv[2] == "host":
        fixture["table_host"] = table(bce, "none")
    else:
        rows = []
        for engine in ENGINES[1:]:
            cc = context(bce, engine)
            rows += table(bce, engine, cc)
            cc.close()
        fixture["table_gpu"] = rows
        cc = context(bce, "dag", keys=True)
        fixture["clocks"] = [clock_record(bce, cc, inputs) for _, inputs in clock_points(rows)]
        cc.close()
    with open(target, "w") as f:
        f.write(dumps(pack(fixture)))
    print("%s: %s -> %s" % (sys.argv[2], {k: len(v) for k, v in fixture.items()}, target))
