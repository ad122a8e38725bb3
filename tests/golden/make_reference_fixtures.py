"""Records what the reference's own programs (oracle/_ref, see oracle/Makefile) compute, as fixtures under
tests/golden/reference/ for the tests that run where there is no checkout of the reference (the GPU tests).

    python tests/golden/make_reference_fixtures.py            # everything but AES
    python tests/golden/make_reference_fixtures.py --aes      # also AES-expanded on the bits back end (minutes)
    python tests/golden/make_reference_fixtures.py --benches  # also the reference's TB_aes (4 minutes)

Per circuit x parameter set x method, from ref_run_oracle (the reference's Circuit on the CPU oracle, keys and input
encryptions from SEED as oracle/refshim/binfhecontext.h documents):
    seed, input bits, output bits, the stream index SetInput encrypts from, gates per Clock round, the numbers of
    Encrypt / EvalNOT / EvalBinGate calls, and the ciphertext of every register (inputs and gate outputs) -- full rows
    while the file stays under 64 KB, one SHA-256 per register (of the row as little-endian 64-bit words) otherwise.
assembler.json: SHA-256 of the reference assembler's text for every Bristol file of tests/golden/circuits, plain and
    annotated -- but neg64 (EQW) and mult2_64 (two output buses), where our assembler differs on purpose and
    tests/test_reference_programs.py compares the live texts through the stated transformation.
aes_expanded_bits.json (--aes): gates per round and output bits of AES-expanded, first vector of aes_vectors.json.
bench_TB_aes.json (--benches): TB_aes, slower than the slowest test of the suite, run at TOY on the bits back end for one
    loop of AES-expanded: its `passes` line, gates per Clock round, and the bits every encrypted run of the harness fed to
    SetInput and read from its OUTPUT gates (from the trace, matched to the text the bench assembled).
    tests/test_reference_programs.py holds kat.aes_case to them.  (TB_md5 on md5.txt -- 77,861 gates, the reference's
    ReadFile and manager are quadratic in them -- had not finished generating its netlist after 13 minutes 46 s of one
    core and would need hours for its eight Clocks: `--bench TB_md5` records it the same way for whoever has them; the
    harness's md5 vectors are pinned live instead, test_md5_harness_vectors_are_kats.)

tests/test_reference_programs.py regenerates the per-circuit fixtures from oracle/_ref and requires identical bytes.
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import kat  # noqa: E402
import oracle_walk as W  # noqa: E402
import ref_trace as RT  # noqa: E402

OUT = os.path.join(HERE, "reference")
SEED = 0x0FE5EED
ROW_LIMIT = 64 << 10

# circuit -> input vectors
VECTORS = {
    "adder_2bit": [[[1, 1], [0, 1]], [[0, 0], [0, 0]], [[1, 0], [1, 1]], [[0, 1], [1, 0]]],
    "parity": [kat.parity_case(0)[0], kat.parity_cascade_case(2)[0]],             # the second one has bit 8 set
    "adder_32bit": [kat.adder_case(0, 32)[0]],                                   # the harnesses' srand(0) vector
    "comparator_32bit_unsigned_lt": [kat.comparator_case(0, "comparator_32bit_unsigned_lt")[0]],
}
TOY_SETS = [(c, "TOY", m) for c in VECTORS for m in ("GINX", "AP")]
STD_SETS = [("adder_2bit", "STD128_OPT", "GINX")]
OLD_FORMAT = ["adder_32bit", "adder_64bit", "mult_32x32", "comparator_32bit_signed_lt", "comparator_32bit_signed_lteq",
              "comparator_32bit_unsigned_lt", "comparator_32bit_unsigned_lteq", "AES-expanded", "AES-non-expanded", "md5"]
NEW_FORMAT = ["adder64", "sub64", "mult64", "zero_equal", "aes_128_new", "sha256_new", "FP-add", "FP-eq", "FP-f2i", "FP-mul"]


def fixture_name(circuit, paramset, method):
    return "%s_%s_%s.json" % (circuit, paramset, method)


def row_digest(row):
    return hashlib.sha256(np.ascontiguousarray(row, dtype="<u8").tobytes()).hexdigest()


def circuit_text(circuit, tmp):
    """path of the assembler text: the two hand-written ones as committed, the Bristol ones through the REFERENCE's assembler"""
    if circuit in ("adder_2bit", "parity"):
        return os.path.join(kat.CIRCUITS, circuit + ".out")
    shutil.copy(os.path.join(kat.CIRCUITS, circuit + ".txt"), os.path.join(tmp, circuit + ".txt"))
    RT.run_program("ref_assemble", [circuit + ".txt", 0, 0], cwd=tmp)
    return os.path.join(tmp, circuit + "_FHE.out")


def record(circuit, paramset, method, vectors=None):
    """-> the fixture's text"""
    vectors = VECTORS[circuit] if vectors is None else vectors
    tmp = tempfile.mkdtemp()
    try:
        path = circuit_text(circuit, tmp)
        nl = W.read_assembler_text(path)
        tr = os.path.join(tmp, "trace")
        out = RT.run_program("ref_run_oracle", [path, paramset, method, "enc"] + [RT.vector_arg(v) for v in vectors],
                             trace=tr, seed=SEED, timeout=3000)
        runs = RT.read_trace(tr)
        clocks = RT.clock_rounds(out)
        assert len(runs) == len(clocks) == len(vectors)
        printed = [[int(ch) for ch in ln[4:]] for ln in out.split("\n") if ln.startswith("OUT ")]
        doc = {"circuit": circuit, "paramset": paramset, "method": method, "seed": SEED,
               "registers": {"inputs": [r for r, _, _ in nl.loads], "gates": [g[1] for g in nl.gates],
                             "bootstrapped": [g[1] for g in nl.gates if g[0] != "NOT"]},
               "rounds": clocks[0], "calls": {"Encrypt": len(runs[0].enc), "EvalNOT": len(runs[0].nots),
                                              "EvalBinGate": len(runs[0].gates)},
               "vectors": []}
        per_vector = []
        for k, (vec, run) in enumerate(zip(vectors, runs)):
            assert clocks[k] == clocks[0]
            ids = RT.match(nl, run)
            bits = RT.output_bits(nl, run, ids)
            assert bits == printed[k]
            rows = RT.register_rows(run, ids)
            per_vector.append(rows)
            doc["vectors"].append({"inputs": vec, "outputs": bits, "enc_base": (k + 2) << 44})
        for full in (True, False):
            for v, rows in zip(doc["vectors"], per_vector):
                v.pop("rows", None)
                v.pop("sha256", None)
                if full:
                    v["rows"] = {str(r): [int(w) for w in rows[r]] for r in sorted(rows)}
                else:
                    v["sha256"] = {str(r): row_digest(rows[r]) for r in sorted(rows)}
            text = json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n"
            if len(text) < ROW_LIMIT:
                break
        return text
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def assembler_digests():
    tmp = tempfile.mkdtemp()
    try:
        doc = {}
        for names, new_flag in ((OLD_FORMAT, 0), (NEW_FORMAT, 1)):
            for n in names:
                shutil.copy(os.path.join(kat.CIRCUITS, n + ".txt"), os.path.join(tmp, n + ".txt"))
                doc[n] = {"new_flag": new_flag}
                for key, dbg in (("plain", 0), ("annotated", 1)):
                    RT.run_program("ref_assemble", [n + ".txt", new_flag, dbg], cwd=tmp)
                    doc[n][key] = hashlib.sha256(open(os.path.join(tmp, n + "_FHE.out"), "rb").read()).hexdigest()
        return json.dumps(doc, sort_keys=True, indent=1) + "\n"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def aes_bits():
    tmp = tempfile.mkdtemp()
    try:
        path = circuit_text("AES-expanded", tmp)
        vec, want = kat.aes_case(kat.AES_VECTORS[0])
        nl = W.read_assembler_text(path)
        tr = os.path.join(tmp, "trace")
        out = RT.run_program("ref_run_bits", [path, "TOY", "GINX", "enc", RT.vector_arg(vec)], trace=tr, timeout=3000)
        (clock,) = RT.clock_rounds(out)
        (run,) = RT.read_trace(tr)
        printed = [[int(ch) for ch in ln[4:]] for ln in out.split("\n") if ln.startswith("OUT ")][0]
        assert printed == want, "the reference's AES-expanded output is not the vector's"
        doc = {"circuit": "AES-expanded", "vector": 0, "rounds": clock, "outputs": printed,
               "calls": {"Encrypt": len(run.enc), "EvalNOT": len(run.nots), "EvalBinGate": len(run.gates)}}
        return json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# program -> (arguments, the text it assembles and runs, under examples/)
SLOW_BENCHES = {
    "TB_aes": (["-z", "-a", "-s", "TOY", "-n", "1", "-c", "1"], "old_bristol_ckts/crypto/AES-expanded_FHE.out"),
    "TB_md5": (["-z", "-a", "-s", "TOY", "-n", "1"], "old_bristol_ckts/crypto/md5_FHE.out"),
}
BENCH_FILES = {"old_bristol_ckts/crypto": ["AES-expanded.txt", "AES-non-expanded.txt", "md5.txt", "md5-test.txt"]}


def bench_doc(name, out, trace, root):
    """what one run of a bench left (its stdout, its trace, its directory) -> the fixture's text"""
    args, rel = SLOW_BENCHES[name]
    passes = [ln.strip() for ln in out.split("\n") if ln.rstrip().endswith(" passes")]
    assert len(passes) == 1 and rel in passes[0] and " fails" not in out, out[-1500:]
    nl = W.read_assembler_text(os.path.join(root, "examples", rel))
    clocks = RT.clock_rounds(out)
    runs = RT.read_trace(trace)
    assert len(clocks) == 2 * len(runs) and all(c == clocks[0] for c in clocks)       # a plaintext and an encrypted Clock per vector
    doc = {"program": name, "args": args, "text": rel, "passes": passes[0], "rounds": clocks[0], "runs": []}
    for run in runs:
        ids = RT.match(nl, run)
        doc["runs"].append({"inputs": ["".join(str(b) for b in bus) for bus in RT.input_bits(nl, run)],
                            "outputs": "".join(str(b) for b in RT.output_bits(nl, run, ids))})
    return json.dumps(doc, sort_keys=True, indent=1) + "\n"


def record_bench(name):
    tmp = tempfile.mkdtemp()
    try:
        for d, files in BENCH_FILES.items():
            os.makedirs(os.path.join(tmp, "examples", d))
            for f in files:
                shutil.copy(os.path.join(kat.CIRCUITS, f), os.path.join(tmp, "examples", d, f))
        tr = os.path.join(tmp, "trace")
        out = RT.run_program(name, SLOW_BENCHES[name][0], cwd=tmp, trace=tr, timeout=3400)
        return bench_doc(name, out, tr, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv):
    assert RT.have_binaries(), "oracle/_ref is not built (make -C oracle, with a checkout of the reference)"
    os.makedirs(OUT, exist_ok=True)
    import time
    for c, p, m in TOY_SETS + STD_SETS:
        t0 = time.time()
        text = record(c, p, m, VECTORS[c][:1] if p != "TOY" else None)
        open(os.path.join(OUT, fixture_name(c, p, m)), "w").write(text)
        print("%s: %d bytes, %.1f s" % (fixture_name(c, p, m), len(text), time.time() - t0), flush=True)
    t0 = time.time()
    open(os.path.join(OUT, "assembler.json"), "w").write(assembler_digests())
    print("assembler.json: %.1f s" % (time.time() - t0), flush=True)
    if "--aes" in argv:
        t0 = time.time()
        open(os.path.join(OUT, "aes_expanded_bits.json"), "w").write(aes_bits())
        print("aes_expanded_bits.json: %.1f s" % (time.time() - t0), flush=True)
    if "--benches" in argv or "--bench" in argv:
        for name in (["TB_aes"] if "--benches" in argv else [argv[argv.index("--bench") + 1]]):
            t0 = time.time()
            open(os.path.join(OUT, "bench_%s.json" % name), "w").write(record_bench(name))
            print("bench_%s.json: %.1f s" % (name, time.time() - t0), flush=True)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
