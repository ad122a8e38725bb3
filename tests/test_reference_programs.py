"""The reference's OWN programs as the test oracle of the host runtime.

oracle/_ref holds the reference's circuit runtime, assembler and test benches, compiled from its unmodified sources
against the stand-in headers of oracle/refshim (oracle/Makefile, target `ref`).  Until now every restatement of the
reference in this suite (tests/oracle_walk.py, tests/kat.py, bench.cpu_baseline, csrc/bristol.cpp, csrc/circuit.cpp) was
checked against the others only; here each is checked against the live programs:

* assembler text, byte for byte, on every Bristol file of tests/golden/circuits;
* the harness vectors (srand / rand inputs, expected outputs) of kat.py against what the TB_* programs encrypt and decrypt;
* the ready-gate rounds of oracle_walk, bench.bristol_frontiers and our Circuit against `Processing: X of Y`;
* the operations of Gate::Evaluate against the netlist (tests/ref_trace.py), XOR expansion and operand order included;
* with the CPU oracle behind the stand-in, every ciphertext of the reference's run against oracle_walk's.

The tests need oracle/_ref; they skip only where neither it nor a checkout of the reference exists.
"""
import os
import re
import shutil
import time

import numpy as np
import pytest

import kat
import oracle_walk as W
import ref_trace as RT
from kat import CIRCUITS

SEED = 0x0FE5EED


@pytest.fixture(scope="module")
def ref():
    if RT.have_checkout():
        assert RT.have_binaries(), "the reference checkout is here but oracle/_ref was not built (make -C oracle)"
    elif not RT.have_binaries():
        pytest.skip("neither oracle/_ref nor a checkout of the reference (looked for at $BCE_REFERENCE, default %s)" % RT.REF_SRC)
    return RT


# ---------------------------------------------------------------------------------------------------------
# assembler
# ---------------------------------------------------------------------------------------------------------
OLD_FORMAT = ["adder_32bit", "adder_64bit", "mult_32x32", "comparator_32bit_signed_lt", "comparator_32bit_signed_lteq",
              "comparator_32bit_unsigned_lt", "comparator_32bit_unsigned_lteq", "AES-expanded", "AES-non-expanded"]
NEW_FORMAT = ["adder64", "sub64", "neg64", "mult64", "mult2_64", "zero_equal", "aes_128_new", "FP-add", "FP-eq", "FP-f2i", "FP-mul"]
# md5.txt (old) and sha256_new.txt (new) assemble to identical bytes as well; the reference needs 9 s and 30 s for them
# (its register search is quadratic), so they are compared by tests/golden/make_reference_fixtures.py, which records the
# digests of the reference's text, and test_assembler_digests_of_every_circuit checks ours against those.

# The deliberate differences of csrc/bristol.cpp from the reference's assembler, each asserted exactly below and only on
# circuits that contain the construct.  Any other difference is a bug.
DELIBERATE = {
    "EQW": "the reference cannot assemble EQW: it writes `#parse error on line L`, spends a register that nothing ever "
           "writes and STOREs it.  Ours makes the EQW's output an alias of its source register: no register, no line.",
    "EQ": "the reference exits on EQ (`Cannot parse EQ!! yet failing`).  Ours emits `R<k> = CONST(<0|1>)`.",
    "output buses": "the reference takes the first output width only and numbers the LAST that-many wires from out0.  Ours "
                    "numbers all output buses in header order and adds `# output buses <w1> <w2> ...`.",
    "input buses": "the reference reads two input widths.  Ours adds `# number input<k> bits <w>` for k > 2 after the "
                   "output line and LOADs from In<k>.",
}


def _ref_assemble(ref, tmp_path, src, new_flag, debug_flag, expect_fail=False):
    """run the reference's assembler in `tmp_path` (it writes <name>_FHE.out next to its input; relative names keep the
    '.' of a directory out of its file-name rule)"""
    name = os.path.basename(src)
    if os.path.abspath(src) != os.path.abspath(os.path.join(tmp_path, name)):
        shutil.copy(src, os.path.join(tmp_path, name))
    if expect_fail:
        import subprocess
        p = subprocess.run([os.path.join(RT.REF_BIN, "ref_assemble"), name, str(int(new_flag)), str(int(debug_flag))],
                           cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        return p
    ref.run_program("ref_assemble", [name, int(new_flag), int(debug_flag)], cwd=str(tmp_path))
    return open(os.path.join(tmp_path, name.split(".")[0] + "_FHE.out"), "rb").read()


def _ours(bce, tmp_path, src, new_flag, debug_flag):
    out = os.path.join(tmp_path, "ours_" + os.path.basename(src).split(".")[0] + ".out")
    bce.assemble_bristol(str(src), out, new_flag=new_flag, debug_flag=debug_flag)
    return open(out, "rb").read()


def _bristol_header(path):
    toks = [ln.split() for ln in open(path) if ln.strip()]
    return toks


def _constructs(path, new_flag):
    toks = _bristol_header(path)
    found = set()
    if new_flag:
        if int(toks[1][0]) > 2:
            found.add("input buses")
        if int(toks[2][0]) > 1:
            found.add("output buses")
    for t in toks[3 if new_flag else 2:]:
        if t[-1] in ("EQ", "EQW"):
            found.add(t[-1])
    return found


def _alias_eqw(ref_text, path):
    """What DELIBERATE["EQW"] says, applied to the reference's text: drop the parse-error line and the terminal-output
    comment that follows it, give every later register the number it has without the wasted ones, point the wasted
    register at its source."""
    toks = _bristol_header(path)
    n_in = sum(int(v) for v in toks[1][1:1 + int(toks[1][0])])
    gates = toks[3:]
    node_reg, remap, wasted = {w: w for w in range(n_in)}, {r: r for r in range(n_in)}, 0
    for j, t in enumerate(gates):
        nin = int(t[0])
        out_node, ref_reg = int(t[2 + nin]), n_in + j
        if t[-1] == "EQW":
            remap[ref_reg] = node_reg[int(t[2])]
            wasted += 1
        else:
            remap[ref_reg] = ref_reg - wasted
        node_reg[out_node] = remap[ref_reg]
    out, skip_terminal = [], False
    for line in ref_text.decode().split("\n"):
        if line.startswith("#parse error on line"):
            skip_terminal = True
            continue
        if skip_terminal and "is a terminal output register" in line:
            skip_terminal = False
            continue
        skip_terminal = False
        m = re.match(r"# (\d+) registers used", line)
        if m:
            line = "# %d registers used" % (int(m.group(1)) - wasted)
        else:
            line = re.sub(r"R(\d+)", lambda m: "R%d" % remap[int(m.group(1))], line)
        out.append(line)
    return "\n".join(out).encode()


def _last_output_bus_only(our_text, path):
    """What DELIBERATE["output buses"] says, undone on OUR text: keep the last bus only, numbered from out0."""
    toks = _bristol_header(path)
    widths = [int(v) for v in toks[2][1:1 + int(toks[2][0])]]
    first = sum(widths[:-1])
    out = []
    for line in our_text.decode().split("\n"):
        if line == "# output buses " + " ".join(str(w) for w in widths):
            continue
        if line == "# number output1 bits %d" % sum(widths):
            line = "# number output1 bits %d" % widths[0]
        m = re.match(r"(# R\d+ is a terminal output register for out)(\d+)$", line) or re.match(r"(Out)(\d+)( = STORE.*)$", line)
        if m:
            k = int(m.group(2))
            if k < first:
                continue
            line = m.group(1) + str(k - first) + (m.group(3) if m.lastindex == 3 else "")
        out.append(line)
    return "\n".join(out).encode()


@pytest.mark.parametrize("debug_flag", [False, True], ids=["plain", "annotated"])
@pytest.mark.parametrize("name,new_flag", [(n, False) for n in OLD_FORMAT] + [(n, True) for n in NEW_FORMAT])
def test_assembler_text_equals_the_reference_assemblers(bce, ref, tmp_path, name, new_flag, debug_flag):
    src = os.path.join(CIRCUITS, name + ".txt")
    theirs = _ref_assemble(ref, tmp_path, src, new_flag, debug_flag)
    ours = _ours(bce, tmp_path, src, new_flag, debug_flag)
    found = _constructs(src, new_flag)
    assert "EQ" not in found and "input buses" not in found       # (the synthetic circuits below cover those)
    if "EQW" in found:
        assert theirs != ours and b"#parse error on line" in theirs
        theirs = _alias_eqw(theirs, src)
    if "output buses" in found:
        assert theirs != ours
        ours = _last_output_bus_only(ours, src)
    if theirs != ours:
        a, b = theirs.decode().split("\n"), ours.decode().split("\n")
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail("%s: line %d differs (%d / %d lines)\n  reference: %r\n  ours:      %r" % (
            name, k + 1, len(a), len(b), a[k] if k < len(a) else None, b[k] if k < len(b) else None))


def test_assembler_kat_fixtures_are_what_the_reference_reads(ref, tmp_path):
    """adder_2bit.out and parity.out are hand-written assembler text the reference ships: its reader and ours
    (oracle_walk.read_assembler_text) must see the same gates -- the reference's run of them matches the netlist."""
    for name, vec in (("adder_2bit.out", [[1, 1], [0, 1]]), ("parity.out", [[1, 0, 1, 1, 0, 0, 1, 0, 0]])):
        nl = W.read_assembler_text(os.path.join(CIRCUITS, name))
        tr = str(tmp_path / (name + ".trace"))
        ref.run_program("ref_run_bits", [os.path.join(CIRCUITS, name), "TOY", "GINX", "enc", RT.vector_arg(vec)], trace=tr)
        (run,) = RT.read_trace(tr)
        RT.match(nl, run)


def test_assembler_refuses_what_ours_extends(bce, ref, tmp_path):
    """EQ and a third input bus: the constructs of DELIBERATE that no committed circuit holds."""
    eq = tmp_path / "eq.txt"            # 2 inputs, one EQ constant
    eq.write_text("3 6\n2 1 1\n1 1\n\n1 1 1 2 EQ\n2 1 0 2 3 XOR\n2 1 1 3 5 AND\n")
    p = _ref_assemble(ref, tmp_path, str(eq), True, False, expect_fail=True)
    assert p.returncode != 0 and "Cannot parse EQ" in p.stdout
    ours = _ours(bce, tmp_path, str(eq), True, False).decode().split("\n")
    assert [ln for ln in ours if "CONST" in ln] == ["R2 = CONST(1)"]
    assert [ln for ln in ours if re.match(r"R\d+ = (XOR|AND)", ln)] == ["R3 = XOR(R0, R2)  !depth = 1", "R4 = AND(R1, R3) !depth = 1"]

    three = tmp_path / "three.txt"      # three input buses, nothing else unusual
    three.write_text("2 6\n3 1 2 1\n1 1\n\n2 1 0 1 4 XOR\n2 1 4 3 5 AND\n")
    # the reference stops at two widths: bus 3's wire is never loaded, and the gate that reads it ends the program
    p = _ref_assemble(ref, tmp_path, str(three), True, False, expect_fail=True)
    assert p.returncode != 0 and "input register not found in reg_node_map" in p.stdout
    theirs = open(str(tmp_path / "three_FHE.out")).read().split("\n")
    assert [ln for ln in theirs if "LOAD" in ln] == ["R0 = LOAD(In1,0)", "R1 = LOAD(In2,0)", "R2 = LOAD(In2,1)"]
    ours = _ours(bce, tmp_path, str(three), True, False).decode().split("\n")
    assert ours[:5] == ["# Max depth 10000", "# number input1 bits 1", "# number input2 bits 2", "# number output1 bits 1",
                        "# number input3 bits 1"]
    assert [ln for ln in ours if "LOAD" in ln] == ["R0 = LOAD(In1,0)", "R1 = LOAD(In2,0)", "R2 = LOAD(In2,1)", "R3 = LOAD(In3,0)"]
    assert [ln for ln in ours if re.match(r"R\d+ = (XOR|AND)", ln)] == ["R4 = XOR(R0, R1)  !depth = 1", "R5 = AND(R4, R3) !depth = 1"]


# ---------------------------------------------------------------------------------------------------------
# test benches
# ---------------------------------------------------------------------------------------------------------
LAYOUT = {
    "simple_ckts/parity": ["parity.out"],
    "simple_ckts/adder_2bit": ["adder_2bit.out"],
    "old_bristol_ckts/arith": ["adder_32bit.txt", "adder_64bit.txt", "mult_32x32.txt", "comparator_32bit_signed_lt.txt",
                               "comparator_32bit_signed_lteq.txt", "comparator_32bit_unsigned_lt.txt",
                               "comparator_32bit_unsigned_lteq.txt"],
    "old_bristol_ckts/crypto": ["AES-expanded.txt", "AES-non-expanded.txt", "md5.txt", "md5-test.txt"],
}


def make_examples(root):
    """the reference's examples/ layout, filled from tests/golden/circuits"""
    for d, files in LAYOUT.items():
        os.makedirs(os.path.join(root, "examples", d))
        for f in files:
            shutil.copy(os.path.join(CIRCUITS, f), os.path.join(root, "examples", d, f))


COMPARATORS = ["comparator_32bit_signed_lteq", "comparator_32bit_unsigned_lteq", "comparator_32bit_signed_lt",
               "comparator_32bit_unsigned_lt"]                                   # TB_comparators' case order


def _parity_cases(t):
    return [kat.parity_case(t), kat.parity_cascade_case(t)]


# program -> (arguments, loops, [(assembled file under examples/, cases(test_ix) -> [(inputs, outputs), ...])])
BENCHES = {
    "TB_adder_2bit": (["-s", "TOY", "-n", "4"], 4,
                      [("simple_ckts/adder_2bit/adder_2bit.out", lambda t: [kat.adder_case(t, 2)])]),
    "TB_parity": (["-s", "TOY", "-n", "3"], 3, [("simple_ckts/parity/parity.out", _parity_cases)]),
    "TB_adders": (["-z", "-a", "-s", "TOY", "-n", "2", "-c", "2"], 2,
                  [("old_bristol_ckts/arith/adder_32bit_FHE.out", lambda t: [kat.adder_case(t, 32)]),
                   ("old_bristol_ckts/arith/adder_64bit_FHE.out", lambda t: [kat.adder_case(t, 64)])]),
    "TB_comparators": (["-z", "-a", "-s", "TOY", "-n", "3", "-c", "4"], 3,
                       [("old_bristol_ckts/arith/%s_FHE.out" % c, (lambda c: lambda t: [kat.comparator_case(t, c)])(c))
                        for c in COMPARATORS]),
    "TB_multipliers": (["-z", "-a", "-s", "TOY", "-n", "1", "-c", "1"], 1,
                       [("old_bristol_ckts/arith/mult_32x32_FHE.out", lambda t: [kat.multiplier_case(t)])]),
}
# TB_aes (255 s for `-n 1 -c 1`: two vectors, a plaintext and an encrypted Clock each) is slower than the slowest test of
# this suite, 124 s: `tests/golden/make_reference_fixtures.py --benches` runs it and records what it encrypts and decrypts,
# and test_slow_bench_vectors_are_kats compares kat.py with the record.  TB_md5 on the real md5.txt (77,861 gates; the
# reference's ReadFile and manager are quadratic in them) had not finished generating its netlist after 13 min 46 s and
# would need hours for its eight Clocks, so test_md5_harness_vectors_are_kats runs the bench live on a wiring-only text.
# TB_sha256 cannot run at all: it wants examples/old_bristol_ckts/crypto/sha-256.txt, and the reference ships no such
# circuit (only sha-256-test.txt).


@pytest.fixture(scope="module")
def benches(ref, tmp_path_factory):
    """every bench run once: name -> (stdout, runs of the trace, directory)"""
    done = {}

    def get(name):
        if name not in done:
            root = str(tmp_path_factory.mktemp(name))
            make_examples(root)
            tr = os.path.join(root, "trace")
            t0 = time.time()
            out = ref.run_program(name, BENCHES[name][0], cwd=root, trace=tr)
            print("%s: %.1f s" % (name, time.time() - t0))
            done[name] = (out, RT.read_trace(tr), root)
        return done[name]
    return get


@pytest.mark.parametrize("name", sorted(BENCHES))
def test_bench_passes_and_its_vectors_are_kats(ref, benches, name):
    """The bench prints its `passes` line, and what it encrypted (SetInput) and decrypted (the OUTPUT gates) in every
    loop is what tests/kat.py restates for that test_ix -- kat.py and golden/glibc_rand_bits.json pinned to the harness."""
    out, runs, root = benches(name)
    _, loops, files = BENCHES[name]
    passes = [ln for ln in out.split("\n") if ln.endswith(" passes")]
    assert len(passes) == len(files) and " fails" not in out, out[-1500:]
    k = 0
    for rel, cases in files:
        assert any(rel in ln for ln in passes), rel
        nl = W.read_assembler_text(os.path.join(root, "examples", rel))
        for t in range(loops):
            for want_in, want_out in cases(t):
                run = runs[k]
                k += 1
                ids = RT.match(nl, run)
                assert RT.input_bits(nl, run) == want_in, "%s test_ix %d: kat.py's inputs are not the harness's" % (rel, t)
                assert RT.output_bits(nl, run, ids) == want_out, "%s test_ix %d: kat.py's outputs are not the harness's" % (rel, t)
    assert k == len(runs)


# ---------------------------------------------------------------------------------------------------------
# round structure
# ---------------------------------------------------------------------------------------------------------
def _assembled(bce, tmp, name):
    out = os.path.join(str(tmp), name + "_FHE.out")
    bce.assemble_bristol(os.path.join(CIRCUITS, name + ".txt"), out)
    return out


ROUND_CIRCUITS = ["adder_2bit", "parity", "adder_32bit", "comparator_32bit_unsigned_lt", "mult_32x32"]


@pytest.fixture(scope="module")
def ref_runs(bce, ref, tmp_path_factory):
    """ref_run_bits, encrypted, one vector: circuit -> (netlist of the text, path, rounds, the run)"""
    done = {}

    def get(name):
        if name not in done:
            tmp = tmp_path_factory.mktemp("rounds_" + name)
            path = os.path.join(CIRCUITS, name + ".out") if name in ("adder_2bit", "parity") else _assembled(bce, tmp, name)
            nl = W.read_assembler_text(path)
            n_bus = 1 + max(v for _, v, _ in nl.loads)
            vec = [[(3 * b + 5 * v + 1) % 2 for (_, vv, b) in nl.loads if vv == v] for v in range(n_bus)]
            tr = os.path.join(str(tmp), "trace")
            t0 = time.time()
            out = ref.run_program("ref_run_bits", [path, "TOY", "GINX", "enc", RT.vector_arg(vec)], trace=tr)
            print("ref_run_bits %s: %.1f s" % (name, time.time() - t0))
            (clock,) = RT.clock_rounds(out)
            (run,) = RT.read_trace(tr)
            done[name] = (nl, path, clock, run, vec)
        return done[name]
    return get


@pytest.mark.parametrize("name", ROUND_CIRCUITS)
def test_clock_rounds_of_the_reference_manager(bce, ref, ref_runs, name):
    """`Processing: X of Y` after every round of the reference == oracle_walk.rounds == bench.bristol_frontiers (what
    cpu_baseline walks) == the levels of our Circuit; EvalBinGate calls == our bootstrap count, Encrypt calls == LOADs."""
    nl, path, clock, run, vec = ref_runs(name)
    assert clock == RT.expected_rounds(nl, W.rounds(nl)), "oracle_walk.rounds is not the reference manager's schedule"
    src = os.path.join(CIRCUITS, name + ".txt")
    if os.path.exists(src):
        import bench
        nb = W.read_bristol_old(src)
        assert clock == RT.expected_rounds(nb, W.rounds(nb))
        n_in, n_wires, fr = bench.bristol_frontiers(src)
        assert n_in == len(nb.loads) and n_wires == nb.n_regs
        assert [[(op if op != "INV" else "NOT", out) for op, _, _, out in r] for r in fr] == \
               [[(g[0], g[1]) for g in r] for r in W.rounds(nb)], "bench.bristol_frontiers walks other rounds than the reference"
        assert clock == RT.expected_rounds(nb, [[(g[0], g[3], g[1], g[2]) for g in r] for r in fr])
    # Our Circuit reports the number of levels and gates, not the gates of each level: no API exposes its per-level counts
    # in the reference-shaped mode, so those are held to the reference's only in total here (and, round by round, through
    # oracle_walk.rounds above, whose schedule the every-register GPU tests replay level by level).
    c = bce.Circuit(None)
    c.ReadFile(path)
    info = c.info()
    assert info["n_levels"] == len(clock) and info["n_gates"] == sum(clock)
    assert info["n_bootstraps"] == len(run.gates), "our bootstrap count is not the reference's EvalBinGate count"
    assert info["n_input_gates"] == len(run.enc)
    c.Reset(); c.setPlaintext(True); c.setRelevel(False)
    c.SetInput(vec)
    ids = RT.match(nl, run)
    assert c.Clock()[0] == RT.output_bits(nl, run, ids)
    assert c.stats()["levels"] == len(clock)


@pytest.mark.parametrize("name", ROUND_CIRCUITS)
def test_operations_of_gate_evaluate_match_the_netlist(ref, ref_runs, name):
    """Every gate of the netlist finds its EvalNOT / EvalBinGate records and every record is used (ref_trace.match);
    the matcher itself must refuse a run whose XOR expansion negates the other operands."""
    nl, _, _, run, _ = ref_runs(name)
    ids = RT.match(nl, run)
    assert set(ids) == {r for r, _, _ in nl.loads} | {g[1] for g in nl.gates}
    # Gate::Evaluate decrypts its inputs (src/gate.cpp:72-77): one Decrypt per gate input, none of them an output
    n_inputs = sum(1 if g[0] == "NOT" else 2 for g in nl.gates) + len(nl.stores)
    assert run.task_dec == n_inputs and len(run.out_dec) == len(nl.stores)
    xors = [g for g in nl.gates if g[0] == "XOR"]
    if xors:
        bad = RT.Run()
        bad.enc, bad.nots, bad.out_dec = run.enc, run.nots, run.out_dec
        not_outs = {o for o, _ in run.nots}
        half = {o for op, o, a, b in run.gates if op == "AND" and (a in not_outs or b in not_outs)}
        # the other operand order: OR(AND(!a, b), AND(a, !b))
        bad.gates = [(op, o, b, a) if op == "OR" and a in half and b in half else (op, o, a, b) for op, o, a, b in run.gates]
        if bad.gates != run.gates:
            with pytest.raises(RT.MatchError, match="XOR"):
                RT.match(nl, bad)


@pytest.mark.parametrize("name", ROUND_CIRCUITS)
def test_our_lowering_computes_what_gate_evaluate_computes(bce, ref, ref_runs, name):
    """OUR descriptors (sched::xor_lower and the negation flags of csrc/schedule.cpp, read back through relevel_plan) are,
    register by register, the same function of the same inputs as the calls the reference's Gate::Evaluate made: same
    gate, same operand order, the same operand negated.  Swapping the negations of the XOR's two ANDs fails here while
    every output bit stays right."""
    nl, path, _, run, _ = ref_runs(name)
    got = {}
    RT.match(nl, run, forms_out=got)
    c = bce.Circuit(None)
    c.ReadFile(path)
    ours = RT.plan_forms(got["F"], nl, c.relevel_plan())
    ops = {g[1]: g for g in nl.gates}
    F = got["F"]          # (our NOT chains are negation flags: compared up to NOT(NOT x) = x, which is the same ciphertext)
    bad = [RT.gate_text(ops[r]) for r in sorted(ops)
           if ops[r][0] != "NOT" and (r not in ours or F.normal(ours[r]) != F.normal(got["reg_form"][r]))]
    assert not bad, "%d gates are lowered to another expression than the reference evaluates: %s" % (len(bad), "; ".join(bad[:6]))


# ---------------------------------------------------------------------------------------------------------
# oracle back end
# ---------------------------------------------------------------------------------------------------------
def _vectors(name):
    if name == "adder_2bit":
        return [[[1, 1], [0, 1]], [[0, 1], [1, 1]]]
    if name == "parity":
        return [kat.parity_case(0)[0], kat.parity_cascade_case(2)[0]]      # (srand(0) and srand(1) give one stream; bit 8 set)
    return [kat.adder_case(0, 32)[0]]


@pytest.mark.parametrize("method", ["GINX", "AP"])
@pytest.mark.parametrize("name", ["adder_2bit", "parity", "adder_32bit"])
def test_reference_program_on_the_oracle_leaves_oracle_walks_ciphertexts(bce, orc, ref, tmp_path, name, method):
    """The reference's Circuit, running on the CPU oracle through the stand-in, decrypts the right bits, and every register
    it leaves -- inputs (BOOTSTRAPPED encryptions at the engine's stream indices) and gate outputs -- is bit for bit
    what oracle_walk.evaluate computes: the walk's reading of SetInput / Clock / Gate::Evaluate is the program's."""
    path = os.path.join(CIRCUITS, name + ".out") if name != "adder_32bit" else _assembled(bce, tmp_path, name)
    nl = W.read_assembler_text(path)
    vectors = _vectors(name)
    tr = str(tmp_path / "trace")
    out = ref.run_program("ref_run_oracle", [path, "TOY", method, "enc"] + [RT.vector_arg(v) for v in vectors], trace=tr, seed=SEED)
    runs = RT.read_trace(tr)
    assert len(runs) == len(vectors)
    o = orc.Oracle(orc.TOY, getattr(orc, method))
    o.keygen(SEED)
    outs = [[int(ch) for ch in ln[4:]] for ln in out.split("\n") if ln.startswith("OUT ")]
    for k, (vec, run) in enumerate(zip(vectors, runs)):
        ids = RT.match(nl, run)
        rows = RT.register_rows(run, ids)
        pool = []
        want, _ = W.evaluate(orc, o, nl, vec, enc_index=(k + 2) << 44, pool_out=pool)
        plain = _plain(nl, vec)
        assert outs[k] == plain == want == RT.output_bits(nl, run, ids)
        for reg in sorted(rows):
            assert np.array_equal(rows[reg], pool[0][reg]), "vector %d: register R%d of the reference program differs from oracle_walk" % (k, reg)


def _plain(nl, vec):
    v = {r: vec[value][bit] for r, value, bit in nl.loads}
    for op, dst, a, b in nl.gates:
        v[dst] = 1 - v[a] if op == "NOT" else (v[a] & v[b] if op == "AND" else v[a] | v[b] if op == "OR" else v[a] ^ v[b])
    return [v[nl.stores[k]] for k in range(1 + max(nl.stores))]


# ---------------------------------------------------------------------------------------------------------
# fixtures for the machines without the reference (tests/golden/reference, read by tests/test_gpu_reference_programs.py)
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_reference_fixtures", os.path.join(kat.GOLDEN, "make_reference_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fixture_sets():
    sets = [(c, "TOY", m) for c in ("adder_2bit", "parity", "adder_32bit", "comparator_32bit_unsigned_lt") for m in ("GINX", "AP")]
    return sets + [("adder_2bit", "STD128_OPT", "GINX")]


@pytest.mark.parametrize("circuit,paramset,method", _fixture_sets())
def test_committed_fixtures_are_what_the_reference_program_leaves_now(ref, gen, circuit, paramset, method):
    """regenerated from oracle/_ref, byte for byte: the fixtures cannot rot"""
    assert (circuit, paramset, method) in gen.TOY_SETS + gen.STD_SETS
    want = open(os.path.join(gen.OUT, gen.fixture_name(circuit, paramset, method))).read()
    got = gen.record(circuit, paramset, method, gen.VECTORS[circuit][:1] if paramset != "TOY" else None)
    assert got == want
    assert len(want) < gen.ROW_LIMIT


def test_assembler_digests_of_every_circuit(bce, tmp_path):
    """needs no reference: our assembler's text has the recorded SHA-256 of the reference assembler's, md5 and sha256_new
    (too slow in the reference's assembler to compare live) included"""
    import hashlib
    import json
    doc = json.load(open(os.path.join(kat.GOLDEN, "reference", "assembler.json")))
    assert {"md5", "sha256_new", "AES-expanded", "adder_32bit"} <= set(doc)
    for name, rec in sorted(doc.items()):
        for key, dbg in (("plain", False), ("annotated", True)):
            ours = _ours(bce, tmp_path, os.path.join(CIRCUITS, name + ".txt"), bool(rec["new_flag"]), dbg)
            assert hashlib.sha256(ours).hexdigest() == rec[key], "%s (%s) is not the reference assembler's text" % (name, key)


def test_aes_expanded_rounds_and_bits_of_the_reference_program():
    """recorded once from ref_run_bits (minutes of the reference manager's own bookkeeping): the rounds oracle_walk and
    bench.cpu_baseline walk for the benchmark circuit, the call counts and the output bits are the reference program's"""
    import json
    import bench
    doc = json.load(open(os.path.join(kat.GOLDEN, "reference", "aes_expanded_bits.json")))
    src = os.path.join(CIRCUITS, "AES-expanded.txt")
    nb = W.read_bristol_old(src)
    ready = W.rounds(nb)
    assert doc["rounds"] == RT.expected_rounds(nb, ready)
    _, _, fr = bench.bristol_frontiers(src)
    assert [len(r) for r in fr] == [len(r) for r in ready] and len(fr) == len(doc["rounds"]) - 1
    assert doc["outputs"] == kat.aes_case(kat.AES_VECTORS[0])[1]
    n_xor = sum(1 for g in nb.gates if g[0] == "XOR")
    n_and = sum(1 for g in nb.gates if g[0] == "AND")
    assert doc["calls"] == {"Encrypt": len(nb.loads), "EvalNOT": 2 * n_xor + sum(1 for g in nb.gates if g[0] == "NOT"),
                            "EvalBinGate": 3 * n_xor + n_and}
    assert doc["calls"]["EvalBinGate"] == 66415            # the bootstrap count DESIGN.md and binfhe_oracle.h quote


@pytest.mark.parametrize("name", ["TB_aes"])
def test_slow_bench_vectors_are_kats(name):
    """TB_aes, recorded by make_reference_fixtures.py --benches: the bench passed, and what it fed to SetInput and read
    from its OUTPUT gates for every vector is what kat.aes_case restates.  Needs no reference."""
    import json
    doc = json.load(open(os.path.join(kat.GOLDEN, "reference", "bench_%s.json" % name)))
    assert doc["passes"].endswith(" passes") and doc["text"] in doc["passes"]
    if name == "TB_aes":
        vs = sorted((v for v in kat.AES_VECTORS if v["circuit"] == "AES-expanded"), key=lambda v: v["case"])
        want = [kat.aes_case(v) for v in vs]                                   # the two cases of src/test_aes.cpp:184-228
        assert len(want) == 2
        src = "AES-expanded.txt"
    else:
        want = [kat.md5_case(i, o) for i, o in kat.hash_vectors("md5-test.txt")]
        assert len(want) == 4
        src = "md5.txt"
    got = [([[int(ch) for ch in bus] for bus in r["inputs"]], [int(ch) for ch in r["outputs"]]) for r in doc["runs"]]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "%s vector %d: kat.py's inputs are not the harness's" % (name, k)
        assert g[1] == w[1], "%s vector %d: kat.py's outputs are not the harness's" % (name, k)
    nb = W.read_bristol_old(os.path.join(CIRCUITS, src))
    assert doc["rounds"] == RT.expected_rounds(nb, W.rounds(nb))


def test_md5_harness_vectors_are_kats(ref, tmp_path):
    """src/test_md5.cpp live, without the hours its 77,861-gate circuit costs the reference's manager: TB_md5 is given a
    small text in place of md5_FHE.out (512 LOADs; Out k = R k OR (R 128+3k AND R 129+3k AND R 130+3k): every wire needs a
    consumer, the reference's manager spins on one without), so the bench itself reports `fails` -- but
    every vector still goes through its own HexStr2UintVec, its reversal and SetInput, and its plaintext mismatch report
    prints the expected word bit by bit.  The 512 bits it encrypts per vector and the 128 it expects must be
    kat.md5_case of the four vectors of md5-test.txt (kat.hash_vectors)."""
    d = tmp_path / "examples" / "old_bristol_ckts" / "crypto"
    d.mkdir(parents=True)
    text = ["# Max depth 10000", "# number input1 bits 512", "# number input2 bits 0", "# number output1 bits 128"]
    text += ["R%d = LOAD(In1,%d)" % (k, k) for k in range(512)]
    for k in range(128):
        a, r = 128 + 3 * k, 512 + 3 * k
        text += ["R%d = AND(R%d, R%d) !depth = 1" % (r, a, a + 1), "R%d = AND(R%d, R%d) !depth = 1" % (r + 1, r, a + 2),
                 "R%d = OR(R%d, R%d) !depth = 1" % (r + 2, k, r + 1)]
    text += ["Out%d = STORE(R%d) ! depth = 0" % (k, 514 + 3 * k) for k in range(128)]
    (d / "md5_FHE.out").write_text("\n".join(text) + "\n")
    tr = str(tmp_path / "trace")
    out = ref.run_program("TB_md5", ["-s", "TOY", "-n", "1"], cwd=str(tmp_path), trace=tr, timeout=120)
    nl = W.read_assembler_text(str(d / "md5_FHE.out"))
    runs = RT.read_trace(tr)
    want = [kat.md5_case(i, o) for i, o in kat.hash_vectors("md5-test.txt")]
    assert len(runs) == len(want) == 4
    blocks = out.split("comp output: ")[1:]
    assert len(blocks) == 4, "the stand-in text happened to compute a digest: no mismatch report to read"
    for k, (run, block, (w_in, w_out)) in enumerate(zip(runs, blocks, want)):
        assert RT.input_bits(nl, run) == w_in, "md5 vector %d: kat.md5_case's input is not what the harness encrypts" % k
        pairs = [ln.split() for ln in block.split("\n")[:128]]          # `computed expected`, bit 127 first
        assert all(len(p) == 2 for p in pairs)
        assert [int(p[1]) for p in pairs][::-1] == w_out, "md5 vector %d: kat.md5_case's output is not what the harness expects" % k
