"""The HIP path against the reference's own Circuit program.

tests/golden/reference/*.json (tests/golden/make_reference_fixtures.py) hold what oracle/_ref/ref_run_oracle -- the
reference's unmodified circuit runtime, on the CPU oracle through oracle/refshim/binfhecontext.h -- left in every
register: full rows for the small circuits, one SHA-256 per register for the others.  Keys and input encryptions come
from one seed on both sides (KeyGen(seed), set_encrypt_seed(seed); the stand-in's Encrypt follows the engine's stream
and index rule and its BOOTSTRAPPED default), so the engine's registers must be those ciphertexts, bit for bit.
Nothing here reads the reference or oracle/_ref: the GPU machine has neither.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from kat import CIRCUITS

pytestmark = pytest.mark.gpu

REFERENCE = os.path.join(GOLDEN, "reference")
TOY_CIRCUITS = ["adder_2bit", "parity", "adder_32bit", "comparator_32bit_unsigned_lt"]


def load(circuit, paramset, method):
    return json.load(open(os.path.join(REFERENCE, "%s_%s_%s.json" % (circuit, paramset, method))))


@pytest.fixture(scope="module")
def contexts(bce):
    """(paramset, method) -> keyed context with the fixtures' seed for keys and for encryption"""
    made = {}

    def get(paramset, method, seed):
        key = (paramset, method)
        if key not in made:
            cc = bce.BinFHEContext(getattr(bce, paramset), getattr(bce, method))
            cc.KeyGen(seed)
            cc.set_encrypt_seed(seed)
            made[key] = cc
        return made[key]
    yield get
    for cc in made.values():
        cc.close()


@pytest.fixture(scope="module")
def texts(bce, tmp_path_factory):
    """circuit -> assembler text (ours: tests/test_reference_programs.py holds it equal to the reference's, byte for byte)"""
    tmp = tmp_path_factory.mktemp("asm")
    made = {}

    def get(circuit):
        if circuit in ("adder_2bit", "parity"):
            return os.path.join(CIRCUITS, circuit + ".out")
        if circuit not in made:
            made[circuit] = os.path.join(str(tmp), circuit + "_FHE.out")
            bce.assemble_bristol(os.path.join(CIRCUITS, circuit + ".txt"), made[circuit])
        return made[circuit]
    return get


def row_digest(row):
    return hashlib.sha256(np.ascontiguousarray(row, dtype="<u8").tobytes()).hexdigest()


def check_registers(cc, fix, vec, regs, base=0, what=""):
    """registers `regs` of the pool (slot = base + register: the netlists number their registers in file order, which is
    the Circuit's wire order) against the reference program's rows or digests; a mismatch names the register"""
    got = cc.lwe_read(np.array([base + r for r in regs], dtype=np.uint32))
    bad = []
    for r, row in zip(regs, got):
        if "rows" in vec:
            same = np.array_equal(row, np.array(vec["rows"][str(r)], dtype=np.uint64))
        else:
            same = row_digest(row) == vec["sha256"][str(r)]
        if not same:
            bad.append("R%d%s" % (r, " (input)" if r in fix["registers"]["inputs"] else ""))
    assert not bad, "%s%d of %d registers differ from the reference program's: %s" % (what, len(bad), len(regs), ", ".join(bad[:12]))


def circuit_for(bce, cc, fix, path):
    c = bce.Circuit(cc)
    c.ReadFile(path)
    info = c.info()
    assert info["n_wires"] == len(fix["registers"]["inputs"]) + len(fix["registers"]["gates"])
    assert info["n_levels"] == len(fix["rounds"]) and info["n_gates"] == sum(fix["rounds"])
    return c


@pytest.mark.parametrize("method", ["GINX", "AP"])
@pytest.mark.parametrize("circuit", TOY_CIRCUITS)
def test_every_register_equals_the_reference_programs(bce, contexts, texts, circuit, method):
    """reference-shaped Clock(): gate-level rounds (no relevel), the three-bootstrap XOR, BOOTSTRAPPED inputs"""
    fix = load(circuit, "TOY", method)
    cc = contexts("TOY", method, fix["seed"])
    c = circuit_for(bce, cc, fix, texts(circuit))
    regs = fix["registers"]["inputs"] + fix["registers"]["bootstrapped"]
    for k, vec in enumerate(fix["vectors"]):
        c.Reset()                                  # ReadFile made the first Reset: this is epoch k + 2, the stream index base
        assert vec["enc_base"] == (k + 2) << 44
        c.setEncrypted(True)
        c.setRelevel(False)
        c.SetInput(vec["inputs"])
        check_registers(cc, fix, vec, fix["registers"]["inputs"], what="after SetInput, vector %d: " % k)
        assert c.Clock()[0] == vec["outputs"]
        st = c.stats()
        assert st["bootstraps"] == fix["calls"]["EvalBinGate"] and st["levels"] == len(fix["rounds"]) and st["verify_fixes"] == 0
        check_registers(cc, fix, vec, regs, what="vector %d: " % k)
    c.close()


@pytest.mark.parametrize("schedule", ["relevel", "instances", "verify"])
@pytest.mark.parametrize("circuit", TOY_CIRCUITS)
def test_other_schedules_leave_the_same_registers(bce, contexts, texts, circuit, schedule):
    """The bootstrap-depth schedule, K = 3 instances and verify mode keep the reference lowering of every gate, so the
    bootstrapped registers are the same ciphertexts; with K = 3 that holds for instance 0, whose inputs come from the
    recorded stream indices -- instances 1 and 2 encrypt from their own and are compared on output bits."""
    fix = load(circuit, "TOY", "GINX")
    cc = contexts("TOY", "GINX", fix["seed"])
    c = circuit_for(bce, cc, fix, texts(circuit))
    vec = fix["vectors"][0]
    regs = fix["registers"]["inputs"] + fix["registers"]["bootstrapped"]
    K = 3 if schedule == "instances" else 1
    if K > 1:
        c.setInstances(K)
    c.Reset()
    c.setEncrypted(True)
    c.setRelevel(schedule != "verify")
    if schedule == "verify":
        c.setVerify(True)
    for i in range(K):
        c.SetInput(vec["inputs"], instance=i)
    out = c.Clock()
    assert out[0] == vec["outputs"]
    for i in range(1, K):
        assert c.Outputs(i)[0] == vec["outputs"], "instance %d" % i
    st = c.stats()
    assert st["verify_fixes"] == 0 and st["bootstraps"] == K * fix["calls"]["EvalBinGate"]
    check_registers(cc, fix, vec, regs, what=schedule + ": ")
    c.close()


@pytest.mark.parametrize("schedule", ["steps", "dataflow"])
def test_std128_registers_equal_the_reference_programs(bce, contexts, schedule):
    """STD128_OPT / GINX, adder_2bit: the kernel bench.py runs (step schedule) and the persistent kernel (setDataflow)
    against the reference program's 17 bootstraps on the oracle"""
    fix = load("adder_2bit", "STD128_OPT", "GINX")
    assert fix["calls"]["EvalBinGate"] + fix["calls"]["Encrypt"] == 17
    cc = contexts("STD128_OPT", "GINX", fix["seed"])
    c = circuit_for(bce, cc, fix, os.path.join(CIRCUITS, "adder_2bit.out"))
    vec = fix["vectors"][0]
    c.Reset()
    c.setEncrypted(True)
    if schedule == "dataflow":
        c.setDataflow(True)
    c.SetInput(vec["inputs"])
    assert c.dataflowActive() == (schedule == "dataflow")
    assert c.Clock()[0] == vec["outputs"]
    assert c.stats()["bootstraps"] == fix["calls"]["EvalBinGate"]
    check_registers(cc, fix, vec, fix["registers"]["inputs"] + fix["registers"]["bootstrapped"], what=schedule + ": ")
    c.close()


@pytest.mark.parametrize("lowering", ["setXorSingle", "setXorShared"])
def test_xor_lowerings_that_change_ciphertexts_keep_the_output_bits(bce, contexts, texts, lowering):
    """excluded from the register comparison by design: one- and two-bootstrap XORs leave other ciphertexts"""
    for circuit in TOY_CIRCUITS:
        fix = load(circuit, "TOY", "GINX")
        cc = contexts("TOY", "GINX", fix["seed"])
        c = circuit_for(bce, cc, fix, texts(circuit))
        for vec in fix["vectors"]:
            c.Reset()
            c.setEncrypted(True)
            getattr(c, lowering)(True)
            c.SetInput(vec["inputs"])
            assert c.Clock()[0] == vec["outputs"], circuit
        c.close()
