"""setXorShared on the host circuit runtime, without an engine: XOR as a PAIR(OR, NAND) descriptor and an AND, two blind
rotations instead of three in the same two steps.  For every netlist under tests/golden/circuits: the schedule holds
AND + OR + 2 XOR blind rotations in as many steps as the reference lowering and passes the runtime's own plan check."""
import os

import pytest

from kat import CIRCUITS

NEW_FORMAT = {"sha256_new.txt", "aes_128_new.txt", "adder64.txt", "sub64.txt", "neg64.txt", "mult64.txt", "mult2_64.txt",
              "zero_equal.txt", "FP-add.txt", "FP-eq.txt", "FP-f2i.txt", "FP-mul.txt"}
VECTORS = {"md5-test.txt", "sha-256-test.txt"}       # hash test vectors, not netlists
NETLISTS = sorted(f for f in os.listdir(CIRCUITS) if f not in VECTORS)


def _read(bce, name):
    c = bce.Circuit()
    if name.endswith(".out"):
        c.ReadFile(os.path.join(CIRCUITS, name))
    else:
        c.ReadBristol(os.path.join(CIRCUITS, name), new_flag=name in NEW_FORMAT)
    return c


def _gate_counts(c):
    """AND / OR / XOR gates of the netlist as the runtime counts them: one plaintext evaluation of all-zero inputs"""
    c.Reset()
    c.setPlaintext(True)
    c.setEncrypted(False)
    c.SetInput([[0] * w for w in c.buses()[0]])
    c.Clock()
    n = c.counts()
    c.Reset()
    return n


def test_the_list_covers_the_directory():
    assert len(NETLISTS) == 24 and "AES-expanded.txt" in NETLISTS and "adder_2bit.out" in NETLISTS


@pytest.mark.parametrize("name", NETLISTS)
def test_two_blind_rotations_per_xor_in_the_same_steps(bce, name):
    c = _read(bce, name)
    n = _gate_counts(c)
    ref_steps, ref_info, ref_hash = c.relevel_steps(), c.info(), c.plan_hash()
    assert sum(ref_steps) == ref_info["n_bootstraps"] == n["and"] + n["or"] + 3 * n["xor"]
    assert not c.xorSharedActive()
    c.setXorShared(True)
    assert c.xorSharedActive()
    steps, info = c.relevel_steps(), c.info()
    assert sum(steps) == info["n_bootstraps"] == n["and"] + n["or"] + 2 * n["xor"]
    assert len(steps) == len(ref_steps) == info["n_relevel_steps"] == ref_info["n_relevel_steps"]
    assert info["n_sublaunches"] == ref_info["n_sublaunches"]
    c.check_relevel()
    assert c.plan_hash() != ref_hash         # the mode is part of what the ranks of a run must agree on
    c.setBalance(False)                      # ASAP placement: an XOR's pair sits where its two ANDs sat
    c.check_relevel()
    shared_asap, shared_stride = c.relevel_steps(), c.info()["slot_stride"]
    c.setXorShared(False)
    assert not c.xorSharedActive() and sum(c.relevel_steps()) == ref_info["n_bootstraps"] and len(c.relevel_steps()) == len(shared_asap)
    assert c.info()["slot_stride"] == shared_stride      # the same two adjacent temporaries per XOR
    c.close()


def test_headline_counts(bce):
    want = {"AES-expanded.txt": (66415, 46090), "sha256_new.txt": (354505, 243861), "adder_64bit.txt": (610, 495)}
    for name, (ref, shared) in want.items():
        c = _read(bce, name)
        assert c.info()["n_bootstraps"] == ref
        c.setXorShared(True)
        assert c.info()["n_bootstraps"] == sum(c.relevel_steps()) == shared
        c.close()


def _set_inputs(c, K, plaintext=True):
    import kat
    c.Reset()
    c.setPlaintext(plaintext)
    c.setEncrypted(False)
    cases = [kat.adder_case(t, 64) for t in range(8)]
    for k in range(K):
        c.SetInput(cases[k % len(cases)][0], instance=k)
    return cases


def test_whether_it_is_active_is_fixed_at_setinput(bce):
    """adder_64bit, K = 64: slack filling lays the pool out for the shared lowering's schedule (stride 899), and neither
    placement of the reference lowering fits it (923 as soon as possible, 1035 by slack).  So setBatched / setRelevel /
    setVerify / setDeviceVerify are refused after SetInput where they would switch the lowering, leave their flag and the
    schedule alone, and pass where they would not; in both directions; and Reset() lifts it."""
    K = 64
    c = _read(bce, "adder_64bit.txt")
    c.setInstances(K)
    c.setXorShared(True)
    cases = _set_inputs(c, K)
    steps, info, plan_hash = c.relevel_steps(), c.info(), c.plan_hash()
    assert c.xorSharedActive() and sum(steps) == 495 and info["slot_stride"] < 923
    for call in (lambda: c.setBatched(False), lambda: c.setRelevel(False), lambda: c.setVerify(True)):
        with pytest.raises(bce.BceError) as e:
            call()
        assert e.value.code == bce.ERR_STATE and "before SetInput" in str(e.value)
        assert c.xorSharedActive() and c.relevel_steps() == steps and c.info() == info and c.plan_hash() == plan_hash
        assert (c.getPlaintext(), c.getEncrypted(), c.getVerify()) == (True, False, False)   # a refused setVerify sets none
    for call in (lambda: c.setBatched(True), lambda: c.setRelevel(True), lambda: c.setVerify(False), lambda: c.setDeviceVerify(True),
                 lambda: c.setGraph(True), lambda: c.setDataflow(True)):
        call()                                               # no change of the lowering: as ever
        assert c.xorSharedActive() and c.relevel_steps() == steps and c.plan_hash() == plan_hash
    c.setDeviceVerify(False)
    c.Clock()
    for k in range(K):
        assert c.Outputs(k)[0] == cases[k % len(cases)][1], k
    # the other direction: requested, inactive when the pool is laid out
    c.Reset()
    c.setBatched(False)                                      # before SetInput: the schedule follows
    assert not c.xorSharedActive() and sum(c.relevel_steps()) == 610
    _set_inputs(c, K)
    with pytest.raises(bce.BceError) as e:
        c.setBatched(True)
    assert e.value.code == bce.ERR_STATE and not c.xorSharedActive() and sum(c.relevel_steps()) == 610
    c.setRelevel(False)                                      # inactive either way
    c.setRelevel(True)
    c.Reset()
    c.setBatched(True)
    assert c.xorSharedActive() and c.relevel_steps() == steps
    c.close()
    # without the option these calls are unrestricted after SetInput, as before
    c = _read(bce, "adder_64bit.txt")
    c.setInstances(K)
    _set_inputs(c, K)
    for call in (lambda: c.setBatched(False), lambda: c.setRelevel(False), lambda: c.setVerify(True), lambda: c.setDeviceVerify(True),
                 lambda: c.setDeviceVerify(False), lambda: c.setVerify(False), lambda: c.setRelevel(True), lambda: c.setBatched(True)):
        call()
        assert not c.xorSharedActive() and sum(c.relevel_steps()) == 610
    c.close()


def test_option_rules(bce):
    c = _read(bce, "adder_2bit.out")
    c.setXorShared(True)
    with pytest.raises(bce.BceError) as e:
        c.setXorFast(True)
    assert e.value.code == bce.ERR_ARG
    c.setXorShared(False)
    c.setXorFast(True)
    with pytest.raises(bce.BceError) as e:
        c.setXorShared(True)
    assert e.value.code == bce.ERR_ARG
    c.setXorFast(False)
    c.setXorShared(True)
    assert sum(c.relevel_steps()) == 10
    # what it is active with: batched launches, the bootstrap-depth schedule, no host-side verify pass
    for off, on in ((lambda: c.setBatched(False), lambda: c.setBatched(True)), (lambda: c.setRelevel(False), lambda: c.setRelevel(True)),
                    (lambda: c.setVerify(True), lambda: c.setVerify(False))):
        off()
        assert not c.xorSharedActive() and sum(c.relevel_steps()) == 13 and c.info()["n_bootstraps"] == 13
        on()
        assert c.xorSharedActive() and sum(c.relevel_steps()) == 10
    c.setVerify(True)                        # Reset() clears the verify flag: the schedule follows
    assert not c.xorSharedActive() and sum(c.relevel_steps()) == 13
    c.Reset()
    assert c.xorSharedActive() and sum(c.relevel_steps()) == c.info()["n_bootstraps"] == 10
    assert [len(st) for st in c.relevel_plan()] == c.relevel_steps()
    c.setVerify(True)
    c.setDeviceVerify(True)                  # the checks run on the device: no host-side pass
    assert c.xorSharedActive() and sum(c.relevel_steps()) == 10
    c.setDeviceVerify(False)
    c.setVerify(False)
    c.setDataflow(True)                      # the dataflow kernel has no pairs: the step schedule runs
    assert c.xorSharedActive() and not c.dataflowActive() and sum(c.relevel_steps()) == 10
    # plaintext evaluation is untouched by the option
    c.Reset()
    c.setPlaintext(True)
    c.setEncrypted(False)
    c.SetInput([[1, 1], [0, 1]])
    o = c.Clock()[0]
    assert o[0] + 2 * o[1] + 4 * o[2] == 5
    with pytest.raises(bce.BceError) as e:   # the lowering is chosen before SetInput
        c.setXorShared(False)
    assert e.value.code == bce.ERR_STATE
    c.close()
