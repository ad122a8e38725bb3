// circuit.hpp -- host circuit runtime: Wire, Gate, GateEvalParams, Circuit.
//
// Keeps the reference's driver API (src/wire.h:48-69, src/gate.h:50-80, src/circuit.h:54-114)
// with two deliberate differences:
//   * `CipherText` is a slot of the engine's device-resident LWE pool (include/bce_gpu.h)
//     instead of lbcrypto::LWECiphertext (src/wire.h:46);
//   * the DAG is indexed (gate ids, CSR fan-out, ready counters) and levelised once, and the
//     executor hands each ready frontier to bce_eval_gates() instead of one OpenMP task per
//     gate (src/circuit.cpp:698-710).  The O(G^2) netlist build (src/circuit.cpp:323-354) and
//     the O(wires x waiting gates) manager scan (src/circuit.cpp:593-677) are not inherited.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bce_circuit.h"
#include "../../include/bce_gpu.h"
#include "run_mode.hpp"
#include "schedule.hpp"

namespace bce {

using NameList = std::vector<std::string>;
using CipherText = uint32_t;  // pool slot (reference: lbcrypto::LWECiphertext)
constexpr CipherText kNoCipherText = 0xFFFFFFFFu;

// src/wire.h:48-69
class Wire {
public:
    void setName(const std::string& n) { name = n; }
    std::string getName() const { return name; }
    void setValue(bool b) { value = b; }
    bool getValue() const { return value; }
    void setFanoutGates(const NameList& f) { fanoutGates = f; }
    NameList getFanoutGates() const { return fanoutGates; }
    unsigned int getNumberFanoutGates() const { return (unsigned int)fanoutGates.size(); }
    void setCipherText(CipherText c) { ct = c; }
    CipherText getCipherText() const { return ct; }
    // erases the first match, or reports an error (src/wire.cpp:54-65)
    void updateFanoutGates(const std::string& gateToRemove);

private:
    std::string name;
    NameList fanoutGates;
    bool value = false;
    CipherText ct = kNoCipherText;
};

using ReadyList = std::vector<bool>;
using CipherTextList = std::vector<CipherText>;
using BitList = std::vector<unsigned int>;

enum class GateEnum { INPUT, OUTPUT, NOT, AND, OR, XOR, DFF, LUT3, LUT4 };  // src/gate.h:50

// src/gate.h:52-63; `cc` is the engine handle and plays BinFHEContext + secret key
class GateEvalParams {
public:
    bool plaintext_flag = false;
    bool encrypted_flag = false;
    bool verify_flag = false;
    bce_ctx* cc = nullptr;
    bool xor_fast = false;            // opt-in: XOR as ONE bootstrap of 2*(ct1-ct2) (BCE_XOR_FAST), not the reference's 3
    bool xor_single = false;          // opt-in: XOR as ONE bootstrap of ct1+ct2 (BCE_XOR, three-level test polynomial)
    int encrypt_mode = BCE_BOOTSTRAPPED;  // output mode of the verify-mode re-encryptions (cc.Encrypt(sk, bit), src/gate.cpp:118,...)
    uint64_t* enc_counter = nullptr;  // PRNG stream index for verify-mode re-encryptions
    unsigned int* fixes = nullptr;    // counts "Bad <OP> fixing" events
};

// src/gate.h:65-80
class Gate {
public:
    void Reset() {}
    // plaintext logic and/or encrypted logic for this one gate (src/gate.cpp:49-229).
    // Encrypted: encout[0] must hold the destination slot; XOR also needs tmp[0], tmp[1].
    void Evaluate(const GateEvalParams&);
    std::string name;
    GateEnum op = GateEnum::INPUT;
    NameList inWireNames;
    ReadyList ready;
    NameList outWireNames;
    CipherTextList encin;
    BitList plainin;
    CipherTextList encout;
    BitList plainout;
    CipherTextList tmp;  // scratch slots for the XOR expansion
};

using Inputs = std::vector<std::vector<unsigned int>>;
using Outputs = std::vector<std::vector<unsigned int>>;
using NetList = std::map<std::string, NameList>;

// a combination of options the runtime does not implement: BCE_ERR_UNSUPPORTED at the C boundary
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };

class Circuit {
public:
    // Circuit(set, method), src/circuit.cpp:45-98: creates the engine on device 0 and generates
    // keys.  Accepts only TOY / STD128_OPT and AP / GINX like the reference; throws otherwise.
    Circuit(int paramset, int method);
    // shares an existing engine (keys already generated); nullptr = plaintext-only circuit
    explicit Circuit(bce_ctx* engine);
    ~Circuit();

    bool ReadFile(const std::string& cktName);                 // src/circuit.cpp:102-366
    bool ReadBristol(const std::string& path, bool new_flag);  // direct netlist -> DAG
    void Reset();                                              // src/circuit.cpp:368-419
    void SetInput(const Inputs& input, bool verbose = false);  // src/circuit.cpp:455-530
    void SetInput(unsigned instance, const Inputs& input, bool verbose = false);
    void setPlaintext(bool b) { opt_.plaintext = b; }
    bool getPlaintext() const { return opt_.plaintext; }
    void setEncrypted(bool b) { opt_.encrypted = b; }
    bool getEncrypted() const { return opt_.encrypted; }
    void setVerify(bool b);                                    // src/circuit.cpp:833-840
    bool getVerify() const { return opt_.verify; }
    Outputs Clock();                                           // src/circuit.cpp:532-573
    void dumpNetList() const;
    void dumpGates() const;
    void dumpGateCount() const;

    // ---- extensions --------------------------------------------------------------
    void setInstances(unsigned k);            // K lock-step input sets (before SetInput)
    // Per-instance key sets (bce_gpu.h, "key sets"): instance k is encrypted, evaluated and decrypted under set ids[k] of the
    // engine.  Before SetInput, one id per instance; an empty list returns to the selected set.  Clock() then runs the
    // bootstrap-depth step schedule keyed (bce_plan_create_keyed; setGraph on top).  Not together with setDataflow, setVerify,
    // setDeviceVerify or gate sharding: Unsupported, from this setter, from those setters and at SetInput.
    void setInstanceKeys(const std::vector<uint32_t>& ids);
    const std::vector<uint32_t>& getInstanceKeys() const { return instance_keys_; }
    unsigned getInstances() const { return instances_; }
    // ---- what a Clock() runs.  The setters below record choices; which path, XOR lowering, device checks and graph
    // replay result from them is decided in ONE place, resolve_mode() in run_mode.hpp (table: DESIGN.md 5.1), and the
    // four ...Active() predicates report its answer for the next Clock().
    void setBatched(bool b) { setModeFlag(opt_.batched, b, "setBatched"); }   // false: one Gate::Evaluate per gate
    // cc.Encrypt(sk, bit) of SetInput (src/circuit.cpp:506) and of the verify-mode repairs (src/gate.cpp:118,139,143,158,179,211):
    // BCE_BOOTSTRAPPED by default, as OpenFHE v1.0.x's Encrypt defaults to BOOTSTRAPPED (one Bootstrap per fresh ciphertext);
    // BCE_FRESH is the opt-in that skips it
    void setEncryptMode(int mode) { encrypt_mode_ = mode; }
    int getEncryptMode() const { return encrypt_mode_; }
    // The XOR lowering: ONE choice, three opt-in setters (std::invalid_argument when another one is on).
    //   setXorFast:   OpenFHE's XOR_FAST gate, one bootstrap of 2 (ct1 - ct2); NOT the reference's semantics
    //                 (src/gate.cpp:194-196 disables it "for now" because of its higher failure rate).
    //   setXorShared: AND(OR(a, b), NAND(a, b)) with the OR and the NAND from one blind rotation (a BCE_PAIR descriptor):
    //                 two rotations per XOR instead of three, the same two steps, the same BIT on every netlist wire.
    //                 Before SetInput (std::logic_error after).  Where it is not active (xorSharedActive()) the reference
    //                 lowering runs.  The lowering and the pool layout are fixed at SetInput: setBatched, setRelevel,
    //                 setDeviceVerify and setVerify are refused after it (std::logic_error, the flag keeps its value)
    //                 where they would change xorSharedActive().  Reset() lifts that.
    //   setXorSingle: one BCE_XOR bootstrap of ct1 + ct2 (three-level test polynomial, bce_gpu.h): XOR_FAST's count and
    //                 depth at a plain gate's noise, on every path XOR_FAST runs on.  Before SetInput (std::logic_error after).
    void setXorFast(bool b) { chooseXor(XorChoice::Fast, b, false); }
    void setXorShared(bool b) { chooseXor(XorChoice::Shared, b, true); }
    void setXorSingle(bool b) { chooseXor(XorChoice::Single, b, true); }
    XorChoice getXorChoice() const { return opt_.xor_choice; }
    bool xorSharedActive() const { return xorMode() == sched::XorMode::Shared; }
    // opt-in: schedule by BOOTSTRAP depth instead of gate level -- NOT gates are folded into their
    // consumers' prep (neg flags) and an XOR's OR shares a launch with the next level's ANDs.  Same
    // ciphertexts as the level schedule (EvalNOT is deterministic), fewer dependent launches.
    void setRelevel(bool b) { setModeFlag(opt_.relevel, b, "setRelevel"); }
    bool getRelevel() const { return opt_.relevel; }
    // the bootstrap-depth schedule fills its steps by slack up to the launch staircase of the engine (default on; see
    // sched::place_by_slack).  lone / full = 0: ask the engine (bce_launch_capacity), else use these capacities (tests).
    void setBalance(bool on, uint32_t lone = 0, uint32_t full = 0) { balance_ = on; cap_lone_ = lone; cap_full_ = full; rebuildRelevel(); }
    // opt-in: hand the engine the whole bootstrap DAG (bce_dag_*): ONE persistent launch per Clock() in which a finished
    // bootstrap releases its consumers on the device -- the ready-gate rule of the reference's manager
    // (src/circuit.cpp:575-683) applied per gate instead of per frontier.  Same ciphertexts in every register as the
    // other schedules.  XOR temporaries get slots of their own (SSA), so choose it before SetInput (switching it off and
    // on again later keeps that layout).  Where it is not available (dataflowActive()) the step schedule runs.
    void setDataflow(bool b);
    bool getDataflow() const { return opt_.dataflow; }
    // opt-in on top of setDataflow and setXorShared: keep the shared lowering on the dataflow schedule, as pair tasks
    // (bce_dag_create_pairs: per XOR a pair task and an AND, the same slot stride).  Without it the two options together
    // run the step schedule.  Before SetInput (std::logic_error after, if it would change).
    void setDataflowShared(bool b);
    bool getDataflowShared() const { return opt_.dataflow_shared; }
    // opt-in: replay the bootstrap-depth schedule's launches as ONE hipGraph per Clock() (bce_plan_run) instead of one
    // host call per step.  Same ciphertexts.
    void setGraph(bool b) { opt_.graph = b; }   // (with setInstanceKeys: the keyed plan's graph)
    bool getGraph() const { return opt_.graph; }
    bool graphActive() const { return runMode().graph; }
    // opt-in: verify mode (src/gate.cpp:153-160: decrypt every gate output, compare with the plaintext pass, "Bad <OP> fixing",
    // replace) checked ON THE DEVICE between the steps of the bootstrap-depth schedule (bce_plan_set_checks), or inside the
    // persistent kernel with setDataflow, instead of the gate-level rounds with one host decryption per level.  Differences
    // to the host path: a repaired register holds the trivial ciphertext of the right bit (bce_gpu.h), and NOT gates have no
    // register on these schedules, so a wrong NOT input is caught at its consumer -- fix counts can differ for that reason.
    void setDeviceVerify(bool b) { if (b) refuseWithKeys("setDeviceVerify"); setModeFlag(opt_.device_verify, b, "setDeviceVerify"); }
    bool getDeviceVerify() const { return opt_.device_verify; }
    bool deviceVerifyActive() const { return runMode().device_checks; }
    const bce_check_report& checkReport() const { return check_report_; }   // of the last Clock() on the device path
    bool dataflowActive() const { return runMode().dataflow; }
    RunMode runMode() const;                  // resolve_mode() of the choices and this circuit's facts
    const std::vector<bce_gate_desc>& dataflowTasks() const { return tasks_.tasks; }
    const std::vector<uint8_t>& dataflowPriorities() const { return tasks_.prio; }
    bool getBalance() const { return balance_; }
    std::vector<uint32_t> relevelStepSizes() const;          // bootstraps per step, one instance
    const std::vector<std::vector<bce_gate_desc>>& relevelStepDescs() const { return steps_.steps; }   // this rank's descriptors, instance 0
    std::vector<uint32_t> relevelPublications() const;       // registers this rank publishes per step (gate sharding)
    bool checkRelevelPlan(std::string* why = nullptr) const { return sched::check(steps_, net_, rank_, gateSharded() ? world_ : 1, why); }
    void setQuiet(bool q) { quiet_ = q; }
    // re-arm for another Clock() on the SAME inputs: keeps mode flags and the input ciphertexts
    // already resident in the device pool (registers are SSA, inputs are never overwritten)
    void Rearm();
    Outputs getOutputs(unsigned instance) const;
    void getCounts(uint32_t out[6]) const;
    const bce_circuit_stats& stats() const { return stats_; }
    bce_circuit_info info() const;
    const std::vector<unsigned>& inputBusBits() const { return n_in_bits_; }
    const std::vector<unsigned>& outputBusBits() const { return out_bus_bits_; }
    void setExchange(uint32_t rank, uint32_t world, int shard_mode, bce_allgather_fn fn, void* user, void* host_send,
                     void* host_recv, void* dev_send, void* dev_recv, uint64_t capacity);
    uint64_t exchangeCapacity(uint32_t world, int shard_mode, bool encrypted) const;
    void enableRccl(bool on) { rccl_ = on; }
    // gate sharding: place a unit on the rank that produced (most of) its inputs, within the fair share of each step
    // (default); off = contiguous split in netlist order.  Every rank must choose the same.
    void setShardLocality(bool on) { shard_locality_ = on; if (world_ > 1) rebuildRelevel(); }
    bool getShardLocality() const { return shard_locality_; }
    // digest of everything the ranks of a gate-sharded run must agree on (owners, publications per step, slot stride,
    // instances): ranks whose devices or environment knobs differ would otherwise build different plans and exchange
    // buffers of different sizes -- compare it across ranks before the first Clock()
    uint64_t planHash() const;
    bce_ctx* engine() const { return cc; }

private:
    struct GateRec {
        GateEnum op;
        int nin;
        int in[2];
        int out;      // wire id, -1 for OUTPUT
        int out_bit;  // OUTPUT only
        std::string name;
    };
    struct LoadRec { unsigned bus, bit; int wire; std::string name; };
    struct ConstRec { int wire; unsigned value; };  // Bristol Fashion EQ: a public constant, no gate
    struct Level {
        std::vector<int> gates;  // file order
        uint32_t n_xor = 0;
    };

    bce_ctx* cc = nullptr;
    bool owns_engine_ = false;
    ModeInputs opt_;   // the caller's choices; the facts are filled in by runMode()
    bool done = false, inputs_set_ = false, quiet_ = false;
    int encrypt_mode_ = BCE_BOOTSTRAPPED;

    std::vector<LoadRec> inputGates;  // LOADs
    std::vector<ConstRec> constWires_; // constants (live from the start, like inputs)
    std::vector<GateRec> allGates;    // everything else, file order
    std::vector<std::string> wire_names_;
    std::map<uint32_t, int> wire_of_reg_;
    std::vector<uint32_t> fan_off_, fan_gate_;  // CSR wire -> consumer gates
    std::vector<Level> levels_;
    uint32_t max_level_xor_ = 0, stride_ = 0;
    std::vector<unsigned> n_output_bits;
    std::vector<unsigned> n_in_bits_;      // width of every input bus (In1, In2, ...)
    std::vector<unsigned> out_bus_bits_;   // width of every output bus; output bit indices run over their concatenation
    unsigned n_buses_ = 0;

    unsigned instances_ = 1;
    std::vector<uint32_t> instance_keys_;           // setInstanceKeys: [instances_] key-set ids, or empty
    void refuseWithKeys(const char* who) const;     // Unsupported when instance keys are set
    void keysCombinationSupported(const char* who) const;   // Unsupported when instance keys meet dataflow, verify, device verify or gate sharding
    std::vector<std::vector<uint8_t>> plain_;       // [instance][wire]
    std::vector<std::vector<uint8_t>> circuitOut;   // [instance][bit]
    uint64_t enc_counter_ = 0, epoch_ = 0;
    unsigned n_input_gates = 0, n_output_gates = 0, n_and_gates = 0, n_or_gates = 0, n_xor_gates = 0, n_not_gates = 0;
    bce_circuit_stats stats_{};
    std::string err_;

    // multi-rank
    uint32_t rank_ = 0, world_ = 1;
    int shard_mode_ = 0;
    bce_allgather_fn xfn_ = nullptr;
    void* xuser_ = nullptr;
    void *host_send_ = nullptr, *host_recv_ = nullptr, *dev_send_ = nullptr, *dev_recv_ = nullptr;
    uint64_t xcap_ = 0;
    bool rccl_ = false;  // device payloads through bce_rccl_allgather on the engine stream (no host sync, no callback)
    bool shard_locality_ = true;  // gate sharding on the bootstrap-depth schedule: a unit goes to the rank that produced its inputs
    sched::LevelShard shard_;     // gate-level rounds under gate sharding: owner of levels_[level].gates[k], publications per level
    bool gateSharded() const { return world_ > 1 && shard_mode_ == 1; }       // every step's / level's gates are split over the ranks
    bool instanceSharded() const { return world_ > 1 && shard_mode_ == 0; }   // every rank evaluates its share of the instances

    int addWire(uint32_t reg);
    int wireOf(uint32_t reg, const char* what, unsigned lineNo) const;
    void finalizeNetlist();
    void buildShardPlan();
    std::pair<unsigned, unsigned> instanceRange() const;   // [lo, hi): the instances this rank evaluates
    sched::Dag net_;          // the levelised netlist as the schedule module reads it
    sched::Units units_;      // rebuilt when the netlist or the XOR mode changes
    sched::XorMode units_mode_ = sched::XorMode::Reference;   // the mode units_ were built for
    sched::XorMode xorMode() const { return runMode().xor_mode; }
    void buildUnits() { units_mode_ = xorMode(); units_ = sched::build_units(net_, units_mode_); tasks_ = {}; }
    void syncXorMode();       // after a change of anything xorMode() reads: units and schedules for the mode that now holds
    void chooseXor(XorChoice which, bool on, bool before_input);
    void setModeFlag(bool& flag, bool b, const char* who);   // sets one of those flags; refused after SetInput where it would switch the lowering
    sched::StepPlan steps_;   // bootstrap-depth schedule: redone when K, capacities, world, locality or balance change
    sched::TaskList tasks_;   // dataflow schedule: held only while it is chosen
    uint32_t base_stride_ = 0;
    bool balance_ = true;
    uint32_t cap_lone_ = 0, cap_full_ = 0;
    std::pair<uint32_t, uint32_t> launchCapacity() const;   // (lone, full) of the launch staircase: set by the caller, else the engine's
    bool tasksHavePairs() const { return units_mode_ == sched::XorMode::Shared; }          // of a task list lowered from units_
    bool tasksExist() const { return !tasksHavePairs() || opt_.dataflow_shared; }              // the dataflow schedule has a list for units_
    sched::TaskList lowerTasks() const { return sched::lower_tasks(units_, net_.n_wires, tasksHavePairs()); }
    void createDag(bce_dag** g);               // bce_dag_create, or bce_dag_create_pairs for a list with pairs
    bce_dag* dag_ = nullptr;
    bce_plan* plan_ = nullptr;                 // the schedule's descriptors resident on the device (and its captured graph)
    uint32_t plan_lo_ = 0, plan_K_ = 0, plan_stride_ = 0;
    bce_plan* vplan_ = nullptr;                // the same schedule with the check lists of device verify mode attached (its own capture)
    bool vplan_checks_ = false;                // ... once they are attached
    void dropPlan() { for (bce_plan** p : {&plan_, &vplan_}) if (*p) { bce_plan_destroy(cc, *p); *p = nullptr; } vplan_checks_ = false; }
    bce_dag* vdag_ = nullptr;                  // the same DAG with the checks of device verify mode attached
    sched::TaskChecks task_checks_;            // of vdag_
    void dropDag() { for (bce_dag** g : {&dag_, &vdag_}) if (*g) { bce_dag_destroy(cc, *g); *g = nullptr; } }
    void clockDag(bool verify);
    void reportChecks(const std::vector<std::vector<uint32_t>>* by_tag, const std::vector<uint32_t>* by_index);   // read the report, print and count the mismatches
    void compareOutputs(unsigned lo, unsigned hi);   // verify mode: OUTPUT gates against the plaintext pass
    std::vector<uint8_t> armChecks(unsigned lo, unsigned hi, const std::vector<uint32_t>& wires);   // expected bits per instance; check reset
    void finishReleveled(unsigned lo, unsigned hi, bool verify);
    void rebuildRelevel();
    std::vector<bce_gate_desc> rebased(std::vector<bce_gate_desc> descs, unsigned lo) const;   // descriptors of instance 0 -> instance lo
    void evalStrided(const std::vector<bce_gate_desc>& descs, unsigned lo, uint32_t K, const char* what);   // one launch, if any
    void decryptOutputs(unsigned lo, unsigned hi, const std::vector<int>* gates);   // OUTPUT gates among `gates` (nullptr: all) -> circuitOut
    void countGates(const std::vector<int>* gates);
    void clockSteps(bool verify);
    std::vector<std::vector<uint32_t>> check_gates_;   // of vplan_: per NON-EMPTY step of steps_ (= per step of the plan), the owning gates
    std::vector<uint32_t> check_wires_;                // ... and the registers checked, step after step
    bce_check_report check_report_{};
    void ensurePlan(bce_plan*& plan, unsigned lo, uint32_t K);  // the schedule's descriptors resident on the device
    void plainRound(size_t level);             // the plaintext pass of one gate level
    void managerRound(size_t level);
    void executeRound(size_t level);
    void exchangeWires(const std::vector<std::vector<int>>& pub);
    void gatherOutputs();
    void requireEngine(const char* what) const;
    void ck(int rc, const char* what) const;
    friend struct ::bce_circuit;
};

}  // namespace bce
