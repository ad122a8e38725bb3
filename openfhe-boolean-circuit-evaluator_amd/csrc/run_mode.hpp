// run_mode.hpp -- what the next Clock() of a Circuit runs: ONE pure function of the caller's choices and four facts.
// Host-only: no engine call, no state.  Everything in circuit.* that asks about the mode (the public predicates,
// xorMode(), the branch in Clock(), the sharding plan) reads a RunMode from resolve_mode(); DESIGN.md 5.1 has the table.
#pragma once
#include <cstdint>

#include "schedule.hpp"   // sched::XorMode

namespace bce {

enum class XorChoice : uint8_t { None, Fast, Shared, Single };   // setXorFast / setXorShared / setXorSingle: one at a time

struct ModeInputs {
    // the caller's choices (the setters of Circuit)
    bool plaintext = false, encrypted = false, verify = false;
    bool batched = true;   // one launch per frontier; false: one Gate::Evaluate per gate, as the reference
    bool relevel = true;   // the bootstrap-depth schedule (same registers, fewer dependent launches); false: the reference's gate-level rounds
    bool graph = false, device_verify = false;
    bool dataflow = false, dataflow_shared = false;
    XorChoice xor_choice = XorChoice::None;
    // facts about the circuit
    bool engine = false;          // it has an engine (not plaintext-only)
    bool dag_supported = false;   // ... whose parameter class has the persistent kernel (bce_dag_supported)
    bool gate_sharded = false;    // every step's / level's gates are split over ranks
    bool tasks = false;           // a dataflow task list exists for the units
};

enum class RunPath : uint8_t { Rounds, Steps, Dag };   // gate-level rounds, bootstrap-depth step schedule, dataflow kernel

struct RunMode {
    RunPath path;              // the branch Clock() takes
    sched::XorMode xor_mode;   // the lowering the units are built for: Shared = xorSharedActive()
    bool device_checks;        // verify mode checked on the device: deviceVerifyActive()
    bool graph;                // the steps replay as one hipGraph: graphActive()
    bool dataflow;             // the dataflow schedule is chosen and available: dataflowActive()
};

// `dataflow` and `graph` do not read plaintext / encrypted / batched, `path` does: they can be set where Clock() runs
// the rounds.  The step schedule also runs with relevel off when dataflow is chosen but not available.
inline RunMode resolve_mode(const ModeInputs& m) {
    const bool shared = m.xor_choice == XorChoice::Shared && m.batched && m.relevel && !m.gate_sharded && !(m.verify && !m.device_verify);
    const bool checks = m.device_verify && m.verify && m.encrypted && m.engine && m.batched && m.relevel && !m.gate_sharded;
    const bool verify_ok = !m.verify || checks;   // no host-side verify pass
    const bool dataflow = m.dataflow && (!shared || m.dataflow_shared) && m.engine && verify_ok && !m.gate_sharded && m.dag_supported && m.tasks;
    const bool graph = m.graph && m.engine && m.relevel && !dataflow && verify_ok && !m.gate_sharded;
    const bool scheduled = ((m.relevel || m.dataflow) && m.encrypted && !m.plaintext && m.batched) || checks;
    const sched::XorMode xor_mode = m.xor_choice == XorChoice::Fast ? sched::XorMode::Fast : m.xor_choice == XorChoice::Single ? sched::XorMode::Single
                                  : shared ? sched::XorMode::Shared : sched::XorMode::Reference;
    return {!scheduled ? RunPath::Rounds : dataflow ? RunPath::Dag : RunPath::Steps, xor_mode, checks, graph, dataflow};
}

}  // namespace bce
