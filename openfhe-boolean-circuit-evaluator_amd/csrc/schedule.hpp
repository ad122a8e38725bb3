// schedule.hpp -- host-only scheduling of a gate DAG: which bootstrap runs in which step, on which rank, in which slot.
// Pure functions over plain data: no engine call, no environment, no output.  From the engine's header only the
// descriptor struct and the BCE_* op codes are used, so the module compiles and is tested on its own
// (tests/integration/schedule_selftest.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bce_gpu.h"

namespace bce::sched {

enum class Op : uint8_t { NOT, AND, OR, XOR, OUTPUT };
struct DagGate { Op op; int in0, in1, out; };   // in1 = -1 for NOT / OUTPUT, out = -1 for OUTPUT
struct Dag {
    uint32_t n_wires = 0;
    std::vector<DagGate> gates;        // level order, file order within a level
    std::vector<uint32_t> level_off;   // gates[level_off[l] .. level_off[l + 1]) = level l
    std::vector<int> outputs;          // the wires the OUTPUT gates read, in FILE order
};

// How an XOR gate is evaluated.  Reference: the reference's three bootstraps (src/gate.cpp:198-202).  Fast: one XOR_FAST
// bootstrap of 2 (ct1 - ct2) (eight times the input variance).  Shared: AND(OR(a, b), NAND(a, b)) with the OR and the NAND
// from ONE blind rotation (a BCE_PAIR descriptor): two blind rotations, the same depth and the same inputs' noise as Reference.
// Single: one BCE_XOR bootstrap of ct1 + ct2 (three-level test polynomial, include/bce_gpu.h): depth 1, a plain gate's noise.
enum class XorMode : uint8_t { Reference, Fast, Shared, Single };
inline XorMode xor_mode(bool xor_fast) { return xor_fast ? XorMode::Fast : XorMode::Reference; }
uint32_t gate_weight(Op op, XorMode mode);   // blind rotations per gate (src/gate.cpp:133,172,200-202)
inline uint32_t gate_weight(Op op, bool xor_fast) { return gate_weight(op, xor_mode(xor_fast)); }
// the two places that spell an XOR, with u's own negations folded in:
//   (a AND !b) -> t1, (!a AND b) -> t2, then t1 OR t2 -> u.out
void xor_lower(const bce_gate_desc& u, uint32_t t1, uint32_t t2, bce_gate_desc out[3]);
//   the pair (a OR b) -> t, (a NAND b) -> t + 1 from one blind rotation, then t AND (t + 1) -> u.out
void xor_lower_shared(const bce_gate_desc& u, uint32_t t, bce_gate_desc out[2]);

// Units of the schedule: a single bootstrap (AND / OR / XOR_FAST / BCE_XOR; its output is ready one step later) or an XOR of lat 2:
// built as the reference builds it (two ANDs in step `start`, their OR in step start + 1) or, `shared`, as a pair in step
// `start` and an AND in step start + 1; d holds in0, in1, out, neg0, neg1.
struct Unit {
    uint32_t asap, start;
    uint8_t lat, owner;
    bce_gate_desc d;
    int32_t p0, p1;   // producing units of the inputs, -1 = primary input / constant
    uint8_t shared = 0;
    uint32_t weight() const { return lat == 2 && !shared ? 2 : 1; }   // blind rotations in the unit's start step
};
struct Units {   // a function of (netlist, XOR mode) except Unit::start and Unit::owner, which placement and assign_owners set
    std::vector<Unit> units;             // topological order
    std::vector<int> base;               // wire -> wire at the bottom of its NOT chain
    std::vector<uint8_t> neg;            // wire -> parity of that chain
    uint32_t depth = 0;                  // bootstrap depth D = steps of the schedule
    std::vector<uint32_t> soff, succ, alap;   // successors (CSR) and ALAP start steps
};
Units build_units(const Dag&, XorMode mode);
inline Units build_units(const Dag& dag, bool xor_fast) { return build_units(dag, xor_mode(xor_fast)); }
inline void place_asap(Units& S) { for (auto& u : S.units) u.start = u.asap; }
// the same D steps filled by SLACK: a step of K x count bootstraps is topped up to the next stair of the launch staircase
// (`lone` bootstraps cost one latency, then one round per `full`) with the ready units of least slack
void place_by_slack(Units&, uint64_t K, uint32_t lone, uint32_t full);
// gate sharding: split every step's units over `world` ranks; locality = follow the inputs' ranks unless that publishes more
void assign_owners(Units&, uint32_t world, bool locality);
std::vector<uint8_t> crossing(const Units&);   // per unit: a consumer unit sits on another rank

struct StepPlan {
    std::vector<std::vector<bce_gate_desc>> steps;
    std::vector<bce_gate_desc> output_nots;                  // NOT wires that OUTPUT gates read: materialised at the end
    std::vector<std::vector<std::vector<int>>> publish;      // [step][rank] -> wires that rank publishes after the step
    uint32_t stride = 0, K = 0;
};
StepPlan lower_steps(const Units&, const Dag&, uint32_t rank, uint32_t world, uint64_t K);   // world 1 = not sharded
struct TaskList { std::vector<bce_gate_desc> tasks; std::vector<uint8_t> prio; uint32_t stride = 0; };
// SSA: every XOR owns its two temporaries n_wires + 2 x, n_wires + 2 x + 1; prio = slack class of the unit.  pairs: the caller
// hands the list to bce_dag_create_pairs, so a shared XOR is lowered to its pair descriptor and its AND (two tasks, both of the
// unit's class); without it shared units are refused (std::logic_error), because bce_dag_create refuses pair descriptors
TaskList lower_tasks(const Units&, uint32_t n_wires, bool pairs = false);
// every step reads only what earlier steps wrote (or received), every XOR temporary is read one step after it is written; a
// pair descriptor writes two adjacent temporaries
bool check(const StepPlan&, const Dag&, uint32_t rank, uint32_t world, std::string* why = nullptr);

// Verify mode on the step schedule (the reference decrypts and compares every GATE output, src/gate.cpp:153-160): per step,
// the descriptors whose `out` is a netlist wire -- AND, OR, the final OR (AND, in shared mode) of a lowered XOR, XOR_FAST /
// XNOR_FAST / BCE_XOR -- as the register they write and the gate (index into Dag::gates) that owns it.  An XOR's two temporaries are not listed.  NOT
// gates have no register on this schedule: a wrong NOT input shows at its consumer.
struct CheckLists {
    std::vector<std::vector<uint32_t>> wires;   // [step] -> registers written in that step, in descriptor order
    std::vector<std::vector<uint32_t>> gates;   // [step] -> owning gate of each
};
CheckLists check_lists(const StepPlan&, const Dag&);
// The same checks on the dataflow schedule: one per task whose `out` is a netlist wire, in task order -- the task (index into
// TaskList::tasks), the register it writes and the owning gate.  As a set of (wire, gate) pairs it equals check_lists of
// any step plan lowered from the same units; the check runs when the task completes, before its consumers are released.
struct TaskChecks { std::vector<uint32_t> tasks, wires, gates; };
TaskChecks task_checks(const TaskList&, const Units&, const Dag&);

// gate sharding of the gate-LEVEL rounds: owner of every gate of a level (0xFF = everyone: OUTPUT), publications after it
struct LevelShard {
    std::vector<std::vector<uint8_t>> owner;                 // [level][k]
    std::vector<std::vector<std::vector<int>>> publish;      // [level][rank]
};
LevelShard shard_levels(const Dag&, uint32_t world, XorMode mode);
inline LevelShard shard_levels(const Dag& dag, uint32_t world, bool xor_fast) { return shard_levels(dag, world, xor_mode(xor_fast)); }

}  // namespace bce::sched
