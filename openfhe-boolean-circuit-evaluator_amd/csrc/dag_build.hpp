// dag_build.hpp -- host-only dependency analysis of a task list for the dataflow schedule (bce_dag_create,
// bce_dag_create_pairs).  Plain data in, plain data out: no HIP header, no engine call, no environment, so the module
// compiles and is tested on its own (tests/integration/dag_build_selftest.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bce_gpu.h"

namespace bce {

// What the persistent kernel needs to know about a task list, as the engine uploads it
struct DagBuild {
    uint32_t n_tasks = 0;
    uint32_t max_slot = 0;                     // the highest slot a task touches
    uint32_t depth = 0;                        // longest producer chain (bootstraps)
    std::vector<uint32_t> dep;                 // producers per task (0, 1 or 2)
    std::vector<uint32_t> cons_off, cons;      // consumers (CSR): ascending, and through in0 before in1 within one consumer
    std::vector<uint8_t> qid;                  // priority class per task
    std::vector<uint32_t> init_items;          // initially ready tasks by class, task order within a class
    std::vector<uint32_t> init_off;            // [n_classes + 1] class q = init_items[init_off[q] .. init_off[q + 1])
    std::vector<uint32_t> qcount;              // [n_classes] tasks per class
};

// On refusal: the BCE_ERR_* code and the message of bce_dag_create
struct DagBuildStatus { int code = BCE_OK; std::string message; };

// The tasks must be in SSA form (a slot is written once and read only by later tasks), so that the order in which the device
// runs independent tasks cannot matter.  allow_pairs: a pair descriptor (BCE_PAIR) is a task with two outputs, `out` and
// `out + 1`; both count for max_slot, the SSA rule and the writers, so a later task that reads either output -- or both,
// like the AND of a shared XOR -- depends on the pair once.  One bootstrap, one item, one level of depth.
// prio: one class below n_classes per task, or null = class 0 everywhere.
DagBuildStatus build_dag(uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bool allow_pairs, uint32_t n_classes,
                         DagBuild& out);

}  // namespace bce
