// dag_build.cpp -- see dag_build.hpp
#include "dag_build.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "desc.hpp"

namespace bce {
namespace {

using u32 = uint32_t;
using u64 = uint64_t;

DagBuildStatus refuse(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return {code, buf};
}

}  // namespace

DagBuildStatus build_dag(u32 n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bool allow_pairs, u32 n_classes, DagBuild& out) {
    out = DagBuild{};
    u64 max_slot64 = 0;
    for (u32 i = 0; i < n_tasks; ++i) {
        const bce_gate_desc& g = tasks[i];
        const DescKind k = desc_kind(g.op);
        if (k.pair() && !allow_pairs) return refuse(BCE_ERR_UNSUPPORTED, "bce_dag_create: task %u is a pair descriptor (BCE_PAIR): bce_dag_create_pairs takes them, or use bce_eval_gates or a bce_plan", i);
        if (!k.boot()) return refuse(BCE_ERR_ARG, "bce_dag_create: task %u is not a bootstrapped gate (op %u)", i, g.op);
        if (prio && prio[i] >= n_classes) return refuse(BCE_ERR_ARG, "bce_dag_create: task %u has priority class %u (0..%u)", i, prio[i], n_classes - 1);
        max_slot64 = std::max(max_slot64, top_slot(g, k));
    }
    if (max_slot64 >= 0xFFFFFFFFull) return refuse(BCE_ERR_POOL, "bce_dag_create: slot %llu outside any pool", (unsigned long long)max_slot64);
    const u32 max_slot = (u32)max_slot64;
    // producers by slot
    std::vector<int32_t> writer((size_t)max_slot + 1, -1);
    std::vector<uint8_t> read_before((size_t)max_slot + 1, 0);
    std::vector<u32> dep(n_tasks, 0), lvl(n_tasks, 1), cons_cnt(n_tasks + 1, 0);
    std::vector<int32_t> p0(n_tasks, -1), p1(n_tasks, -1);
    u32 depth = 0;
    for (u32 i = 0; i < n_tasks; ++i) {
        const bce_gate_desc& g = tasks[i];
        const DescKind k = desc_kind(g.op);
        p0[i] = writer[g.in0]; read_before[g.in0] = 1;
        if (k.inputs == 2) { p1[i] = writer[g.in1]; read_before[g.in1] = 1; }
        if (p1[i] == p0[i]) p1[i] = -1;   // both outputs of one pair, or the same slot twice: one producer
        for (u32 o = g.out, last = g.out + (k.outputs - 1u); o <= last; ++o) {
            if (writer[o] >= 0) return refuse(BCE_ERR_ARG, "bce_dag_create: slot %u is written by tasks %d and %u (SSA form required)", o, writer[o], i);
            if (read_before[o]) return refuse(BCE_ERR_ARG, "bce_dag_create: task %u writes slot %u that an earlier task (or itself) reads", i, o);
            writer[o] = (int32_t)i;
        }
        for (int32_t p : {p0[i], p1[i]})
            if (p >= 0) { ++dep[i]; ++cons_cnt[p + 1]; lvl[i] = std::max(lvl[i], lvl[p] + 1); }
        depth = std::max(depth, lvl[i]);
    }
    std::vector<u32> cons_off(cons_cnt);
    for (u32 i = 0; i < n_tasks; ++i) cons_off[i + 1] += cons_off[i];
    std::vector<u32> cons(std::max<u32>(1, cons_off[n_tasks])), fill(cons_off.begin(), cons_off.end() - 1);
    for (u32 i = 0; i < n_tasks; ++i)
        for (int32_t p : {p0[i], p1[i]}) if (p >= 0) cons[fill[p]++] = i;
    std::vector<uint8_t> qid(n_tasks, 0);
    if (prio) qid.assign(prio, prio + n_tasks);

    out.init_off.assign(n_classes + 1, 0);
    out.qcount.assign(n_classes, 0);
    for (u32 q = 0; q < n_classes; ++q) {
        out.init_off[q] = (u32)out.init_items.size();
        for (u32 i = 0; i < n_tasks; ++i) {
            if (qid[i] != q) continue;
            ++out.qcount[q];
            if (dep[i] == 0) out.init_items.push_back(i);
        }
    }
    out.init_off[n_classes] = (u32)out.init_items.size();
    if (out.init_items.empty()) return refuse(BCE_ERR_ARG, "bce_dag_create: no task is ready at the start");
    out.n_tasks = n_tasks; out.max_slot = max_slot; out.depth = depth;
    out.dep = std::move(dep); out.cons_off = std::move(cons_off); out.cons = std::move(cons); out.qid = std::move(qid);
    return {};
}

}  // namespace bce
