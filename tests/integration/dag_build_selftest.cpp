// dag_build_selftest.cpp -- the dependency analysis of the dataflow schedule (csrc/dag_build.cpp) and the descriptor rule
// (csrc/desc.hpp) on their own: no engine, no GPU, no netlist reader.
//   1. hand-written task lists with the exact arrays the engine uploads (dep, cons_off, cons, qid, init_items, init_off, qcount)
//      and depth / max_slot;
//   2. random gate DAGs (the generator of schedule_dataflow_shared_selftest.cpp) through build_units -> lower_tasks in
//      Reference mode (no pairs) and in Shared mode (pairs), with a few refresh tasks appended, against a brute-force model
//      written here: the producers of a task are the earlier tasks one of whose output slots it reads.  Every array equal;
//   3. every refusal with its status code and its text;
//   4. the descriptor classifier over every op code, every legal and some illegal BCE_PAIR words.
// Compile with dag_build.cpp and schedule.cpp only:
//   c++ -std=c++17 dag_build_selftest.cpp ../../<package>/csrc/dag_build.cpp ../../<package>/csrc/schedule.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/dag_build.hpp"
#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/desc.hpp"
#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/schedule.hpp"

using namespace bce;
using namespace bce::sched;

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

typedef std::vector<uint32_t> V;
static const uint32_t kClasses = 4;
static const uint32_t kPair = BCE_PAIR(BCE_OR, BCE_NAND);

static bce_gate_desc T(uint32_t op, uint32_t in0, uint32_t in1, uint32_t out) { return bce_gate_desc{op, in0, in1, out, 0, 0}; }

static std::string show(const V& v) {
    std::string s = "{";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "}";
}
#define SAME(got, want, what) REQUIRE((got) == (want), "%s: %s is %s, expected %s", name, what, show(got).c_str(), show(want).c_str())

// ---- 1. hand-written lists ------------------------------------------------------------------------------------------
struct Want { V dep, cons_off, cons, init_items, init_off, qcount; uint32_t depth, max_slot; };

static void exact(const char* name, const std::vector<bce_gate_desc>& tasks, const std::vector<uint8_t>* prio, bool allow_pairs, const Want& w) {
    DagBuild b;
    const DagBuildStatus st = build_dag((uint32_t)tasks.size(), tasks.data(), prio ? prio->data() : nullptr, allow_pairs, kClasses, b);
    REQUIRE(st.code == BCE_OK && st.message.empty(), "%s: refused with %d: %s", name, st.code, st.message.c_str());
    REQUIRE(b.n_tasks == tasks.size(), "%s: n_tasks %u", name, b.n_tasks);
    SAME(b.dep, w.dep, "dep");
    SAME(b.cons_off, w.cons_off, "cons_off");
    SAME(b.cons, w.cons, "cons");
    SAME(b.init_items, w.init_items, "init_items");
    SAME(b.init_off, w.init_off, "init_off");
    SAME(b.qcount, w.qcount, "qcount");
    REQUIRE(b.depth == w.depth && b.max_slot == w.max_slot, "%s: depth %u (expected %u), max_slot %u (expected %u)", name, b.depth, w.depth, b.max_slot, w.max_slot);
    REQUIRE(b.qid == (prio ? *prio : std::vector<uint8_t>(tasks.size(), 0)), "%s: qid", name);
}

static void hand_written() {
    exact("one task", {T(BCE_AND, 0, 1, 2)}, nullptr, false,
          {{0}, {0, 0}, {0} /* never empty: one word at least */, {0}, {0, 1, 1, 1, 1}, {1, 0, 0, 0}, 1, 2});
    exact("chain of three", {T(BCE_AND, 0, 1, 2), T(BCE_OR, 2, 0, 3), T(BCE_NAND, 3, 2, 4)}, nullptr, false,
          {{0, 1, 2}, {0, 2, 3, 3}, {1, 2, 2}, {0}, {0, 1, 1, 1, 1}, {3, 0, 0, 0}, 3, 4});
    exact("one slot on both inputs", {T(BCE_AND, 0, 1, 2), T(BCE_XOR_FAST, 2, 2, 3)}, nullptr, false,
          {{0, 1}, {0, 1, 1}, {1}, {0}, {0, 1, 1, 1, 1}, {2, 0, 0, 0}, 2, 3});
    exact("pair, then the AND of both outputs", {T(kPair, 0, 1, 2), T(BCE_AND, 2, 3, 4)}, nullptr, true,
          {{0, 1}, {0, 1, 1}, {1}, {0}, {0, 1, 1, 1, 1}, {2, 0, 0, 0}, 2, 4});
    exact("pair, then one reader per output", {T(kPair, 0, 1, 2), T(BCE_AND, 2, 0, 4), T(BCE_OR, 1, 3, 5)}, nullptr, true,
          {{0, 1, 1}, {0, 2, 2, 2}, {1, 2}, {0}, {0, 1, 1, 1, 1}, {3, 0, 0, 0}, 2, 5});
    // in1 of a refresh is not an input: no dependency through it (tasks 1, 4), not marked as read (task 3 may write slot 4
    // that task 2 names), not counted for max_slot (task 4)
    exact("refresh ignores in1",
          {T(BCE_AND, 0, 1, 2), T(BCE_OP_REFRESH, 0, 2, 3), T(BCE_OP_REFRESH, 1, 4, 5), T(BCE_OR, 0, 1, 4), T(BCE_OP_REFRESH, 2, 0xFFFFFFFFu, 6)}, nullptr, false,
          {{0, 0, 0, 0, 1}, {0, 1, 1, 1, 1, 1}, {4}, {0, 1, 2, 3}, {0, 4, 4, 4, 4}, {5, 0, 0, 0}, 2, 6});
    const std::vector<bce_gate_desc> six = {T(BCE_AND, 0, 1, 10), T(BCE_OR, 0, 1, 11), T(BCE_AND, 10, 11, 12),
                                            T(BCE_NOR, 0, 1, 13), T(BCE_NAND, 0, 1, 14), T(BCE_OR, 13, 14, 15)};
    const std::vector<uint8_t> classes = {3, 1, 0, 1, 2, 3};
    exact("four classes, explicit", six, &classes, false,
          {{0, 0, 2, 0, 0, 2}, {0, 1, 2, 2, 3, 4, 4}, {2, 2, 5, 5}, {1, 3, 4, 0}, {0, 0, 2, 3, 4}, {1, 2, 1, 2}, 2, 15});
    exact("four classes, no priorities", six, nullptr, false,
          {{0, 0, 2, 0, 0, 2}, {0, 1, 2, 2, 3, 4, 4}, {2, 2, 5, 5}, {0, 1, 3, 4}, {0, 4, 4, 4, 4}, {6, 0, 0, 0}, 2, 15});
}

// ---- 2. random lists against a brute-force model ---------------------------------------------------------------------
static std::mt19937 rng(20251019u);
static uint32_t pick(uint32_t n) { return rng() % n; }

static Dag random_dag(uint32_t n_gates) {
    Dag dag;
    const uint32_t n_inputs = 1 + pick(6);
    std::vector<DagGate> g;
    std::vector<int> level(n_inputs, 0);   // per wire
    int wires = (int)n_inputs;
    auto add = [&](Op op, int a, int b) {
        const bool out = op != Op::OUTPUT;
        g.push_back({op, a, b, out ? wires : -1});
        if (out) { level.push_back(1 + std::max(level[a], b >= 0 ? level[b] : 0)); ++wires; }
    };
    while (g.size() < n_gates) {
        const uint32_t k = pick(10);
        const int a = (int)pick(wires);
        if (k < 2) add(Op::NOT, a, -1);
        else if (k == 2) add(pick(2) ? Op::AND : Op::XOR, a, a);                        // repeated input
        else if (k == 3) {                                                             // NOT chain into an OUTPUT
            int w = a;
            for (uint32_t c = pick(5); c > 0 && g.size() + 1 < n_gates; --c) { add(Op::NOT, w, -1); w = wires - 1; }
            add(Op::OUTPUT, w, -1);
        } else add(k < 6 ? Op::AND : k < 8 ? Op::XOR : Op::OR, a, (int)pick(wires));
    }
    add(Op::OUTPUT, wires - 1, -1);
    // file order -> level order (file order within a level); an OUTPUT sits one level after the wire it reads
    std::vector<int> glevel(g.size()), idx(g.size());
    for (size_t i = 0; i < g.size(); ++i) { glevel[i] = g[i].out >= 0 ? level[g[i].out] : level[g[i].in0] + 1; idx[i] = (int)i; }
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return glevel[x] < glevel[y]; });
    dag.n_wires = (uint32_t)wires;
    dag.level_off.push_back(0);
    for (size_t k = 0; k < idx.size(); ++k) {
        if (k && glevel[idx[k]] != glevel[idx[k - 1]]) dag.level_off.push_back((uint32_t)k);
        dag.gates.push_back(g[idx[k]]);
    }
    dag.level_off.push_back((uint32_t)g.size());
    for (const auto& x : g) if (x.op == Op::OUTPUT) dag.outputs.push_back(x.in0);
    return dag;
}

static uint64_t n_lists = 0, n_tasks_seen = 0, n_pairs_seen = 0, n_refresh_seen = 0;

// The model, from the descriptors alone: the slots a task reads and writes by its own reading of bce_gpu.h, producers by
// comparing every earlier task's outputs with them
static void against_model(TaskList L, bool allow_pairs) {
    for (uint32_t k = pick(4); k > 0 && !L.tasks.empty(); --k) {   // refreshes of existing slots into fresh ones; in1 is noise
        L.tasks.push_back(T(BCE_OP_REFRESH, pick(L.stride), pick(L.stride + 8), L.stride));
        L.prio.push_back((uint8_t)pick(kClasses));
        ++L.stride; ++n_refresh_seen;
    }
    const size_t n = L.tasks.size();
    const char* name = allow_pairs ? "random list with pairs" : "random list";
    DagBuild b;
    const DagBuildStatus st = build_dag((uint32_t)n, L.tasks.data(), L.prio.data(), allow_pairs, kClasses, b);
    if (n == 0) { REQUIRE(st.code == BCE_ERR_ARG, "an empty list has no ready task"); return; }
    REQUIRE(st.code == BCE_OK, "%s: refused with %d: %s", name, st.code, st.message.c_str());

    std::vector<V> producers(n), consumers(n);
    V dep(n), lvl(n), qcount(kClasses, 0), init_off, init_items, cons_off(1, 0), cons;
    uint32_t depth = 0, max_slot = 0;
    for (size_t i = 0; i < n; ++i) {
        const bce_gate_desc& d = L.tasks[i];
        V reads = {d.in0};
        if (d.op != BCE_OP_REFRESH) reads.push_back(d.in1);
        const uint32_t outs = (d.op >> 8) ? 2 : 1;
        n_pairs_seen += outs == 2;
        for (uint32_t s : reads) max_slot = std::max(max_slot, s);
        max_slot = std::max(max_slot, d.out + outs - 1);
        lvl[i] = 1;
        for (size_t j = 0; j < i; ++j) {
            const bce_gate_desc& e = L.tasks[j];
            const uint32_t e_outs = (e.op >> 8) ? 2 : 1;
            bool feeds = false;
            for (uint32_t s : reads) feeds = feeds || (s >= e.out && s < e.out + e_outs);
            if (!feeds) continue;
            producers[i].push_back((uint32_t)j);
            consumers[j].push_back((uint32_t)i);
            lvl[i] = std::max(lvl[i], lvl[j] + 1);
        }
        dep[i] = (uint32_t)producers[i].size();
        depth = std::max(depth, lvl[i]);
        ++qcount[L.prio[i]];
    }
    for (size_t p = 0; p < n; ++p) {
        cons.insert(cons.end(), consumers[p].begin(), consumers[p].end());
        cons_off.push_back((uint32_t)cons.size());
    }
    if (cons.empty()) cons.push_back(0);
    for (uint32_t q = 0; q < kClasses; ++q) {
        init_off.push_back((uint32_t)init_items.size());
        for (size_t i = 0; i < n; ++i) if (L.prio[i] == q && dep[i] == 0) init_items.push_back((uint32_t)i);
    }
    init_off.push_back((uint32_t)init_items.size());

    SAME(b.dep, dep, "dep");
    SAME(b.cons_off, cons_off, "cons_off");
    SAME(b.cons, cons, "cons");
    SAME(b.init_items, init_items, "init_items");
    SAME(b.init_off, init_off, "init_off");
    SAME(b.qcount, qcount, "qcount");
    REQUIRE(b.qid == L.prio, "%s: qid", name);
    REQUIRE(b.n_tasks == n && b.depth == depth && b.max_slot == max_slot, "%s: n_tasks %u, depth %u (model %u), max_slot %u (model %u)", name, b.n_tasks, b.depth, depth, b.max_slot, max_slot);
    ++n_lists; n_tasks_seen += n;
}

static void random_lists() {
    for (int t = 0; t < 200; ++t) {
        const Dag dag = random_dag(t < 8 ? 1 + t : 1 + pick(250));
        against_model(lower_tasks(build_units(dag, XorMode::Reference), dag.n_wires), false);
        against_model(lower_tasks(build_units(dag, XorMode::Shared), dag.n_wires, true), true);
        against_model(lower_tasks(build_units(dag, XorMode::Reference), dag.n_wires, true), true);   // plain lists give the same DAG
    }
    REQUIRE(n_lists > 500 && n_tasks_seen > 50000 && n_pairs_seen > 1000 && n_refresh_seen > 100, "the lists hold tasks, pairs and refreshes");
}

// ---- 3. refusals -------------------------------------------------------------------------------------------------------
static void refused(const std::vector<bce_gate_desc>& tasks, const std::vector<uint8_t>* prio, bool allow_pairs, int code, const char* text) {
    DagBuild b;
    const DagBuildStatus st = build_dag((uint32_t)tasks.size(), tasks.data(), prio ? prio->data() : nullptr, allow_pairs, kClasses, b);
    REQUIRE(st.code == code && st.message == text, "expected %d \"%s\", got %d \"%s\"", code, text, st.code, st.message.c_str());
}

static void refusals() {
    const bce_gate_desc ok = T(BCE_AND, 0, 1, 2);
    refused({ok, T(kPair, 0, 1, 3)}, nullptr, false, BCE_ERR_UNSUPPORTED,
            "bce_dag_create: task 1 is a pair descriptor (BCE_PAIR): bce_dag_create_pairs takes them, or use bce_eval_gates or a bce_plan");
    refused({T(BCE_OP_NOT, 0, 0, 1)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: task 0 is not a bootstrapped gate (op 16)");
    refused({ok, T(BCE_OP_COPY, 0, 0, 3)}, nullptr, true, BCE_ERR_ARG, "bce_dag_create: task 1 is not a bootstrapped gate (op 18)");
    for (const bool pairs : {false, true}) {   // illegal high bits are no pair: the same refusal from both creators
        refused({T(BCE_PAIR(BCE_OR, BCE_OR), 0, 1, 2)}, nullptr, pairs, BCE_ERR_ARG, "bce_dag_create: task 0 is not a bootstrapped gate (op 256)");
        refused({T(BCE_PAIR(BCE_XOR_FAST, BCE_AND), 0, 1, 2)}, nullptr, pairs, BCE_ERR_ARG, "bce_dag_create: task 0 is not a bootstrapped gate (op 516)");
        refused({T(kPair | (1u << 16), 0, 1, 2)}, nullptr, pairs, BCE_ERR_ARG, "bce_dag_create: task 0 is not a bootstrapped gate (op 66560)");
    }
    const std::vector<uint8_t> one_too_many = {0, kClasses};
    refused({ok, T(BCE_OR, 0, 1, 3)}, &one_too_many, false, BCE_ERR_ARG, "bce_dag_create: task 1 has priority class 4 (0..3)");
    refused({T(BCE_AND, 0xFFFFFFFFu, 1, 2)}, nullptr, false, BCE_ERR_POOL, "bce_dag_create: slot 4294967295 outside any pool");
    refused({T(BCE_AND, 0, 0xFFFFFFFFu, 2)}, nullptr, false, BCE_ERR_POOL, "bce_dag_create: slot 4294967295 outside any pool");
    refused({T(BCE_AND, 0, 1, 0xFFFFFFFFu)}, nullptr, false, BCE_ERR_POOL, "bce_dag_create: slot 4294967295 outside any pool");
    refused({T(kPair, 0, 1, 0xFFFFFFFEu)}, nullptr, true, BCE_ERR_POOL, "bce_dag_create: slot 4294967295 outside any pool");
    refused({T(kPair, 0, 1, 0xFFFFFFFFu)}, nullptr, true, BCE_ERR_POOL, "bce_dag_create: slot 4294967296 outside any pool");
    refused({ok, T(BCE_OR, 0, 1, 2)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: slot 2 is written by tasks 0 and 1 (SSA form required)");
    refused({T(BCE_AND, 0, 1, 3), T(kPair, 0, 1, 2)}, nullptr, true, BCE_ERR_ARG, "bce_dag_create: slot 3 is written by tasks 0 and 1 (SSA form required)");
    refused({ok, T(BCE_OR, 2, 0, 1)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: task 1 writes slot 1 that an earlier task (or itself) reads");
    refused({T(BCE_AND, 0, 1, 0)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: task 0 writes slot 0 that an earlier task (or itself) reads");
    refused({T(kPair, 0, 3, 2)}, nullptr, true, BCE_ERR_ARG, "bce_dag_create: task 0 writes slot 3 that an earlier task (or itself) reads");
    // the order of the checks: per task pair, gate, class; then the slot range; then the SSA rules in task order
    const std::vector<uint8_t> bad_class = {9};
    refused({T(kPair, 0, 1, 2)}, &bad_class, false, BCE_ERR_UNSUPPORTED,
            "bce_dag_create: task 0 is a pair descriptor (BCE_PAIR): bce_dag_create_pairs takes them, or use bce_eval_gates or a bce_plan");
    refused({T(BCE_OP_NOT, 0, 0, 1)}, &bad_class, false, BCE_ERR_ARG, "bce_dag_create: task 0 is not a bootstrapped gate (op 16)");
    refused({T(BCE_AND, 0xFFFFFFFFu, 1, 2), T(BCE_OR, 0, 1, 2)}, &one_too_many, false, BCE_ERR_ARG, "bce_dag_create: task 1 has priority class 4 (0..3)");
    refused({T(BCE_AND, 0xFFFFFFFFu, 1, 2), T(BCE_OR, 0, 1, 2)}, nullptr, false, BCE_ERR_POOL, "bce_dag_create: slot 4294967295 outside any pool");
    refused({ok, T(BCE_OR, 0, 1, 2), T(BCE_AND, 0, 1, 0)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: slot 2 is written by tasks 0 and 1 (SSA form required)");
    refused({T(BCE_AND, 2, 1, 3), ok, T(BCE_OR, 0, 1, 3)}, nullptr, false, BCE_ERR_ARG, "bce_dag_create: task 1 writes slot 2 that an earlier task (or itself) reads");
}

// ---- 4. the descriptor classifier -------------------------------------------------------------------------------------
static void classifier() {
    struct Row { uint32_t op; DescClass cls; uint32_t inputs, outputs; int pair; };
    std::vector<Row> rows = {
        {BCE_OR, DescClass::Gate, 2, 1, 0}, {BCE_AND, DescClass::Gate, 2, 1, 0}, {BCE_NOR, DescClass::Gate, 2, 1, 0}, {BCE_NAND, DescClass::Gate, 2, 1, 0},
        {BCE_XOR_FAST, DescClass::Gate, 2, 1, 0}, {BCE_XNOR_FAST, DescClass::Gate, 2, 1, 0},
        {BCE_OP_NOT, DescClass::Unary, 1, 1, 0}, {BCE_OP_REFRESH, DescClass::Refresh, 1, 1, 0}, {BCE_OP_COPY, DescClass::Unary, 1, 1, 0},
    };
    for (uint32_t op = BCE_XNOR_FAST + 1; op <= 0xFFu; ++op)
        if (op < BCE_OP_NOT || op > BCE_OP_COPY) rows.push_back({op, DescClass::None, 0, 1, 0});
    uint32_t legal = 0;
    for (uint32_t a = 0; a <= 6; ++a)
        for (uint32_t b = 0; b <= 6; ++b) {   // every pair word of two small codes: legal = two different gates of OR, AND, NOR, NAND
            const bool ok = a <= BCE_NAND && b <= BCE_NAND && a != b;
            legal += ok;
            rows.push_back(ok ? Row{BCE_PAIR(a, b), DescClass::Gate, 2, 2, 1} : Row{BCE_PAIR(a, b), DescClass::None, 0, 1, -1});
        }
    REQUIRE(legal == 12, "twelve legal pairs");
    for (const uint32_t op : {BCE_PAIR(BCE_OP_REFRESH, BCE_OR), BCE_PAIR(BCE_OR, BCE_OP_NOT), BCE_PAIR(BCE_OR, 254), kPair | (1u << 16), kPair | (1u << 31), 0x100u, 0xFFFFFFFFu})
        rows.push_back({op, DescClass::None, 0, 1, -1});
    for (const Row& r : rows) {
        const DescKind k = desc_kind(r.op);
        REQUIRE(k.cls == r.cls && k.inputs == r.inputs && k.outputs == r.outputs && pair_kind(r.op) == r.pair, "op %u: class %d, %u inputs, %u outputs, pair_kind %d", r.op, (int)k.cls, k.inputs, k.outputs, pair_kind(r.op));
        REQUIRE(k.boot() == (r.cls == DescClass::Gate || r.cls == DescClass::Refresh) && k.pair() == (r.pair > 0), "op %u: boot / pair", r.op);
    }
    struct Top { uint32_t op, in0, in1, out; uint64_t top; };
    const Top tops[] = {
        {BCE_AND, 5, 9, 3, 9}, {BCE_AND, 9, 5, 3, 9}, {BCE_XNOR_FAST, 1, 2, 7, 7},
        {BCE_OP_REFRESH, 5, 9, 3, 5}, {BCE_OP_REFRESH, 1, 9, 3, 3}, {BCE_OP_NOT, 5, 9, 3, 5}, {BCE_OP_COPY, 1, 0xFFFFFFFFu, 3, 3},
        {kPair, 1, 2, 7, 8}, {kPair, 1, 8, 7, 8}, {kPair, 9, 2, 7, 9}, {kPair, 1, 2, 0xFFFFFFFFu, 0x100000000ull},
        {BCE_AND, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFull},
    };
    for (const Top& t : tops) {
        const uint64_t got = top_slot(T(t.op, t.in0, t.in1, t.out), desc_kind(t.op));
        REQUIRE(got == t.top, "top slot of op %u (%u, %u -> %u) is %llu, expected %llu", t.op, t.in0, t.in1, t.out, (unsigned long long)got, (unsigned long long)t.top);
    }
}

int main() {
    classifier();
    hand_written();
    refusals();
    random_lists();
    std::printf("dag build selftest ok: %llu random lists, %llu tasks, %llu of them pairs, %llu refreshes\n", (unsigned long long)n_lists,
                (unsigned long long)n_tasks_seen, (unsigned long long)n_pairs_seen, (unsigned long long)n_refresh_seen);
    return 0;
}
