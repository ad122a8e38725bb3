// dag_verify_selftest.cpp -- the check list of verify mode on the dataflow schedule (sched::task_checks), on its own: no
// netlist reader, no engine, no GPU.  Random gate DAGs (NOT chains, `a op a` gates, NOTs into OUTPUTs), XORs lowered as
// the reference builds them and as XOR_FAST, and for every task list
//   * task_checks names every gate-output register (AND, OR, the final OR of a lowered XOR, XOR_FAST) exactly once, with
//     the task that writes it and the gate that owns it, and never an XOR temporary;
//   * the (register, gate) pairs are those of check_lists on the step plan lowered from the same units;
//   * evaluated in plaintext in RANDOM dependency-respecting orders (the device runs ready tasks in any order) with one
//     input bit flipped and a check + repair at every task's completion -- before anything that reads its output runs --
//     the failing checks and the final value of every register equal those of the step-by-step simulation.
// Compile with schedule.cpp only:  c++ -std=c++17 dag_verify_selftest.cpp ../../<package>/csrc/schedule.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/schedule.hpp"

using namespace bce::sched;

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static std::mt19937 rng(20251018u);
static uint32_t pick(uint32_t n) { return rng() % n; }

struct Net { Dag dag; uint32_t n_inputs; };

static Net random_dag(uint32_t n_gates) {
    Net N;
    N.n_inputs = 1 + pick(6);
    std::vector<DagGate> g;
    std::vector<int> level(N.n_inputs, 0);   // per wire
    int wires = (int)N.n_inputs;
    auto add = [&](Op op, int a, int b) {
        const bool out = op != Op::OUTPUT;
        g.push_back({op, a, b, out ? wires : -1});
        if (out) { level.push_back(1 + std::max(level[a], b >= 0 ? level[b] : 0)); ++wires; }
    };
    while (g.size() < n_gates) {
        const uint32_t k = pick(10);
        const int a = (int)pick(wires);
        if (k < 2) add(Op::NOT, a, -1);
        else if (k == 2) add(pick(2) ? Op::AND : Op::XOR, a, a);
        else if (k == 3) {
            int w = a;
            for (uint32_t c = pick(4); c > 0 && g.size() + 1 < n_gates; --c) { add(Op::NOT, w, -1); w = wires - 1; }
            add(Op::OUTPUT, w, -1);
        } else add(k < 6 ? Op::AND : k < 8 ? Op::XOR : Op::OR, a, (int)pick(wires));
    }
    add(Op::OUTPUT, wires - 1, -1);
    std::vector<int> glevel(g.size()), idx(g.size());
    for (size_t i = 0; i < g.size(); ++i) { glevel[i] = g[i].out >= 0 ? level[g[i].out] : level[g[i].in0] + 1; idx[i] = (int)i; }
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return glevel[x] < glevel[y]; });
    N.dag.n_wires = (uint32_t)wires;
    N.dag.level_off.push_back(0);
    for (size_t k = 0; k < idx.size(); ++k) {
        if (k && glevel[idx[k]] != glevel[idx[k - 1]]) N.dag.level_off.push_back((uint32_t)k);
        N.dag.gates.push_back(g[idx[k]]);
    }
    N.dag.level_off.push_back((uint32_t)g.size());
    for (const auto& x : g) if (x.op == Op::OUTPUT) N.dag.outputs.push_back(x.in0);
    return N;
}

static std::vector<uint8_t> evaluate(const Net& N, const std::vector<uint8_t>& in) {
    std::vector<uint8_t> v(N.dag.n_wires, 0);
    std::copy(in.begin(), in.end(), v.begin());
    for (const auto& g : N.dag.gates) switch (g.op) {
        case Op::NOT: v[g.out] = !v[g.in0]; break;
        case Op::AND: v[g.out] = v[g.in0] & v[g.in1]; break;
        case Op::OR: v[g.out] = v[g.in0] | v[g.in1]; break;
        case Op::XOR: v[g.out] = v[g.in0] ^ v[g.in1]; break;
        default: break;
    }
    return v;
}

static uint8_t run(const bce_gate_desc& d, const std::vector<uint8_t>& val) {
    REQUIRE(d.in0 < val.size() && d.in1 < val.size() && d.out < val.size(), "slot outside the stride");
    const uint8_t a = val[d.in0] ^ (uint8_t)d.neg0, b = val[d.in1] ^ (uint8_t)d.neg1;
    switch (d.op) {
        case BCE_AND: return a & b;
        case BCE_OR: return a | b;
        case BCE_XOR_FAST: return a ^ b;
        case BCE_XNOR_FAST: return !(a ^ b);
        default: REQUIRE(false, "unexpected op %u", d.op);
    }
    return 0;
}

static uint64_t n_lists = 0, n_checks = 0, n_orders = 0, n_repairs = 0;

static void one_net(const Net& N, bool xor_fast) {
    const Dag& dag = N.dag;
    const uint32_t W = dag.n_wires;
    Units U = build_units(dag, xor_fast);
    place_asap(U);
    const StepPlan P = lower_steps(U, dag, 0, 1, 1);
    const CheckLists C = check_lists(P, dag);
    const TaskList T = lower_tasks(U, W);
    const TaskChecks TC = task_checks(T, U, dag);
    REQUIRE(TC.tasks.size() == TC.wires.size() && TC.tasks.size() == TC.gates.size(), "three entries per check");

    // every gate-output register exactly once, with its task and its gate; no temporary
    std::vector<uint32_t> listed(W, 0), is_gate_out(W, 0);
    uint64_t gate_outs = 0;
    for (const auto& g : dag.gates) if (g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) { is_gate_out[g.out] = 1; ++gate_outs; }
    std::vector<int32_t> check_of_task(T.tasks.size(), -1);
    for (size_t i = 0; i < TC.tasks.size(); ++i) {
        const uint32_t t = TC.tasks[i], w = TC.wires[i], gi = TC.gates[i];
        REQUIRE(t < T.tasks.size(), "check %zu names task %u of %zu", i, t, T.tasks.size());
        REQUIRE(check_of_task[t] < 0, "task %u is listed twice", t);
        check_of_task[t] = (int32_t)i;
        REQUIRE(T.tasks[t].out == w, "check %zu: task %u writes slot %u, listed register %u", i, t, T.tasks[t].out, w);
        REQUIRE(w < W, "check %zu lists slot %u, an XOR temporary (registers end at %u)", i, w, W);
        REQUIRE(is_gate_out[w], "check %zu lists register %u, which no AND / OR / XOR drives", i, w);
        REQUIRE(gi < dag.gates.size() && dag.gates[gi].out == (int)w, "owner of register %u", w);
        const Op op = dag.gates[gi].op;
        REQUIRE(op == Op::AND || op == Op::OR || op == Op::XOR, "owner of register %u is not a bootstrapped gate", w);
        if (op == Op::XOR) REQUIRE(xor_fast ? (T.tasks[t].op == BCE_XOR_FAST || T.tasks[t].op == BCE_XNOR_FAST) : T.tasks[t].op == BCE_OR, "an XOR's register is written by op %u", T.tasks[t].op);
        ++listed[w];
    }
    for (uint32_t w = 0; w < W; ++w) REQUIRE(listed[w] == is_gate_out[w], "register %u is listed %u times", w, listed[w]);
    REQUIRE(TC.tasks.size() == gate_outs, "%zu checks for %llu gates", TC.tasks.size(), (unsigned long long)gate_outs);
    for (size_t t = 0; t < T.tasks.size(); ++t) if (check_of_task[t] < 0) REQUIRE(T.tasks[t].out >= W, "task %zu writes register %u unchecked", t, T.tasks[t].out);
    n_checks += TC.tasks.size();

    // the same (register, gate) pairs as the step plan's lists
    std::vector<std::pair<uint32_t, uint32_t>> a, b;
    for (size_t i = 0; i < TC.wires.size(); ++i) a.push_back({TC.wires[i], TC.gates[i]});
    for (size_t s = 0; s < C.wires.size(); ++s) for (size_t k = 0; k < C.wires[s].size(); ++k) b.push_back({C.wires[s][k], C.gates[s][k]});
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    REQUIRE(a == b, "task_checks and check_lists name different (register, gate) pairs");

    // one input flipped; the step-by-step simulation with repair after every step
    std::vector<uint8_t> in(N.n_inputs);
    for (auto& x : in) x = (uint8_t)pick(2);
    const std::vector<uint8_t> want = evaluate(N, in);
    const uint32_t flip = pick(N.n_inputs);
    std::vector<uint8_t> bad_steps(W, 0), val_steps(P.stride, 0);
    std::copy(in.begin(), in.end(), val_steps.begin());
    val_steps[flip] ^= 1;
    for (size_t s = 0; s < P.steps.size(); ++s) {
        std::vector<uint8_t> out;
        for (const auto& d : P.steps[s]) out.push_back(run(d, val_steps));
        for (size_t k = 0; k < P.steps[s].size(); ++k) val_steps[P.steps[s][k].out] = out[k];
        for (uint32_t w : C.wires[s]) { if (val_steps[w] != want[w]) { bad_steps[w] = 1; ++n_repairs; } val_steps[w] = want[w]; }
    }

    // producers of every task (SSA: one writer per slot), then random dependency-respecting orders
    std::vector<int32_t> writer(T.stride, -1);
    for (size_t t = 0; t < T.tasks.size(); ++t) {
        REQUIRE(T.tasks[t].out < T.stride && writer[T.tasks[t].out] < 0, "slot %u is written twice", T.tasks[t].out);
        writer[T.tasks[t].out] = (int32_t)t;
    }
    std::vector<std::vector<uint32_t>> cons(T.tasks.size());
    std::vector<uint32_t> dep0(T.tasks.size(), 0);
    for (size_t t = 0; t < T.tasks.size(); ++t) {
        const int32_t p0 = writer[T.tasks[t].in0], p1 = writer[T.tasks[t].in1];
        REQUIRE(p0 < (int32_t)t && p1 < (int32_t)t, "task %zu reads what a later task writes", t);
        if (p0 >= 0) { cons[p0].push_back((uint32_t)t); ++dep0[t]; }
        if (p1 >= 0 && p1 != p0) { cons[p1].push_back((uint32_t)t); ++dep0[t]; }
    }
    for (int order = 0; order < 3; ++order) {
        std::vector<uint8_t> val(T.stride, 0), bad(W, 0);
        std::copy(in.begin(), in.end(), val.begin());
        val[flip] ^= 1;
        std::vector<uint32_t> dep = dep0, ready;
        for (size_t t = 0; t < T.tasks.size(); ++t) if (!dep[t]) ready.push_back((uint32_t)t);
        size_t done = 0;
        while (!ready.empty()) {
            const size_t at = pick((uint32_t)ready.size());
            const uint32_t t = ready[at];
            ready[at] = ready.back();
            ready.pop_back();
            const bce_gate_desc& d = T.tasks[t];
            val[d.out] = run(d, val);
            if (check_of_task[t] >= 0) {        // check and repair at completion, before the consumers are released
                if (val[d.out] != want[d.out]) bad[d.out] = 1;
                val[d.out] = want[d.out];
            }
            for (uint32_t c : cons[t]) if (--dep[c] == 0) ready.push_back(c);
            ++done;
        }
        REQUIRE(done == T.tasks.size(), "%zu of %zu tasks ran", done, T.tasks.size());
        for (uint32_t w = 0; w < W; ++w) {
            if (!is_gate_out[w]) continue;
            REQUIRE(bad[w] == bad_steps[w], "register %u: check %s on the task list, %s on the step plan", w, bad[w] ? "fails" : "passes", bad_steps[w] ? "fails" : "passes");
            REQUIRE(val[w] == val_steps[w], "register %u ends as %u on the task list, %u on the step plan", w, val[w], val_steps[w]);
        }
        ++n_orders;
    }
    ++n_lists;
}

int main() {
    for (int rep = 0; rep < 300; ++rep) {
        const Net N = random_dag(1 + pick(rep < 250 ? 120 : 400));
        for (int xf = 0; xf < 2; ++xf) one_net(N, xf != 0);
    }
    std::printf("dag verify selftest ok: %llu task lists, %llu checks, %llu random orders, %llu simulated repairs\n",
                (unsigned long long)n_lists, (unsigned long long)n_checks, (unsigned long long)n_orders, (unsigned long long)n_repairs);
    return 0;
}
