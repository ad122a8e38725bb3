// verify_selftest.cpp -- the check lists of verify mode on the step schedule (sched::check_lists), on their own: no
// netlist reader, no engine, no GPU.  Random gate DAGs (NOT chains, `a op a` gates, NOTs into OUTPUTs), XORs lowered as
// the reference builds them and as XOR_FAST, ASAP and slack placement, and for every plan
//   * the per-step lists name every gate-output register (AND, OR, the final OR of a lowered XOR, XOR_FAST) exactly once,
//     in the step that writes it, with the gate that owns it, and never an XOR temporary;
//   * executing the steps in plaintext, every listed register holds, right after its step, the bit a direct evaluation
//     of the DAG gives that wire: the expected bits of the device-side check are the plaintext pass's;
//   * with one input bit flipped and every listed register REPAIRED to its expected bit after its step (what the device
//     check does with repair on), every later step reads correct registers again: a mismatch can only sit in a step
//     that reads the flipped input directly (through any NOT chain folded into the descriptor).
// Compile with schedule.cpp only:  c++ -std=c++17 verify_selftest.cpp ../../<package>/csrc/schedule.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
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

static uint64_t n_plans = 0, n_checks = 0, n_repairs = 0;

static void one_plan(const Net& N, const Units& U, bool xor_fast, uint64_t K) {
    const Dag& dag = N.dag;
    const StepPlan P = lower_steps(U, dag, 0, 1, K);
    const CheckLists C = check_lists(P, dag);
    const uint32_t W = dag.n_wires;
    REQUIRE(C.wires.size() == P.steps.size() && C.gates.size() == P.steps.size(), "one list per step");
    // every gate-output register exactly once, in the step that writes it, with its own gate; no temporary
    std::vector<uint32_t> listed(W, 0), is_gate_out(W, 0);
    uint64_t gate_outs = 0;
    for (const auto& g : dag.gates) if (g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) { is_gate_out[g.out] = 1; ++gate_outs; }
    uint64_t total = 0;
    for (size_t s = 0; s < P.steps.size(); ++s) {
        REQUIRE(C.wires[s].size() == C.gates[s].size(), "lists of step %zu", s);
        for (size_t k = 0; k < C.wires[s].size(); ++k) {
            const uint32_t w = C.wires[s][k], gi = C.gates[s][k];
            REQUIRE(w < W, "step %zu lists slot %u, an XOR temporary (registers end at %u)", s, w, W);
            REQUIRE(is_gate_out[w], "step %zu lists register %u, which no AND / OR / XOR drives", s, w);
            REQUIRE(gi < dag.gates.size() && dag.gates[gi].out == (int)w, "owner of register %u", w);
            const Op op = dag.gates[gi].op;
            REQUIRE(op == Op::AND || op == Op::OR || op == Op::XOR, "owner of register %u is not a bootstrapped gate", w);
            ++listed[w];
            uint32_t writers = 0;
            for (const auto& d : P.steps[s]) if (d.out == w) {
                ++writers;
                if (op == Op::XOR) REQUIRE(xor_fast ? (d.op == BCE_XOR_FAST || d.op == BCE_XNOR_FAST) : d.op == BCE_OR, "an XOR's register is written by op %u", d.op);
            }
            REQUIRE(writers == 1, "register %u is listed in step %zu, which writes it %u times", w, s, writers);
            ++total;
        }
    }
    for (uint32_t w = 0; w < W; ++w) REQUIRE(listed[w] == is_gate_out[w], "register %u is listed %u times", w, listed[w]);
    REQUIRE(total == gate_outs, "%llu checks for %llu gates", (unsigned long long)total, (unsigned long long)gate_outs);
    n_checks += total;

    // expected bits = the plaintext pass
    std::vector<uint8_t> in(N.n_inputs);
    for (auto& b : in) b = (uint8_t)pick(2);
    const std::vector<uint8_t> want = evaluate(N, in);
    {
        std::vector<uint8_t> val(P.stride, 0);
        std::copy(in.begin(), in.end(), val.begin());
        for (size_t s = 0; s < P.steps.size(); ++s) {
            std::vector<uint8_t> out;
            for (const auto& d : P.steps[s]) out.push_back(run(d, val));   // a step's descriptors are independent
            for (size_t k = 0; k < P.steps[s].size(); ++k) val[P.steps[s][k].out] = out[k];
            for (uint32_t w : C.wires[s]) REQUIRE(val[w] == want[w], "register %u after step %zu: %u, plaintext pass %u", w, s, val[w], want[w]);
        }
    }
    // one input flipped, every listed register repaired after its step: mismatches only where the flipped input is read
    {
        const uint32_t flip = pick(N.n_inputs);
        std::vector<uint8_t> val(P.stride, 0);
        std::copy(in.begin(), in.end(), val.begin());
        val[flip] ^= 1;
        std::vector<uint8_t> tainted(P.stride, 0);   // slots computed from the flipped input and not repaired: XOR temporaries
        tainted[flip] = 1;
        for (size_t s = 0; s < P.steps.size(); ++s) {
            std::vector<uint8_t> out, t;
            for (const auto& d : P.steps[s]) { out.push_back(run(d, val)); t.push_back(tainted[d.in0] | tainted[d.in1]); }
            for (size_t k = 0; k < P.steps[s].size(); ++k) { val[P.steps[s][k].out] = out[k]; tainted[P.steps[s][k].out] = t[k]; }
            for (uint32_t w : C.wires[s]) {
                if (val[w] != want[w]) { REQUIRE(tainted[w], "register %u is wrong after step %zu although nothing it read was", w, s); ++n_repairs; }
                val[w] = want[w];
                tainted[w] = 0;
            }
        }
        for (uint32_t w = N.n_inputs; w < W; ++w) if (is_gate_out[w]) REQUIRE(val[w] == want[w], "register %u after the repaired run", w);
    }
    ++n_plans;
}

int main() {
    for (int rep = 0; rep < 300; ++rep) {
        const Net N = random_dag(1 + pick(rep < 250 ? 120 : 400));
        for (int xf = 0; xf < 2; ++xf) {
            Units U = build_units(N.dag, xf != 0);
            place_asap(U);
            one_plan(N, U, xf != 0, 1);
            const uint64_t K = 1 + pick(4);
            place_by_slack(U, K, 4 + pick(12), 8 + pick(24));
            one_plan(N, U, xf != 0, K);
        }
    }
    std::printf("verify selftest ok: %llu plans, %llu checks, %llu simulated repairs\n", (unsigned long long)n_plans,
                (unsigned long long)n_checks, (unsigned long long)n_repairs);
    return 0;
}
