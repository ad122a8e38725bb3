// schedule_dataflow_shared_selftest.cpp -- the task list of the dataflow schedule in shared-XOR mode, on its own: no netlist
// reader, no engine, no GPU.  lower_tasks(units, n_wires, pairs = true) lowers a shared XOR to a BCE_PAIR(OR, NAND) task
// writing the XOR's own two adjacent temporaries and an AND of the two.  Random gate DAGs (the generator of
// schedule_xor_shared_selftest.cpp) go through build_units(Shared) -> lower_tasks -> task_checks:
//   * the list is in SSA form and topological order, a pair writes two temporaries, and a consumer of both outputs of a pair
//     has ONE producer (the dependency analysis bce_dag_create_pairs does);
//   * executed in plaintext in a random dependency-respecting order, every gate register holds the value the reference
//     lowering's list leaves there, which is the netlist's;
//   * two tasks per XOR, the stride and the priority classes of the reference list, both tasks of an XOR in one class;
//   * task_checks names the same (register, gate) pairs as for the reference list, and the task it names for an XOR is the AND;
//   * without `pairs` shared units are still refused.
// Compile with schedule.cpp only:  c++ -std=c++17 schedule_dataflow_shared_selftest.cpp ../../<package>/csrc/schedule.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/schedule.hpp"

using namespace bce::sched;

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static std::mt19937 rng(20251019u);
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

static uint8_t gate(uint32_t op, uint8_t a, uint8_t b) {
    switch (op) {
        case BCE_OR: return a | b;
        case BCE_AND: return a & b;
        case BCE_NOR: return !(a | b);
        case BCE_NAND: return !(a & b);
        default: REQUIRE(false, "unexpected gate %u", op);
    }
    return 0;
}

static uint64_t n_tasks_run = 0, n_pairs_run = 0;

// SSA form, topological order, producers as bce_dag_create_pairs derives them; then a random dependency-respecting execution.
// Returns the value of every slot (0xFF: never written).
static std::vector<uint8_t> check_and_run(const TaskList& T, const Net& N, const std::vector<uint8_t>& in) {
    const uint32_t W = N.dag.n_wires;
    const size_t n = T.tasks.size();
    REQUIRE(T.prio.size() == n && T.stride >= W, "one class per task");
    std::vector<int32_t> writer(T.stride, -1);
    std::vector<uint8_t> read_before(T.stride, 0), val(T.stride, 0xFF);
    std::vector<uint8_t> is_out(W, 0);
    for (const auto& g : N.dag.gates) if ((g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) && g.out >= 0) is_out[g.out] = 1;
    for (uint32_t w = 0; w < W; ++w) if (!is_out[w]) val[w] = w < N.n_inputs ? in[w] : 0xFE;   // 0xFE: a NOT wire, folded away
    std::vector<std::vector<uint32_t>> cons(n);
    std::vector<uint32_t> left(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const bce_gate_desc& d = T.tasks[i];
        const uint32_t outs = (d.op >> 8) ? 2 : 1;
        REQUIRE(T.prio[i] < 4, "priority class");
        REQUIRE(d.in0 < T.stride && d.in1 < T.stride && d.out + outs <= T.stride, "slot outside the stride");
        if (outs == 2) REQUIRE(d.op == BCE_PAIR(BCE_OR, BCE_NAND) && d.out >= W, "a pair writes two temporaries");
        else REQUIRE(d.op == BCE_AND || d.op == BCE_OR, "a plain task is an AND or an OR (op %u)", d.op);
        int32_t p0 = writer[d.in0], p1 = writer[d.in1];
        for (uint32_t x : {d.in0, d.in1}) {
            REQUIRE(writer[x] >= 0 || (x < W && !is_out[x] && val[x] <= 1), "task %zu reads slot %u before anything defines it", i, x);
            read_before[x] = 1;
        }
        if (p1 == p0) p1 = -1;               // both outputs of one pair, or the same slot twice: one producer
        for (uint32_t o = d.out; o < d.out + outs; ++o) {
            REQUIRE(writer[o] < 0 && !read_before[o] && (o >= W || is_out[o]), "slot %u: not in SSA form", o);
            writer[o] = (int32_t)i;
        }
        for (int32_t p : {p0, p1}) if (p >= 0) { REQUIRE((size_t)p < i, "not in topological order"); cons[p].push_back((uint32_t)i); ++left[i]; }
    }
    std::vector<uint32_t> ready;
    for (size_t i = 0; i < n; ++i) if (!left[i]) ready.push_back((uint32_t)i);
    size_t done = 0;
    while (!ready.empty()) {
        const size_t k = pick((uint32_t)ready.size());
        const uint32_t i = ready[k];
        ready[k] = ready.back(); ready.pop_back();
        const bce_gate_desc& d = T.tasks[i];
        REQUIRE(val[d.in0] <= 1 && val[d.in1] <= 1, "task %u runs before its inputs hold a value", i);
        const uint8_t a = val[d.in0] ^ (uint8_t)d.neg0, b = val[d.in1] ^ (uint8_t)d.neg1;
        val[d.out] = gate(d.op & 0xFFu, a, b);
        if (d.op >> 8) { val[d.out + 1] = gate((d.op >> 8) - 1, a, b); ++n_pairs_run; }
        ++done; ++n_tasks_run;
        for (uint32_t c : cons[i]) if (--left[c] == 0) ready.push_back(c);
    }
    REQUIRE(done == n, "a task never became ready");
    return val;
}

static std::set<std::pair<uint32_t, uint32_t>> checked(const TaskChecks& C) {
    std::set<std::pair<uint32_t, uint32_t>> s;
    for (size_t i = 0; i < C.wires.size(); ++i) s.insert({C.wires[i], C.gates[i]});
    return s;
}

int main() {
    const int n_dags = 300;
    uint64_t n_xor_total = 0;
    for (int t = 0; t < n_dags; ++t) {
        const Net N = random_dag(t < 8 ? 1 + t : 1 + pick(400));
        const uint32_t W = N.dag.n_wires;
        std::vector<uint8_t> in(N.n_inputs);
        for (auto& b : in) b = (uint8_t)pick(2);
        const std::vector<uint8_t> want = evaluate(N, in);
        uint64_t n_and_or = 0, n_xor = 0;
        for (const auto& g : N.dag.gates) { n_and_or += g.op == Op::AND || g.op == Op::OR; n_xor += g.op == Op::XOR; }
        n_xor_total += n_xor;
        const Units R = build_units(N.dag, XorMode::Reference), S = build_units(N.dag, XorMode::Shared);
        bool refused = n_xor == 0;
        try { lower_tasks(S, W); } catch (const std::logic_error&) { refused = true; }
        REQUIRE(refused, "lower_tasks without `pairs` accepted shared XORs");
        const TaskList TR = lower_tasks(R, W), TS = lower_tasks(S, W, true), TRp = lower_tasks(R, W, true);
        REQUIRE(TRp.tasks.size() == TR.tasks.size() && TRp.stride == TR.stride && TRp.prio == TR.prio, "`pairs` changes nothing for reference units");
        REQUIRE(TR.tasks.size() == n_and_or + 3 * n_xor && TS.tasks.size() == n_and_or + 2 * n_xor, "two tasks per shared XOR");
        REQUIRE(TS.stride == W + 2 * n_xor && TS.stride == TR.stride, "the stride stays n_wires + 2 per XOR");
        // unit by unit: the same class in both lists, a shared XOR = the pair into n_wires + 2 x and the AND of the two
        size_t ir = 0, is = 0;
        uint32_t nx = 0;
        for (const Unit& u : S.units) {
            if (u.lat == 1) {
                REQUIRE(TS.prio[is] == TR.prio[ir] && TS.tasks[is].out == u.d.out, "a plain unit is one task");
                ++ir; ++is;
                continue;
            }
            const bce_gate_desc &p = TS.tasks[is], &a = TS.tasks[is + 1];
            const uint32_t tmp = W + 2 * nx++;
            REQUIRE(p.op == BCE_PAIR(BCE_OR, BCE_NAND) && p.out == tmp && p.in0 == u.d.in0 && p.in1 == u.d.in1 && p.neg0 == u.d.neg0 && p.neg1 == u.d.neg1, "the pair of an XOR");
            REQUIRE(a.op == BCE_AND && a.in0 == tmp && a.in1 == tmp + 1 && a.out == u.d.out && !a.neg0 && !a.neg1, "the AND of an XOR");
            REQUIRE(TS.prio[is] == TR.prio[ir] && TS.prio[is + 1] == TR.prio[ir] && TR.prio[ir + 1] == TR.prio[ir] && TR.prio[ir + 2] == TR.prio[ir], "both tasks take the unit's class");
            ir += 3; is += 2;
        }
        REQUIRE(ir == TR.tasks.size() && is == TS.tasks.size() && nx == n_xor, "every unit accounted for");
        const std::vector<uint8_t> vr = check_and_run(TR, N, in), vs = check_and_run(TS, N, in);
        for (const Unit& u : S.units)
            REQUIRE(vs[u.d.out] == vr[u.d.out] && vs[u.d.out] == want[u.d.out], "register %u: shared list %u, reference list %u, netlist %u", u.d.out, vs[u.d.out], vr[u.d.out], want[u.d.out]);
        const TaskChecks CR = task_checks(TR, R, N.dag), CS = task_checks(TS, S, N.dag);
        REQUIRE(checked(CS) == checked(CR) && CS.tasks.size() == S.units.size(), "the checked registers depend on the XOR mode");
        for (size_t i = 0; i < CS.tasks.size(); ++i) {
            const bce_gate_desc& d = TS.tasks[CS.tasks[i]];
            REQUIRE(!(d.op >> 8) && d.out == CS.wires[i] && d.out < W, "a check names the task that writes a netlist register");
            if (N.dag.gates[CS.gates[i]].op == Op::XOR) REQUIRE(d.op == BCE_AND && d.in0 >= W && d.in1 == d.in0 + 1, "an XOR's check sits on its AND task");
        }
    }
    REQUIRE(n_xor_total > 1000 && n_pairs_run == n_xor_total, "the DAGs hold XORs");
    std::printf("schedule dataflow-shared selftest ok: %d DAGs, %llu tasks executed, %llu of them pairs\n", n_dags,
                (unsigned long long)n_tasks_run, (unsigned long long)n_pairs_run);
    return 0;
}
