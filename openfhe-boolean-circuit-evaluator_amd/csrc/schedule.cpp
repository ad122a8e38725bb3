// schedule.cpp -- see schedule.hpp.  Bootstrap-depth (re-levelled) schedule: SURVEY 8(f2).
#include "schedule.hpp"

#include <algorithm>
#include <queue>
#include <stdexcept>

#include "desc.hpp"

namespace bce::sched {

uint32_t gate_weight(Op op, XorMode mode) {
    return op == Op::XOR ? (mode == XorMode::Fast || mode == XorMode::Single ? 1 : mode == XorMode::Shared ? 2 : 3) : (op == Op::AND || op == Op::OR) ? 1 : 0;
}

void xor_lower(const bce_gate_desc& u, uint32_t t1, uint32_t t2, bce_gate_desc out[3]) {
    out[0] = {BCE_AND, u.in0, u.in1, t1, u.neg0, u.neg1 ^ 1u};
    out[1] = {BCE_AND, u.in0, u.in1, t2, u.neg0 ^ 1u, u.neg1};
    out[2] = {BCE_OR, t1, t2, u.out, 0, 0};
}

void xor_lower_shared(const bce_gate_desc& u, uint32_t t, bce_gate_desc out[2]) {
    out[0] = {BCE_PAIR(BCE_OR, BCE_NAND), u.in0, u.in1, t, u.neg0, u.neg1};
    out[1] = {BCE_AND, t, t + 1, u.out, 0, 0};
}

// units in topological order (NOT chains resolved into negation flags), their successors (CSR) and ALAP start steps
Units build_units(const Dag& dag, XorMode mode) {
    Units S;
    const size_t W = dag.n_wires;
    S.base.resize(W);
    S.neg.assign(W, 0);
    for (size_t w = 0; w < W; ++w) S.base[w] = (int)w;
    std::vector<uint32_t> depth(W, 0);
    std::vector<int32_t> prod(W, -1);   // base wire -> unit that produces it
    auto& units = S.units;
    units.reserve(dag.gates.size());
    for (const DagGate& g : dag.gates) {   // level order: bases are resolved before they are read
        if (g.op == Op::NOT) {
            S.base[g.out] = S.base[g.in0];
            S.neg[g.out] = S.neg[g.in0] ^ 1;
            depth[g.out] = depth[g.in0];
        } else if (g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) {
            const uint32_t b0 = (uint32_t)S.base[g.in0], b1 = (uint32_t)S.base[g.in1];
            const uint32_t n0 = S.neg[g.in0], n1 = S.neg[g.in1];
            const uint32_t d = 1 + std::max(depth[g.in0], depth[g.in1]);
            Unit u{d, d, 1, 0, {0, b0, b1, (uint32_t)g.out, n0, n1}, prod[b0], prod[b1]};
            if (g.op != Op::XOR) {
                u.d.op = (uint32_t)(g.op == Op::AND ? BCE_AND : BCE_OR);
            } else if (mode == XorMode::Fast) {
                // XOR_FAST of negated inputs: NOT a XOR NOT b = a XOR b; one negation flips the result
                u.d.op = (uint32_t)((n0 ^ n1) ? BCE_XNOR_FAST : BCE_XOR_FAST);
                u.d.neg0 = u.d.neg1 = 0;
            } else if (mode == XorMode::Single) {
                u.d.op = BCE_XOR;   // of the inputs as negated: the flags stay, as for AND
            } else {
                u.lat = 2;
                u.shared = mode == XorMode::Shared;
            }
            depth[g.out] = d + u.lat - 1;
            prod[g.out] = (int32_t)units.size();
            units.push_back(u);
        }
    }
    for (const auto& u : units) S.depth = std::max(S.depth, u.asap + u.lat - 1);
    const size_t U = units.size();
    S.soff.assign(U + 1, 0);
    for (const auto& u : units) { if (u.p0 >= 0) ++S.soff[u.p0 + 1]; if (u.p1 >= 0 && u.p1 != u.p0) ++S.soff[u.p1 + 1]; }
    for (size_t i = 0; i < U; ++i) S.soff[i + 1] += S.soff[i];
    S.succ.resize(S.soff[U]);
    std::vector<uint32_t> fill(S.soff.begin(), S.soff.end() - 1);
    for (size_t i = 0; i < U; ++i) {
        const Unit& u = units[i];
        if (u.p0 >= 0) S.succ[fill[u.p0]++] = (uint32_t)i;
        if (u.p1 >= 0 && u.p1 != u.p0) S.succ[fill[u.p1]++] = (uint32_t)i;
    }
    S.alap.resize(U);
    for (size_t i = U; i-- > 0;) {
        uint32_t a = S.depth - units[i].lat + 1;
        for (uint32_t k = S.soff[i]; k < S.soff[i + 1]; ++k) a = std::min(a, S.alap[S.succ[k]] - units[i].lat);
        S.alap[i] = a;
    }
    return S;
}

// List scheduling, least slack first.  Units that must run now (ALAP step reached) always do, so the depth stays D; which
// step a gate runs in does not change its ciphertext.
void place_by_slack(Units& S, uint64_t K, uint32_t lone, uint32_t full) {
    auto& units = S.units;
    const size_t U = units.size();
    const uint32_t D = S.depth;
    const auto &soff = S.soff, &succ = S.succ, &alap = S.alap;
    using Key = std::pair<uint32_t, uint32_t>;   // (ALAP step, unit)
    std::priority_queue<Key, std::vector<Key>, std::greater<Key>> ready;
    std::vector<std::vector<uint32_t>> later(D + 2);   // units that become ready at a step
    std::vector<uint32_t> waiting(U), ready_at(U, 1);
    for (size_t i = 0; i < U; ++i) {
        const Unit& u = units[i];
        waiting[i] = (u.p0 >= 0) + (u.p1 >= 0 && u.p1 != u.p0);
        if (!waiting[i]) ready.push({alap[i], (uint32_t)i});
    }
    std::vector<uint32_t> ors_due(D + 2, 0);   // ORs (shared mode: ANDs) of the XORs started one step earlier
    std::vector<uint32_t> chosen;
    for (uint32_t s = 1; s <= D; ++s) {
        for (uint32_t i : later[s]) ready.push({alap[i], i});
        chosen.clear();
        uint64_t cnt = ors_due[s];
        while (!ready.empty() && ready.top().first <= s) {   // no slack left
            const uint32_t i = ready.top().second; ready.pop();
            chosen.push_back(i); cnt += units[i].weight();
        }
        const uint64_t n = cnt * K;
        const uint64_t cap = (n <= lone ? lone : (n + full - 1) / full * full) / K;
        while (!ready.empty()) {
            const uint32_t i = ready.top().second;
            const uint64_t w = units[i].weight();
            if (cnt + w > cap) break;
            // an XOR started in the last step would put its OR beyond D only if its ALAP allowed it: it does not
            ready.pop(); chosen.push_back(i); cnt += w;
        }
        for (uint32_t i : chosen) {
            Unit& u = units[i];
            u.start = s;
            if (u.lat == 2) ++ors_due[s + 1];
            for (uint32_t k = soff[i]; k < soff[i + 1]; ++k) {
                const uint32_t q = succ[k];
                ready_at[q] = std::max(ready_at[q], s + u.lat);
                if (--waiting[q] == 0) later[ready_at[q]].push_back(q);
            }
        }
    }
    if (!ready.empty()) throw std::logic_error("buildRelevelPlan: units left unscheduled");
}

// One split of every step's units over the ranks by bootstrap weight (an XOR's three bootstraps stay on one rank: its
// temporaries are local), on top of the ORs each rank carries over from the previous step.
static void split_steps(std::vector<Unit>& units, const std::vector<std::vector<uint32_t>>& by_step, uint32_t world, bool locality) {
    std::vector<uint64_t> carried(world, 0), next_carried(world, 0);
    for (size_t st = 1; st < by_step.size(); ++st) {
        uint64_t total = 0;
        for (uint32_t r = 0; r < world; ++r) total += carried[r];
        for (uint32_t i : by_step[st]) total += units[i].weight();
        std::fill(next_carried.begin(), next_carried.end(), 0);
        if (!locality) {
            // contiguous split in netlist order: rank r ends where the running load (carried ORs of ranks <= r + the units
            // given out so far) reaches (r + 1) / world of the step's total (midpoint rule: within one unit of the fair share)
            uint32_t r = 0;
            uint64_t cum = carried[0];
            for (uint32_t i : by_step[st]) {
                const uint64_t w = units[i].weight();
                while (r + 1 < world && (2 * cum + w) * world > 2 * (uint64_t)(r + 1) * total) { ++r; cum += carried[r]; }
                units[i].owner = (uint8_t)r;
                cum += w;
                if (units[i].lat == 2) ++next_carried[r];
            }
            carried.swap(next_carried);
            continue;
        }
        // locality first ("schedule a gate on the GPU that produced most of its inputs"), balance as the
        // constraint: every rank may take up to its fair share of the step's bootstraps (rounded up, + one unit so that
        // an XOR's pair never has to split).  Units whose two producers sit on one rank choose first, then those with
        // one producing rank, then the free ones fill the least loaded ranks.
        const uint64_t share = (total + world - 1) / world + 1;
        std::vector<uint64_t> load(carried);
        std::vector<uint32_t> rest;
        auto place = [&](uint32_t i, uint32_t r) {
            units[i].owner = (uint8_t)r;
            load[r] += units[i].weight();
            if (units[i].lat == 2) ++next_carried[r];
        };
        auto owner_of = [&](int32_t p) -> int { return p >= 0 ? (int)units[p].owner : -1; };
        for (int pass = 0; pass < 2; ++pass)
            for (uint32_t i : by_step[st]) {
                const uint64_t w = units[i].weight();
                const int a = owner_of(units[i].p0), b = owner_of(units[i].p1);
                const bool both = a >= 0 && a == b;
                if (pass == 0) {
                    if (both && load[a] + w <= share) place(i, (uint32_t)a);
                    else if (!both) continue;
                    else rest.push_back(i);
                } else if (!both) {
                    // one producing rank, or two different ones: the lighter of them if it has room
                    int c = -1;
                    if (a >= 0 && load[a] + w <= share) c = a;
                    if (b >= 0 && load[b] + w <= share && (c < 0 || load[b] < load[c])) c = b;
                    if (c >= 0) place(i, (uint32_t)c); else rest.push_back(i);
                }
            }
        std::sort(rest.begin(), rest.end());   // netlist order
        for (uint32_t i : rest) {
            uint32_t r = 0;
            for (uint32_t k = 1; k < world; ++k) if (load[k] < load[r]) r = k;
            place(i, r);
        }
        carried.swap(next_carried);
    }
}

std::vector<uint8_t> crossing(const Units& S) {
    std::vector<uint8_t> x(S.units.size(), 0);
    for (const Unit& u : S.units) {
        if (u.p0 >= 0 && S.units[u.p0].owner != u.owner) x[u.p0] = 1;
        if (u.p1 >= 0 && S.units[u.p1].owner != u.owner) x[u.p1] = 1;
    }
    return x;
}

// Deterministic: every rank computes the same owners.
void assign_owners(Units& S, uint32_t world, bool locality) {
    std::vector<std::vector<uint32_t>> by_step(S.depth + 1);
    for (size_t i = 0; i < S.units.size(); ++i) by_step[S.units[i].start].push_back((uint32_t)i);
    split_steps(S.units, by_step, world, false);
    if (!locality) return;
    // keep whichever split publishes less: netlist order already is a locality order for some circuits (sha256 on two
    // ranks), input-following placement wins on others (AES-expanded on eight: 21.0 k -> 11.9 k crossing outputs)
    auto published = [&] { const auto x = crossing(S); return std::count(x.begin(), x.end(), 1); };
    const auto contiguous = published();
    split_steps(S.units, by_step, world, true);
    if (published() > contiguous) split_steps(S.units, by_step, world, false);
}

StepPlan lower_steps(const Units& S, const Dag& dag, uint32_t rank, uint32_t world, uint64_t K) {
    StepPlan P;
    const uint32_t D = S.depth, W = dag.n_wires;
    const bool sharded = world > 1;
    if (sharded) {
        // publications: an output crosses when a consumer unit sits on another rank, or when an OUTPUT gate reads it (every
        // rank decrypts every output, as in the gate-level plan); it is published after the step that produces it
        std::vector<uint8_t> feeds_output(W, 0);
        for (int w : dag.outputs) feeds_output[S.base[w]] = 1;
        const std::vector<uint8_t> cross = crossing(S);
        P.publish.assign(D, std::vector<std::vector<int>>(world));
        for (size_t i = 0; i < S.units.size(); ++i) {
            const Unit& u = S.units[i];
            if (cross[i] || feeds_output[u.d.out]) P.publish[u.start + u.lat - 2][u.owner].push_back((int)u.d.out);
        }
    }
    // temporaries of the XORs: two parity banks (a step's ANDs write one bank while the previous step's ORs read the other);
    // the slot stride must be the same on every rank: the banks are sized for the fullest step of ANY rank
    std::vector<uint32_t> xor_at((size_t)(D + 2) * world, 0);
    uint32_t max_x = 0;
    for (const auto& u : S.units) if (u.lat == 2) max_x = std::max(max_x, ++xor_at[(size_t)u.start * world + (sharded ? u.owner : 0)]);
    P.stride = W + 4 * max_x;
    P.K = (uint32_t)K;
    P.steps.assign(D, {});
    xor_at.assign(D + 2, 0);
    for (const auto& u : S.units) {
        if (sharded && u.owner != rank) continue;
        if (u.lat == 1) { P.steps[u.start - 1].push_back(u.d); continue; }
        const uint32_t idx = xor_at[u.start]++, t = W + (u.start & 1) * 2 * max_x + 2 * idx;
        bce_gate_desc x[3];
        if (u.shared) xor_lower_shared(u.d, t, x);
        else xor_lower(u.d, t, t + 1, x);
        const int first = u.shared ? 1 : 2;   // descriptors of the start step; the last one runs one step later
        P.steps[u.start - 1].insert(P.steps[u.start - 1].end(), x, x + first);
        P.steps[u.start].push_back(x[first]);
    }
    // NOT wires consumed by OUTPUT gates need a real ciphertext (decrypt must see EvalNOT's output); double negation: a copy
    std::vector<uint8_t> done_not(W, 0);
    for (int w : dag.outputs) {
        if (S.base[w] == w || done_not[w]) continue;
        done_not[w] = 1;
        const uint32_t b = (uint32_t)S.base[w];
        P.output_nots.push_back({(uint32_t)(S.neg[w] ? BCE_OP_NOT : BCE_OP_COPY), b, b, (uint32_t)w, 0, 0});
    }
    return P;
}

// Tasks = the units in topological order.  Priority class of a task = slack of its unit (ALAP step - ASAP step) with the
// bounds 0, 1, 2 (0,2,8 and 1,4,16 are 2-3 % slower on AES at K = 4 / 8): the device pulls the critical path first.
// A shared unit (pairs = true) is two tasks: the pair into the XOR's own two adjacent temporaries, then the AND of the two.
TaskList lower_tasks(const Units& S, uint32_t n_wires, bool pairs) {
    TaskList T;
    uint32_t nx = 0;
    for (size_t i = 0; i < S.units.size(); ++i) {
        const Unit& u = S.units[i];
        const uint32_t slack = S.alap[i] - u.asap;
        const uint8_t pc = slack == 0 ? 0 : slack <= 1 ? 1 : slack <= 2 ? 2 : 3;
        if (u.lat == 1) { T.tasks.push_back(u.d); T.prio.push_back(pc); continue; }
        if (u.shared && !pairs) throw std::logic_error("lower_tasks: shared XORs need the task list with pairs (bce_dag_create_pairs)");
        bce_gate_desc x[3];
        const uint32_t n = u.shared ? 2 : 3;
        if (u.shared) xor_lower_shared(u.d, n_wires + 2 * nx, x);
        else xor_lower(u.d, n_wires + 2 * nx, n_wires + 2 * nx + 1, x);
        ++nx;
        T.tasks.insert(T.tasks.end(), x, x + n);
        T.prio.insert(T.prio.end(), n, pc);
    }
    T.stride = n_wires + 2 * nx;
    return T;
}

bool check(const StepPlan& P, const Dag& dag, uint32_t rank, uint32_t world, std::string* why) {
    const size_t W = dag.n_wires;
    std::vector<int32_t> written(P.stride, -1);   // step that wrote a slot; inputs and constants: step -1 = "before"
    std::vector<uint8_t> is_out(W, 0);
    for (const auto& g : dag.gates) if ((g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) && g.out >= 0) is_out[g.out] = 1;
    auto fail = [&](const std::string& m) { if (why) *why = m; return false; };
    for (size_t s = 0; s < P.steps.size(); ++s) {
        for (const auto& d : P.steps[s])
            for (uint32_t in : {d.in0, d.in1}) {
                if (in >= P.stride) return fail("input slot outside the stride");
                if (in < W) {
                    if (is_out[in] && (written[in] < 0 || written[in] >= (int32_t)s)) return fail("step " + std::to_string(s) + " reads register " + std::to_string(in) + " before it is written");
                } else if (written[in] != (int32_t)s - 1) {
                    return fail("step " + std::to_string(s) + " reads an XOR temporary that was not written in the previous step");
                }
            }
        for (const auto& d : P.steps[s]) {
            const uint32_t outs = desc_kind(d.op).outputs;   // a pair writes out and out + 1, both temporaries
            if (outs == 2 && d.out < W) return fail("a pair writes a netlist register");
            for (uint32_t o = d.out; o < d.out + outs; ++o) {
                if (o >= P.stride) return fail("output slot outside the stride");
                if (o < W && written[o] >= 0) return fail("register written twice");
                if (written[o] == (int32_t)s) return fail("slot written twice in one step");
                written[o] = (int32_t)s;
            }
        }
        // gate sharding: what the other ranks publish after this step arrives before the next one
        if (s < P.publish.size())
            for (uint32_t r = 0; r < world; ++r) {
                if (r == rank) {
                    for (int w : P.publish[s][r]) if (written[w] != (int32_t)s) return fail("publishes register " + std::to_string(w) + " in a step that did not write it");
                } else {
                    for (int w : P.publish[s][r]) { if (written[w] >= 0) return fail("receives a register it wrote itself"); written[w] = (int32_t)s; }
                }
            }
    }
    if (P.publish.empty())
        for (size_t w = 0; w < W; ++w) if (is_out[w] && written[w] < 0) return fail("register " + std::to_string(w) + " never written");
    return true;
}

// wire -> the bootstrapped gate that drives it, -1 for every other wire
static std::vector<int32_t> gate_of_wire(const Dag& dag) {
    std::vector<int32_t> owner(dag.n_wires, -1);
    for (size_t j = 0; j < dag.gates.size(); ++j) {
        const DagGate& g = dag.gates[j];
        if ((g.op == Op::AND || g.op == Op::OR || g.op == Op::XOR) && g.out >= 0) owner[g.out] = (int32_t)j;
    }
    return owner;
}

CheckLists check_lists(const StepPlan& P, const Dag& dag) {
    CheckLists C;
    const std::vector<int32_t> owner = gate_of_wire(dag);
    C.wires.resize(P.steps.size());
    C.gates.resize(P.steps.size());
    for (size_t s = 0; s < P.steps.size(); ++s)
        for (const bce_gate_desc& d : P.steps[s]) {
            if (d.out >= dag.n_wires) continue;   // an XOR's temporary
            if (owner[d.out] < 0) throw std::logic_error("check_lists: a step writes a register no gate drives");
            C.wires[s].push_back(d.out);
            C.gates[s].push_back((uint32_t)owner[d.out]);
        }
    return C;
}

TaskChecks task_checks(const TaskList& T, const Units& S, const Dag& dag) {
    TaskChecks C;
    const std::vector<int32_t> owner = gate_of_wire(dag);
    size_t listed = 0;
    for (size_t t = 0; t < T.tasks.size(); ++t) {
        const bce_gate_desc& d = T.tasks[t];
        if (d.out >= dag.n_wires) continue;   // an XOR's temporary
        if (owner[d.out] < 0) throw std::logic_error("task_checks: a task writes a register no gate drives");
        C.tasks.push_back((uint32_t)t);
        C.wires.push_back(d.out);
        C.gates.push_back((uint32_t)owner[d.out]);
        ++listed;
    }
    if (listed != S.units.size()) throw std::logic_error("task_checks: the task list was not lowered from these units");
    return C;
}

LevelShard shard_levels(const Dag& dag, uint32_t world, XorMode mode) {
    LevelShard L;
    const size_t Lc = dag.level_off.empty() ? 0 : dag.level_off.size() - 1;
    auto cost = [&](const DagGate& g) { return (uint64_t)4 * gate_weight(g.op, mode) + 1; };   // NOT/OUTPUT weigh 1/4 bootstrap
    L.owner.resize(Lc);
    std::vector<uint8_t> gate_owner(dag.gates.size(), 0xFF);   // 0xFF = everyone (OUTPUT)
    for (size_t l = 0; l < Lc; ++l) {
        const uint32_t lo = dag.level_off[l], hi = dag.level_off[l + 1];
        uint64_t total = 0, cum = 0;
        for (uint32_t j = lo; j < hi; ++j) total += cost(dag.gates[j]);
        L.owner[l].resize(hi - lo);
        for (uint32_t j = lo; j < hi; ++j) {
            const DagGate& g = dag.gates[j];
            uint8_t o = (uint8_t)std::min<uint64_t>(world - 1, cum * world / std::max<uint64_t>(total, 1));
            cum += cost(g);
            if (g.op == Op::OUTPUT) o = 0xFF;
            L.owner[l][j - lo] = gate_owner[j] = o;
        }
    }
    // a wire is published after its level when one of its consumers (an OUTPUT gate included) is not its producer's alone
    std::vector<int32_t> prod(dag.n_wires, -1);
    for (size_t j = 0; j < dag.gates.size(); ++j) if (dag.gates[j].out >= 0) prod[dag.gates[j].out] = (int32_t)j;
    std::vector<uint8_t> cross(dag.gates.size(), 0);
    for (size_t j = 0; j < dag.gates.size(); ++j)
        for (int w : {dag.gates[j].in0, dag.gates[j].in1})
            if (w >= 0 && prod[w] >= 0 && gate_owner[prod[w]] != gate_owner[j]) cross[prod[w]] = 1;
    L.publish.assign(Lc, std::vector<std::vector<int>>(world));
    for (size_t l = 0; l < Lc; ++l)
        for (uint32_t j = dag.level_off[l]; j < dag.level_off[l + 1]; ++j)
            if (cross[j]) L.publish[l][gate_owner[j]].push_back(dag.gates[j].out);
    return L;
}

}  // namespace bce::sched
