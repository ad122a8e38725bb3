// circuit.cpp -- host DAG walker (see circuit.hpp).  Behavioural contract: SURVEY.md App. F.
#include "circuit.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <queue>
#include <sstream>
#include <stdexcept>

#include "bristol.hpp"

namespace bce {

namespace {
using Clock_t = std::chrono::steady_clock;
double ms_since(Clock_t::time_point t0) { return std::chrono::duration<double, std::milli>(Clock_t::now() - t0).count(); }
bool contains(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }
const char* op_name(GateEnum op) {
    switch (op) {
        case GateEnum::INPUT: return "INPUT";
        case GateEnum::OUTPUT: return "OUTPUT";
        case GateEnum::NOT: return "NOT";
        case GateEnum::AND: return "AND";
        case GateEnum::OR: return "OR";
        case GateEnum::XOR: return "XOR";
        default: return "?";
    }
}
sched::Op sched_op(GateEnum op) {
    return op == GateEnum::NOT ? sched::Op::NOT : op == GateEnum::AND ? sched::Op::AND : op == GateEnum::OR ? sched::Op::OR
         : op == GateEnum::XOR ? sched::Op::XOR : sched::Op::OUTPUT;
}
}  // namespace

// ---- Wire -------------------------------------------------------------------------------
void Wire::updateFanoutGates(const std::string& gateToRemove) {
    auto it = std::find(fanoutGates.begin(), fanoutGates.end(), gateToRemove);
    if (it == fanoutGates.end()) {
        std::cerr << "error can't find " << gateToRemove << " in fanout of wire " << name << std::endl;
        return;
    }
    fanoutGates.erase(it);
}

// ---- Gate -------------------------------------------------------------------------------
static void gate_ck(const GateEvalParams& gep, int rc, const std::string& name) {
    if (rc != BCE_OK) throw std::runtime_error("gate " + name + ": " + bce_last_error(gep.cc));
}

// verify-and-fix (src/gate.cpp:113-120,153-160,174-181,206-213)
static void verify_fix(const GateEvalParams& gep, const char* opn, CipherText slot, unsigned expect, bool fix,
                       const std::string& name) {
    uint8_t res = 0;
    gate_ck(gep, bce_decrypt_bits(gep.cc, &slot, 1, &res), name);
    if (res != expect) {
        std::cerr << "Bad " << opn << " fixing" << std::endl;
        if (gep.fixes) ++*gep.fixes;
        if (fix) {
            uint8_t bit = (uint8_t)expect;
            uint64_t idx = gep.enc_counter ? (*gep.enc_counter)++ : 0;
            gate_ck(gep, bce_encrypt_bits(gep.cc, &bit, &slot, 1, idx, gep.encrypt_mode), name);
        }
    }
}

void Gate::Evaluate(const GateEvalParams& gep) {
    bool all_ready = true;
    for (bool r : ready) all_ready = all_ready && r;
    if (!all_ready) std::cerr << "error, executing gate " << name << " but inputs not ready!" << std::endl;
    const bool pt = gep.plaintext_flag, en = gep.encrypted_flag, vf = gep.verify_flag;
    if (en && !gep.cc) throw std::runtime_error("gate " + name + ": encrypted evaluation needs an engine");
    auto enc_dst = [&]() -> CipherText {
        if (encout.empty() || encout[0] == kNoCipherText) throw std::runtime_error("gate " + name + ": no destination slot");
        return encout[0];
    };
    switch (op) {
        case GateEnum::INPUT:
            std::cerr << "error executing input should not happen" << std::endl;
            break;
        case GateEnum::OUTPUT:
            if (pt) { plainout.resize(1); plainout[0] = plainin[0]; }
            if (en) {
                encout.resize(1);
                encout[0] = encin[0];  // copy of the handle (src/gate.cpp:90-94)
                if (vf) verify_fix(gep, "OUTPUT", encout[0], plainout[0], false, name);
            }
            break;
        case GateEnum::NOT:
            if (pt) { plainout.resize(1); plainout[0] = !plainin[0]; }
            if (en) {
                bce_gate_desc d{BCE_OP_NOT, encin[0], encin[0], enc_dst(), 0, 0};
                gate_ck(gep, bce_eval_gates(gep.cc, 1, &d), name);
                if (vf) verify_fix(gep, "NOT", encout[0], plainout[0], true, name);
            }
            break;
        case GateEnum::AND:
        case GateEnum::OR:
            if (pt) {
                plainout.resize(1);
                plainout[0] = (op == GateEnum::AND) ? (plainin[0] && plainin[1]) : (plainin[0] || plainin[1]);
            }
            if (en) {
                // The reference retries AND after a throw because OpenFHE rejects ct1 == ct2
                // (src/gate.cpp:131-152); the engine computes on values, so equal handles are legal.
                bce_gate_desc d{(uint32_t)(op == GateEnum::AND ? BCE_AND : BCE_OR), encin[0], encin[1], enc_dst(), 0, 0};
                gate_ck(gep, bce_eval_gates(gep.cc, 1, &d), name);
                if (vf) verify_fix(gep, op == GateEnum::AND ? "AND" : "OR", encout[0], plainout[0], true, name);
            }
            break;
        case GateEnum::XOR:
            if (pt) { plainout.resize(1); plainout[0] = plainin[0] ^ plainin[1]; }
            if (en && (gep.xor_fast || gep.xor_single)) {
                bce_gate_desc d{(uint32_t)(gep.xor_single ? BCE_XOR : BCE_XOR_FAST), encin[0], encin[1], enc_dst(), 0, 0};
                gate_ck(gep, bce_eval_gates(gep.cc, 1, &d), name);
                if (vf) verify_fix(gep, "XOR", encout[0], plainout[0], true, name);
            } else if (en) {
                // (a AND !b) OR (!a AND b), src/gate.cpp:198-202; the NOTs are folded into the prep
                if (tmp.size() < 2) throw std::runtime_error("gate " + name + ": XOR needs two scratch slots");
                bce_gate_desc x[3];
                sched::xor_lower({0, encin[0], encin[1], enc_dst(), 0, 0}, tmp[0], tmp[1], x);
                gate_ck(gep, bce_eval_gates(gep.cc, 2, x), name);
                gate_ck(gep, bce_eval_gates(gep.cc, 1, &x[2]), name);
                if (vf) verify_fix(gep, "XOR", encout[0], plainout[0], true, name);
            }
            break;
        case GateEnum::DFF: std::cerr << "remember to write DFF" << std::endl; break;
        case GateEnum::LUT3: std::cerr << "remember to write LUT3" << std::endl; break;
        case GateEnum::LUT4: std::cerr << "remember to write LUT4" << std::endl; break;
        default: std::cerr << "bad gate eval" << std::endl;
    }
}

// ---- Circuit ------------------------------------------------------------------------------
Circuit::Circuit(int set, int method) {
    std::cout << "Generating crypto context" << std::endl;
    if (set == BCE_TOY) {
        std::cout << "*************************\nWARNING TOY Security used\n*************************" << std::endl;
    } else if (set == BCE_STD128_OPT) {
        std::cout << "STD 128 Optimized Security used" << std::endl;
    } else {
        throw std::invalid_argument("Error Bad security");  // the reference exits here (src/circuit.cpp:75-78)
    }
    if (method == BCE_AP) std::cout << "AP used" << std::endl;
    else if (method == BCE_GINX) std::cout << "GINX used" << std::endl;
    else throw std::invalid_argument("Error Bad method");
    int rc = bce_ctx_create(set, method, 0, &cc);
    if (rc != BCE_OK) throw std::runtime_error(std::string("GenerateBinFHEContext: ") + bce_last_error(nullptr));
    owns_engine_ = true;
    std::cout << "Generating crypto keys" << std::endl;
    rc = bce_keygen(cc, nullptr);  // cc.KeyGen() + BTKeyGen (src/circuit.cpp:90-91): seed from OS entropy
    if (rc != BCE_OK) {
        std::string m = bce_last_error(cc);
        bce_ctx_destroy(cc);
        throw std::runtime_error("BTKeyGen: " + m);
    }
    std::cout << "Done" << std::endl;
}

Circuit::Circuit(bce_ctx* engine) : cc(engine) { quiet_ = true; }

Circuit::~Circuit() {
    dropDag();
    dropPlan();
    if (owns_engine_ && cc) bce_ctx_destroy(cc);
}

void Circuit::requireEngine(const char* what) const {
    if (!cc) throw std::runtime_error(std::string(what) + ": this circuit has no engine (plaintext-only); encrypted mode needs the HIP engine");
}
void Circuit::ck(int rc, const char* what) const {
    if (rc != BCE_OK) throw std::runtime_error(std::string(what) + ": " + bce_last_error(cc));
}

int Circuit::addWire(uint32_t reg) {
    auto it = wire_of_reg_.find(reg);
    if (it != wire_of_reg_.end()) return it->second;
    int id = (int)wire_names_.size();
    wire_of_reg_[reg] = id;
    wire_names_.push_back("R:" + std::to_string(reg));
    return id;
}

int Circuit::wireOf(uint32_t reg, const char* what, unsigned lineNo) const {
    auto it = wire_of_reg_.find(reg);
    if (it == wire_of_reg_.end())
        throw std::runtime_error(std::string(what) + " parse error line " + std::to_string(lineNo) + ": register R" + std::to_string(reg) + " used before it is defined");
    return it->second;
}

bool Circuit::ReadFile(const std::string& inFname) {
    if (!quiet_) std::cout << "Loading circuit description " << inFname << std::endl;
    std::ifstream in(inFname);
    if (!in) throw std::runtime_error("error opening file " + inFname);
    inputGates.clear(); constWires_.clear(); allGates.clear(); wire_names_.clear(); wire_of_reg_.clear();
    unsigned lineNo = 0, gateNo = 0, max_out = 0;
    bool any_out = false;
    std::string t;
    n_buses_ = 0; n_in_bits_.assign(2, 0); out_bus_bits_.clear();
    while (std::getline(in, t)) {
        ++lineNo;
        if (!quiet_ && lineNo % 100 == 0) std::cout << "\r loading line " << lineNo << std::flush;
        if (!t.empty() && t[0] == '#') {
            // "# output buses w1 w2 ...": written by this assembler for circuits with several output values
            if (t.rfind("# output buses", 0) == 0) {
                std::istringstream ob(t.substr(14));
                unsigned w;
                out_bus_bits_.clear();
                while (ob >> w) out_bus_bits_.push_back(w);
            }
            continue;
        }
        unsigned n1 = 0, n2 = 0, n3 = 0;
        auto two_in = [&](const char* fmt, const char* what, GateEnum op) {
            if (std::sscanf(t.c_str(), fmt, &n1, &n2, &n3) != 3) throw std::runtime_error(std::string(what) + " parse error line " + std::to_string(lineNo));
            GateRec g{op, 2, {wireOf(n2, what, lineNo), wireOf(n3, what, lineNo)}, -1, -1, std::string(what) + ":" + std::to_string(gateNo++)};
            g.out = addWire(n1);
            allGates.push_back(g);
        };
        // dispatch order of the reference reader (src/circuit.cpp:144,171,199,223,246,270,292)
        if (contains(t, "CONST")) {
            // extension of the text format (Bristol Fashion EQ): a register holding a public constant
            if (std::sscanf(t.c_str(), "R%u = CONST(%u)", &n1, &n2) != 2 || n2 > 1)
                throw std::runtime_error("CONST parse error line " + std::to_string(lineNo));
            constWires_.push_back({addWire(n1), n2});
        } else if (contains(t, "LOAD")) {
            if (std::sscanf(t.c_str(), "R%u = LOAD(In%u, %u)", &n1, &n2, &n3) != 3 || n2 < 1 || n2 > 64)
                throw std::runtime_error("LOAD parse error line " + std::to_string(lineNo));
            LoadRec l{n2 - 1, n3, addWire(n1), "INPUT:" + std::to_string(gateNo++)};
            n_buses_ = std::max(n_buses_, n2);
            if (n_in_bits_.size() < n2) n_in_bits_.resize(n2, 0);
            n_in_bits_[n2 - 1] = std::max(n_in_bits_[n2 - 1], n3 + 1);
            inputGates.push_back(l);
        } else if (contains(t, "STORE")) {
            if (std::sscanf(t.c_str(), "Out%u = STORE(R%u)", &n1, &n2) != 2) throw std::runtime_error("STORE parse error line " + std::to_string(lineNo));
            GateRec g{GateEnum::OUTPUT, 1, {wireOf(n2, "STORE", lineNo), -1}, -1, (int)n1, "OUTPUT:" + std::to_string(gateNo++)};
            allGates.push_back(g);
            max_out = std::max(max_out, n1);
            any_out = true;
        } else if (contains(t, "NOT")) {
            if (std::sscanf(t.c_str(), "R%u = NOT(R%u)", &n1, &n2) != 2) throw std::runtime_error("NOT parse error line " + std::to_string(lineNo));
            GateRec g{GateEnum::NOT, 1, {wireOf(n2, "NOT", lineNo), -1}, -1, -1, "NOT:" + std::to_string(gateNo++)};
            g.out = addWire(n1);
            allGates.push_back(g);
        } else if (contains(t, "AND")) {
            two_in("R%u = AND(R%u, R%u)", "AND", GateEnum::AND);
        } else if (contains(t, " OR")) {
            two_in("R%u = OR(R%u, R%u)", "OR", GateEnum::OR);
        } else if (contains(t, "XOR")) {
            two_in("R%u = XOR(R%u, R%u)", "XOR", GateEnum::XOR);
        } else if (contains(t, "BOOT")) {
            // no-op
        }
    }
    n_output_bits.assign(1, any_out ? max_out + 1 : 0);
    {
        unsigned tot = 0;
        for (unsigned w : out_bus_bits_) tot += w;
        if (out_bus_bits_.empty() || tot != n_output_bits[0]) out_bus_bits_.assign(1, n_output_bits[0]);
    }
    if (!quiet_) {
        std::cout << std::endl << "generating output nbits " << n_output_bits[0] << std::endl;
        std::cout << "generating netlist" << std::endl;
    }
    finalizeNetlist();
    if (!quiet_) std::cout << "Done" << std::endl;
    return true;
}

bool Circuit::ReadBristol(const std::string& path, bool new_flag) {
    Analysis A = analyze_bristol(path, false, new_flag, true);
    const Variable& v = A.variables;
    const Function& f = A.functions;
    inputGates.clear(); constWires_.clear(); allGates.clear(); wire_names_.clear(); wire_of_reg_.clear();
    unsigned gateNo = 0;
    // same register numbering as the assembler: inputs first (bus after bus), then one register per gate
    std::vector<int> node_wire(v.n_tot, -1);
    uint32_t reg = 0;
    {
        unsigned node = 0;
        for (size_t bus = 0; bus < v.in_bits.size(); ++bus)
            for (unsigned b = 0; b < v.in_bits[bus]; ++b, ++node) {
                node_wire[node] = addWire(reg++);
                inputGates.push_back({(unsigned)bus, b, node_wire[node], "INPUT:" + std::to_string(gateNo++)});
            }
    }
    n_in_bits_ = v.in_bits;
    while (n_in_bits_.size() > 1 && n_in_bits_.back() == 0) n_in_bits_.pop_back();   // old format: "n 0 m" = one input
    n_buses_ = (unsigned)n_in_bits_.size();
    if (n_in_bits_.size() < 2) n_in_bits_.resize(2, 0);
    out_bus_bits_ = v.out_bits;
    for (size_t i = 0; i < f.call_list.size(); ++i) {
        const std::string& op = f.call_list[i];
        GateRec g{};
        g.in[0] = g.in[1] = -1; g.out_bit = -1;
        const auto& il = f.in_list[i];
        if (op == " EQ") {
            // constant: a register that is live from the start; encrypted runs hold it as the trivial (noiseless)
            // ciphertext (0, value * q/4) -- a public constant needs no key
            const int w = addWire(reg++);
            node_wire[f.out_list[i].at(0)] = w;
            constWires_.push_back({w, il.at(0)});
            continue;
        }
        for (unsigned w : il) if (node_wire[w] < 0) throw std::runtime_error("ReadBristol: gate " + std::to_string(i) + " uses undefined wire");
        if (op == "XOR" || op == "AND") {
            if (il.size() != 2) throw std::runtime_error("ReadBristol: bad arity");
            g.op = op == "XOR" ? GateEnum::XOR : GateEnum::AND; g.nin = 2; g.in[0] = node_wire[il[0]]; g.in[1] = node_wire[il[1]];
        } else if (op == "NOT") {
            g.op = GateEnum::NOT; g.nin = 1; g.in[0] = node_wire[il.at(0)];
        } else if (op == "EQW") {
            // Bristol Fashion wire copy: no gate, the output node is an alias of the input wire
            // (the reference's assembler only emits a parse-error comment for it, src/assemble.cpp:370-373)
            node_wire[f.out_list[i].at(0)] = node_wire[il.at(0)];
            continue;
        } else {
            throw std::runtime_error("ReadBristol: unsupported op " + op + " at gate " + std::to_string(i));
        }
        g.name = std::string(op_name(g.op)) + ":" + std::to_string(gateNo++);
        g.out = addWire(reg++);
        node_wire[f.out_list[i].at(0)] = g.out;
        allGates.push_back(g);
    }
    for (unsigned o = 0; o < v.n_out1_bits; ++o) {
        int w = node_wire[v.n_tot - v.n_out1_bits + o];
        if (w < 0) throw std::runtime_error("ReadBristol: output node never driven");
        allGates.push_back(GateRec{GateEnum::OUTPUT, 1, {w, -1}, -1, (int)o, "OUTPUT:" + std::to_string(gateNo++)});
    }
    // internally ONE concatenated bus (bit indices run over all output values); getOutputs() splits it
    n_output_bits.assign(1, v.n_out1_bits);
    finalizeNetlist();
    return true;
}

// CSR fan-out + static ASAP levelisation (what _CircuitManager discovers round by round)
void Circuit::finalizeNetlist() {
    const size_t W = wire_names_.size(), G = allGates.size();
    fan_off_.assign(W + 1, 0);
    for (const auto& g : allGates) for (int k = 0; k < g.nin; ++k) ++fan_off_[g.in[k] + 1];
    for (size_t w = 0; w < W; ++w) fan_off_[w + 1] += fan_off_[w];
    fan_gate_.assign(fan_off_[W], 0);
    std::vector<uint32_t> pos(fan_off_.begin(), fan_off_.end() - 1);
    for (size_t gi = 0; gi < G; ++gi) for (int k = 0; k < allGates[gi].nin; ++k) fan_gate_[pos[allGates[gi].in[k]]++] = (uint32_t)gi;

    levels_.clear();
    std::vector<int> ready(G, 0), active;
    for (const auto& l : inputGates) active.push_back(l.wire);
    for (const auto& k : constWires_) active.push_back(k.wire);
    max_level_xor_ = 0;
    while (!active.empty()) {
        Level L;
        for (int w : active)
            for (uint32_t e = fan_off_[w]; e < fan_off_[w + 1]; ++e) {
                uint32_t gi = fan_gate_[e];
                if (++ready[gi] == allGates[gi].nin) L.gates.push_back((int)gi);
            }
        if (L.gates.empty()) break;
        std::sort(L.gates.begin(), L.gates.end());
        active.clear();
        for (int gi : L.gates) {
            if (allGates[gi].op == GateEnum::XOR) ++L.n_xor;
            if (allGates[gi].out >= 0) active.push_back(allGates[gi].out);
        }
        max_level_xor_ = std::max(max_level_xor_, L.n_xor);
        levels_.push_back(std::move(L));
    }
    base_stride_ = stride_ = (uint32_t)W + 2 * max_level_xor_;
    inputs_set_ = false;
    // the same netlist as the schedule module reads it: level order, OUTPUT wires in file order
    net_ = sched::Dag{(uint32_t)W, {}, {0}, {}};
    for (const auto& L : levels_) {
        for (int gi : L.gates) net_.gates.push_back({sched_op(allGates[gi].op), allGates[gi].in[0], allGates[gi].nin > 1 ? allGates[gi].in[1] : -1, allGates[gi].out});
        net_.level_off.push_back((uint32_t)net_.gates.size());
    }
    for (const auto& g : allGates) if (g.op == GateEnum::OUTPUT) net_.outputs.push_back(g.in[0]);
    buildUnits();
    rebuildRelevel();  // also sizes the scratch slots the re-levelled schedule needs
    buildShardPlan();
    Reset();
}

void Circuit::Reset() {
    n_input_gates = n_output_gates = n_and_gates = n_or_gates = n_xor_gates = n_not_gates = 0;
    opt_.plaintext = opt_.encrypted = opt_.verify = false;
    done = false;
    inputs_set_ = false;
    syncXorMode();   // verify is one of the things xorMode() reads
    ++epoch_;
    plain_.assign(instances_, std::vector<uint8_t>(wire_names_.size(), 0));
    circuitOut.assign(instances_, std::vector<uint8_t>(n_output_bits.empty() ? 0 : n_output_bits[0], 0));
    stats_ = bce_circuit_stats{};
}

void Circuit::Rearm() {
    if (!inputs_set_) throw std::logic_error("Rearm: SetInput has not been called");
    n_output_gates = n_and_gates = n_or_gates = n_xor_gates = n_not_gates = 0;
    done = false;
    stats_ = bce_circuit_stats{};
}

RunMode Circuit::runMode() const {
    ModeInputs m = opt_;
    m.engine = cc != nullptr;
    m.dag_supported = cc && bce_dag_supported(cc);
    m.gate_sharded = gateSharded();
    m.tasks = !tasks_.tasks.empty();
    return resolve_mode(m);
}

void Circuit::refuseWithKeys(const char* who) const {
    if (!instance_keys_.empty()) throw Unsupported(std::string(who) + " together with setInstanceKeys: per-instance key sets run the step schedule only");
}
void Circuit::keysCombinationSupported(const char* who) const {
    if (instance_keys_.empty()) return;
    const char* with = opt_.dataflow ? "setDataflow" : opt_.verify ? "setVerify" : opt_.device_verify ? "setDeviceVerify" : gateSharded() ? "gate sharding" : nullptr;
    if (with) throw Unsupported(std::string(who) + ": setInstanceKeys together with " + with + " is not supported");
}

void Circuit::setInstanceKeys(const std::vector<uint32_t>& ids) {
    if (inputs_set_) throw std::logic_error("setInstanceKeys: call it before SetInput");
    if (!ids.empty() && ids.size() != instances_) throw std::invalid_argument("setInstanceKeys: " + std::to_string(ids.size()) + " ids for " + std::to_string(instances_) + " instances");
    const std::vector<uint32_t> was = std::move(instance_keys_);
    instance_keys_ = ids;
    try {
        keysCombinationSupported("setInstanceKeys");
    } catch (...) {
        instance_keys_ = was;
        throw;
    }
    dropPlan();
}

void Circuit::setVerify(bool b) {
    if (b) refuseWithKeys("setVerify");
    setModeFlag(opt_.verify, b, "setVerify");   // one of the things xorMode() reads
    if (b) { setPlaintext(true); setEncrypted(true); }
}

void Circuit::setInstances(unsigned k) {
    if (k == 0) throw std::invalid_argument("setInstances: need at least one instance");
    if (k != instances_) instance_keys_.clear();   // one id per instance: the list of another K no longer fits
    instances_ = k;
    plain_.assign(instances_, std::vector<uint8_t>(wire_names_.size(), 0));
    circuitOut.assign(instances_, std::vector<uint8_t>(n_output_bits.empty() ? 0 : n_output_bits[0], 0));
    buildShardPlan();
    rebuildRelevel();   // the balanced schedule depends on K
}

std::pair<unsigned, unsigned> Circuit::instanceRange() const {
    const unsigned per = instances_ / world_;
    return instanceSharded() ? std::make_pair(rank_ * per, rank_ * per + per) : std::make_pair(0u, instances_);
}

void Circuit::SetInput(const Inputs& input, bool verbose) { SetInput(0, input, verbose); }

void Circuit::SetInput(unsigned inst, const Inputs& input, bool verbose) {
    if (inst >= instances_) throw std::out_of_range("SetInput: instance out of range");
    keysCombinationSupported("SetInput");
    size_t total_bits = 0;
    for (size_t k = 0; k < input.size(); ++k) {
        if (verbose) std::cout << "setting input " << k << " size " << input[k].size() << std::endl;
        total_bits += input[k].size();
    }
    if (verbose) std::cout << "set input total of " << input.size() << " inputs" << std::endl;
    const auto [lo, hi] = instanceRange();
    const bool mine = inst >= lo && inst < hi;
    std::vector<uint8_t> bits;
    std::vector<uint32_t> slots;
    n_input_gates = 0;
    for (const auto& l : inputGates) {
        if (l.bus >= input.size() || l.bit >= input[l.bus].size())
            throw std::out_of_range("SetInput: " + l.name + " reads In" + std::to_string(l.bus + 1) + " bit " + std::to_string(l.bit) + " which was not supplied");
        uint8_t v = input[l.bus][l.bit] ? 1 : 0;
        ++n_input_gates;
        plain_[inst][l.wire] = v;
        bits.push_back(v);
        slots.push_back(inst * stride_ + (uint32_t)l.wire);
    }
    for (const auto& k : constWires_) plain_[inst][k.wire] = (uint8_t)k.value;
    if (total_bits != inputGates.size())
        std::cerr << "error: total_inputs: " << total_bits << " #used: " << inputGates.size() << std::endl;
    else if (verbose)
        std::cout << "input confirmed" << std::endl;
    if (opt_.encrypted && mine) {  // encrypted mode must be on at call time (src/circuit.cpp:505-507)
        requireEngine("SetInput");
        ck(bce_pool_reserve(cc, instances_ * stride_), "SetInput(pool)");
        // stream index = (evaluation epoch, instance, input position): every rank draws the same ciphertexts
        uint64_t base = ((epoch_ & 0xFFFFFull) << 44) | ((uint64_t)inst << 24);
        if (instance_keys_.empty()) {
            ck(bce_encrypt_bits(cc, bits.data(), slots.data(), (uint32_t)slots.size(), base, encrypt_mode_), "SetInput(Encrypt)");
        } else {   // under the instance's key set; the selection is restored whatever happens
            const uint32_t was = bce_keyset_selected(cc);
            ck(bce_keyset_select(cc, instance_keys_[inst]), "SetInput(key set)");
            const int rc = bce_encrypt_bits(cc, bits.data(), slots.data(), (uint32_t)slots.size(), base, encrypt_mode_);
            const std::string msg = rc != BCE_OK ? bce_last_error(cc) : "";
            bce_keyset_select(cc, was);
            if (rc != BCE_OK) throw std::runtime_error("SetInput(Encrypt): " + msg);
        }
        if (!constWires_.empty()) {
            // public constants: trivial ciphertexts (a = 0, b = value * q/4), exact and noiseless
            uint64_t p[BCE_P_COUNT];
            ck(bce_get_params(cc, p), "SetInput(params)");
            const size_t W = (size_t)p[BCE_P_n] + 1;
            std::vector<uint64_t> cts(constWires_.size() * W, 0);
            std::vector<uint32_t> cslots;
            for (size_t k = 0; k < constWires_.size(); ++k) {
                cts[k * W + W - 1] = constWires_[k].value ? p[BCE_P_q] / 4 : 0;
                cslots.push_back(inst * stride_ + (uint32_t)constWires_[k].wire);
            }
            ck(bce_lwe_write(cc, cslots.data(), (uint32_t)cslots.size(), cts.data()), "SetInput(constants)");
        }
    }
    inputs_set_ = true;
}

// ---- sharding plan --------------------------------------------------------------------------
void Circuit::buildShardPlan() {
    shard_ = gateSharded() ? sched::shard_levels(net_, world_, xorMode()) : sched::LevelShard{};
}

uint64_t Circuit::exchangeCapacity(uint32_t world, int shard_mode, bool encrypted) const {
    uint64_t W = 4;
    if (encrypted && cc) { uint64_t p[BCE_P_COUNT]; bce_get_params(cc, p); W = 4 * (p[BCE_P_n] + 1); }
    const uint64_t nout = n_output_bits.empty() ? 0 : n_output_bits[0];
    if (world <= 1) return 0;
    if (shard_mode == 0) return std::max<uint64_t>(64, (uint64_t)(instances_ / world) * nout);
    // mode 1: widest per-rank publication over all levels (plan must be built for this world)
    uint64_t widest = 0;
    for (const auto& lv : shard_.publish) for (const auto& r : lv) widest = std::max<uint64_t>(widest, r.size());
    if (shard_.publish.empty()) for (const auto& lv : levels_) widest = std::max<uint64_t>(widest, lv.gates.size());
    // bootstrap-depth schedule under gate sharding: per-step publications (before the plan exists for this world: a step's
    // outputs are at most its descriptors; slack filling under a larger world can widen steps up to the whole circuit's width)
    for (const auto& st : steps_.publish) for (const auto& r : st) widest = std::max<uint64_t>(widest, r.size());
    if (steps_.publish.empty()) for (const auto& st : steps_.steps) widest = std::max<uint64_t>(widest, st.size());
    // (callers size their buffers with this BEFORE set_exchange and ask again afterwards: the plan for the new world may
    // publish more per step than the estimate -- dist.Exchange does)
    return std::max<uint64_t>(64, widest * instances_ * (encrypted ? W : 1));
}

void Circuit::setExchange(uint32_t rank, uint32_t world, int shard_mode, bce_allgather_fn fn, void* user, void* host_send,
                          void* host_recv, void* dev_send, void* dev_recv, uint64_t capacity) {
    if (world == 0 || rank >= world) throw std::invalid_argument("setExchange: bad rank/world");
    if (world > 1 && !fn) throw std::invalid_argument("setExchange: allgather callback missing");
    if (world > 1 && shard_mode == 0 && instances_ % world) throw std::invalid_argument("setExchange: instance sharding needs instances divisible by world");
    if (world > 250) throw std::invalid_argument("setExchange: world too large");
    if (world > 1 && shard_mode == 1) refuseWithKeys("gate sharding (setExchange)");
    rank_ = rank; world_ = world; shard_mode_ = shard_mode; xfn_ = fn; xuser_ = user;
    if (units_mode_ != xorMode()) buildUnits();   // gate sharding keeps the reference lowering
    host_send_ = host_send; host_recv_ = host_recv; dev_send_ = dev_send; dev_recv_ = dev_recv; xcap_ = capacity;
    buildShardPlan();
    rebuildRelevel();   // the number of instances this rank evaluates may have changed
}

uint64_t Circuit::planHash() const {
    uint64_t h = 0xcbf29ce484222325ull;   // FNV-1a over 64-bit words
    auto mix = [&](uint64_t v) { h = (h ^ v) * 0x100000001b3ull; };
    mix(world_); mix((uint64_t)shard_mode_); mix(stride_); mix(instances_); mix(opt_.relevel ? 1 : 0); mix((uint64_t)xorMode());
    if (opt_.dataflow_shared) mix(0x6466736872ull);   // "dfshr"; mixed only when set: the hashes without the flag are pinned (tests/golden)
    for (const auto& lv : shard_.owner) { mix(lv.size()); for (uint8_t o : lv) mix(o); }
    for (const auto& lv : shard_.publish) for (const auto& r : lv) { mix(r.size()); for (int w : r) mix((uint64_t)w); }
    for (const auto& st : steps_.publish) for (const auto& r : st) { mix(r.size()); for (int w : r) mix((uint64_t)w); }
    return h;
}

// one exchange: pub[r] = the wires rank r publishes (every rank knows every list: the plan is static)
void Circuit::exchangeWires(const std::vector<std::vector<int>>& pub) {
    if (!gateSharded()) return;
    size_t widest = 0;
    for (uint32_t r = 0; r < world_; ++r) widest = std::max(widest, pub[r].size());
    if (widest == 0) return;
    const auto& mine = pub[rank_];
    const unsigned K = instances_;
    if (opt_.plaintext) {
        const uint64_t bytes = (uint64_t)widest * K;
        if (bytes > xcap_ || !host_send_ || !host_recv_) throw std::runtime_error("exchange: host buffers too small");
        uint8_t* s = (uint8_t*)host_send_;
        std::memset(s, 0, bytes);
        for (unsigned i = 0; i < K; ++i) for (size_t k = 0; k < mine.size(); ++k) s[i * widest + k] = plain_[i][mine[k]];
        if (xfn_(xuser_, bytes, 0) != 0) throw std::runtime_error("exchange: allgather callback failed");
        const uint8_t* rcv = (const uint8_t*)host_recv_;
        for (uint32_t r = 0; r < world_; ++r) {
            if (r == rank_) continue;
            const auto& theirs = pub[r];
            for (unsigned i = 0; i < K; ++i) for (size_t k = 0; k < theirs.size(); ++k) plain_[i][theirs[k]] = rcv[(uint64_t)r * bytes + i * widest + k];
        }
        ++stats_.exchanges;
    }
    if (opt_.encrypted) {
        uint64_t p[BCE_P_COUNT];
        bce_get_params(cc, p);
        const uint64_t W = 4 * (p[BCE_P_n] + 1);
        const uint64_t bytes = (uint64_t)widest * K * W;
        if (bytes > xcap_ || !dev_send_ || !dev_recv_) throw std::runtime_error("exchange: device buffers too small");
        std::vector<uint32_t> slots;
        for (unsigned i = 0; i < K; ++i) for (size_t k = 0; k < widest; ++k) slots.push_back(i * stride_ + (uint32_t)(k < mine.size() ? mine[k] : (mine.empty() ? 0 : mine[0])));
        ck(bce_pool_gather(cc, slots.data(), (uint32_t)slots.size(), dev_send_), "exchange(gather)");
        if (rccl_) {
            // stream-ordered: pack kernel -> ncclAllGather -> scatter kernels, all on the engine's stream
            ck(bce_rccl_allgather(cc, dev_send_, dev_recv_, bytes), "exchange(RCCL all-gather)");
        } else {
            ck(bce_synchronize(cc), "exchange(sync)");
            if (xfn_(xuser_, bytes, 1) != 0) throw std::runtime_error("exchange: allgather callback failed");
        }
        for (uint32_t r = 0; r < world_; ++r) {
            if (r == rank_) continue;
            const auto& theirs = pub[r];
            if (theirs.empty()) continue;
            // rows [i][k<theirs.size()] of rank r's block
            for (unsigned i = 0; i < K; ++i) {
                slots.clear();
                for (size_t k = 0; k < theirs.size(); ++k) slots.push_back(i * stride_ + (uint32_t)theirs[k]);
                const char* src = (const char*)dev_recv_ + (uint64_t)r * bytes + (uint64_t)i * widest * W;
                ck(bce_pool_scatter(cc, slots.data(), (uint32_t)slots.size(), src), "exchange(scatter)");
            }
        }
        ++stats_.exchanges;
        stats_.exchanged_cts += (uint64_t)mine.size() * K;
    }
}

// shard_mode 0: every rank ends with the outputs of all instances
void Circuit::gatherOutputs() {
    if (!instanceSharded()) return;
    const uint64_t nout = n_output_bits[0];
    const auto [lo, hi] = instanceRange();
    const uint64_t bytes = (uint64_t)(hi - lo) * nout;
    if (bytes == 0) return;
    if (bytes > xcap_ || !host_send_ || !host_recv_) throw std::runtime_error("gatherOutputs: host buffers too small");
    uint8_t* s = (uint8_t*)host_send_;
    for (unsigned i = lo; i < hi; ++i) std::memcpy(s + (uint64_t)(i - lo) * nout, circuitOut[i].data(), nout);
    if (xfn_(xuser_, bytes, 0) != 0) throw std::runtime_error("gatherOutputs: allgather callback failed");
    const uint8_t* rcv = (const uint8_t*)host_recv_;
    const unsigned per = hi - lo;
    for (uint32_t r = 0; r < world_; ++r)
        for (unsigned k = 0; k < per; ++k) std::memcpy(circuitOut[r * per + k].data(), rcv + (uint64_t)r * bytes + (uint64_t)k * nout, nout);
    ++stats_.exchanges;
}

// ---- re-levelled (bootstrap-depth) schedule: SURVEY 8(f2), built by the schedule module (schedule.hpp) ----------------
// One bootstrap is one workgroup, so a frontier call costs a staircase in its size (one bootstrap latency up to `lone`
// bootstraps, then one round per `full` resident workgroups; bce_launch_capacity): the capacities slack filling works with.
std::pair<uint32_t, uint32_t> Circuit::launchCapacity() const {
    if (cap_lone_ && cap_full_) return {cap_lone_, cap_full_};
    uint32_t a = 0, b = 0;
    return cc && bce_launch_capacity(cc, &a, &b) == BCE_OK && a && b ? std::make_pair(a, b) : std::make_pair(256u, 512u);
}

// (re)build the bootstrap-depth schedule for the current K / capacities / ranks (place, then lower), the dataflow task list
// while that schedule is chosen, and size the per-instance slot stride for them.  The stride is part of the pool layout:
// not after SetInput.
void Circuit::rebuildRelevel() {
    dropPlan();   // the resident copies of the schedules belong to the plans they were built from
    dropDag();
    const auto [lo, hi] = instanceRange();
    const uint64_t K = std::max(1u, hi - lo);
    const uint32_t world = gateSharded() ? world_ : 1;   // gate sharding: every step's units are split over the ranks
    const bool want_tasks = opt_.dataflow && tasksExist();   // shared XORs: pair tasks, with setDataflowShared only
    if (!want_tasks || tasks_.tasks.empty()) tasks_ = want_tasks ? lowerTasks() : sched::TaskList{};   // a function of the units
    auto plan = [&](bool by_slack) {   // returns the slot stride the schedules need
        if (by_slack && !units_.units.empty()) {
            const auto [lone, full] = launchCapacity();
            sched::place_by_slack(units_, K, lone * world, full * world);   // the stairs of `world` devices working on one step
        } else {
            sched::place_asap(units_);
        }
        if (world > 1) sched::assign_owners(units_, world, shard_locality_);
        steps_ = sched::lower_steps(units_, net_, rank_, world, K);
        return std::max({base_stride_, steps_.stride, tasks_.stride});
    };
    uint32_t need = plan(balance_);
    // the inputs already sit in a pool laid out for a smaller stride: keep the layout, fall back to ASAP placement
    // (whose temporaries the stride of finalizeNetlist() always covers)
    if (inputs_set_ && need > stride_ && balance_) need = plan(false);
    if (inputs_set_ && need > stride_) throw std::logic_error("the schedule needs a larger slot stride than the pool was laid out with");
    if (!inputs_set_) stride_ = need;
}

// per-step bootstrap counts of the schedule (for one instance)
std::vector<uint32_t> Circuit::relevelStepSizes() const {
    std::vector<uint32_t> v;
    for (const auto& st : steps_.steps) v.push_back((uint32_t)st.size());
    return v;
}

std::vector<uint32_t> Circuit::relevelPublications() const {
    std::vector<uint32_t> v(steps_.steps.size(), 0);
    for (size_t s = 0; s < steps_.publish.size() && s < v.size(); ++s) v[s] = (uint32_t)steps_.publish[s][rank_].size();
    return v;
}

// the one XOR choice behind setXorFast / setXorShared / setXorSingle (circuit.hpp)
void Circuit::chooseXor(XorChoice which, bool b, bool before_input) {
    static const char* const setter[] = {"", "setXorFast", "setXorShared", "setXorSingle"};
    const std::string who = setter[(int)which];
    const XorChoice cur = opt_.xor_choice;
    if (b && cur != XorChoice::None && cur != which)
        throw std::invalid_argument(who + ": not together with " + (which == XorChoice::Single ? "setXorFast or setXorShared" : setter[(int)cur]));
    if (before_input && inputs_set_ && b != (cur == which)) throw std::logic_error(who + ": choose the XOR lowering before SetInput");
    if (b) opt_.xor_choice = which;
    else if (cur == which) opt_.xor_choice = XorChoice::None;
    if (which == XorChoice::Shared) return syncXorMode();
    buildUnits();
    buildShardPlan();
    rebuildRelevel();
}

// The two lowerings use the same temporaries (two adjacent slots per XOR): under the same placement the slot stride does
// not depend on the mode.  Placement by slack does depend on it (a shared XOR weighs 1 + 1, a reference one 2 + 1), so the
// stride of one lowering's schedule need not hold the other's: the mode is settled when the pool is laid out.
void Circuit::syncXorMode() {
    if (units_mode_ == xorMode()) return;
    buildUnits();
    rebuildRelevel();
}

void Circuit::setModeFlag(bool& flag, bool b, const char* who) {
    const bool was = flag;
    flag = b;
    if (inputs_set_ && units_mode_ != xorMode()) {
        flag = was;
        throw std::logic_error(std::string(who) + ": it would switch the XOR lowering chosen with setXorShared; call it before SetInput");
    }
    syncXorMode();
}

// the schedule's descriptors on the device (bce_plan), for the instances [lo, lo + K)
void Circuit::ensurePlan(bce_plan*& plan, unsigned lo, uint32_t K) {
    if (steps_.steps.empty() || (balance_ && steps_.K != std::max(1u, K))) rebuildRelevel();
    if (steps_.stride > stride_) throw std::logic_error("re-levelled schedule needs more scratch slots than the pool stride");
    // the schedule's descriptors live on the device from the first Clock() on (bce_plan): a step is one call without an
    // upload; with setGraph the whole schedule is one hipGraph launch
    if ((plan_ || vplan_) && (plan_lo_ != lo || plan_K_ != K || plan_stride_ != stride_)) dropPlan();
    if (!plan && K) {
        std::vector<uint32_t> sizes;
        std::vector<bce_gate_desc> all;
        for (const auto& st : steps_.steps)
            if (!st.empty()) { sizes.push_back((uint32_t)st.size()); all.insert(all.end(), st.begin(), st.end()); }
        if (!sizes.empty()) {
            // with setInstanceKeys: the ids of the instances [lo, lo + K), fixed in the plan
            const uint32_t* const keys = instance_keys_.empty() ? nullptr : instance_keys_.data() + lo;
            ck(bce_plan_create_keyed(cc, (uint32_t)sizes.size(), sizes.data(), all.data(), K, stride_, lo * stride_, keys, &plan), "Clock(schedule upload)");
            plan_lo_ = lo; plan_K_ = K; plan_stride_ = stride_;
        }
    }
}

// ---- the bootstrap-depth schedule on the resident plan, step by step or as one hipGraph -----------------------------
// verify: verify mode's checks on the device (bce_plan_set_checks).  The reference checks every gate as it evaluates it
// (src/gate.cpp:113-120,153-160,174-181,206-213).  Here the plaintext pass runs first for all levels, its bits become the
// expected values of the plan's per-step check lists, and the report is read once, after the last step.
void Circuit::clockSteps(bool verify) {
    if (!verify && opt_.verify) throw std::logic_error("re-levelled schedule is not available in verify mode");
    const auto [lo, hi] = instanceRange();
    const uint32_t K = hi - lo;
    if (verify) for (size_t l = 0; l < levels_.size(); ++l) plainRound(l);
    bce_plan*& plan = verify ? vplan_ : plan_;   // a plan of its own: the verify-off runs keep theirs (and its captured graph)
    ensurePlan(plan, lo, K);
    if (verify) check_report_ = bce_check_report{};
    if (verify && plan) {
        if (!vplan_checks_) {
            const sched::CheckLists all = sched::check_lists(steps_, net_);
            check_gates_.clear();
            check_wires_.clear();
            std::vector<uint32_t> sizes;
            for (size_t s = 0; s < steps_.steps.size(); ++s) {
                if (steps_.steps[s].empty()) continue;   // the plan holds the non-empty steps
                check_gates_.push_back(all.gates[s]);
                sizes.push_back((uint32_t)all.wires[s].size());
                check_wires_.insert(check_wires_.end(), all.wires[s].begin(), all.wires[s].end());
            }
            ck(bce_plan_set_checks(cc, plan, sizes.data(), check_wires_.data(), 1), "Clock(check lists)");
            vplan_checks_ = true;
        }
        const std::vector<uint8_t> expect = armChecks(lo, hi, check_wires_);
        if (!expect.empty()) ck(bce_plan_set_expected(cc, plan, expect.data()), "Clock(expected bits)");
    }
    const bool graph = plan && runMode().graph;
    if (graph) ck(bce_plan_run(cc, plan), "Clock(schedule graph)");
    uint32_t ps = 0;
    for (size_t s = 0; s < steps_.steps.size(); ++s) {
        if (plan && !steps_.steps[s].empty()) {
            if (!graph) ck(bce_plan_run_step(cc, plan, ps++), "Clock(re-levelled step)");
            ++stats_.sublaunches;
        }
        if (!graph && gateSharded()) exchangeWires(steps_.publish[s]);   // outputs of this step whose consumers sit on other ranks
    }
    if (verify && plan) reportChecks(&check_gates_, nullptr);
    finishReleveled(lo, hi, verify);
    stats_.levels = (uint32_t)steps_.steps.size();
}

// verify prologue once the plan / DAG exists: the plaintext pass's bits of `wires`, instance after instance, and a fresh report
std::vector<uint8_t> Circuit::armChecks(unsigned lo, unsigned hi, const std::vector<uint32_t>& wires) {
    std::vector<uint8_t> expect;
    for (unsigned i = lo; i < hi; ++i)
        for (uint32_t w : wires) expect.push_back(plain_[i][w]);
    ck(bce_check_reset(cc), "Clock(check reset)");
    return expect;
}

// the report of the run, read once: one "Bad <OP> fixing" line per logged mismatch, all mismatches into verify_fixes.  The
// owning gate of a log entry: by_tag[tag][index] (step schedule: tag = step) or by_index[index] (dataflow: tag = task)
void Circuit::reportChecks(const std::vector<std::vector<uint32_t>>* by_tag, const std::vector<uint32_t>* by_index) {
    std::vector<bce_check_entry> log(BCE_CHECK_LOG_CAP);
    ck(bce_check_get(cc, &check_report_, log.data(), (uint32_t)log.size()), "Clock(check report)");
    for (uint32_t k = 0; k < check_report_.log_count; ++k) {
        const bce_check_entry& e = log[k];
        const char* name = "?";
        int64_t gate = -1;
        if (by_tag && e.tag < by_tag->size() && e.index < (*by_tag)[e.tag].size()) gate = (*by_tag)[e.tag][e.index];
        if (by_index && e.index < by_index->size()) gate = (*by_index)[e.index];
        if (gate >= 0) {
            const sched::Op op = net_.gates[gate].op;
            name = op == sched::Op::AND ? "AND" : op == sched::Op::OR ? "OR" : "XOR";
        }
        std::cerr << "Bad " << name << " fixing" << std::endl;
    }
    if (check_report_.mismatches > check_report_.log_count)
        std::cerr << "(" << (check_report_.mismatches - check_report_.log_count) << " more mismatches than the device log holds)" << std::endl;
    stats_.verify_fixes += (uint32_t)check_report_.mismatches;
}

// OUTPUT gates: compared, counted and reported, not repaired (as the gate-level path does)
void Circuit::compareOutputs(unsigned lo, unsigned hi) {
    for (const GateRec& g : allGates) {
        if (g.op != GateEnum::OUTPUT) continue;
        for (unsigned i = lo; i < hi; ++i) {
            if (circuitOut[i][g.out_bit] == plain_[i][g.in[0]]) continue;
            std::cerr << "Bad OUTPUT fixing" << std::endl;
            ++stats_.verify_fixes;
        }
    }
}

// ---- dataflow schedule: the whole bootstrap DAG in one persistent launch (bce_dag_*) -------------------------------
// Tasks = the units of the bootstrap-depth schedule in topological order, an XOR as its two ANDs and its OR with
// temporaries of its own (SSA: the device runs independent tasks in any order, so no slot may be reused); sched::lower_tasks.
// Under the shared lowering there is a list only with setDataflowShared: a pair task into the same two temporaries, then the AND.
void Circuit::setDataflow(bool b) {
    if (b) refuseWithKeys("setDataflow");
    if (inputs_set_) {
        // the pool layout is fixed.  The schedule can be switched off and on again while that layout has room for its
        // temporaries (it was chosen when the inputs were set; tools/verify_cost.py alternates the schedules on one set of
        // input ciphertexts): only the choice changes, the schedules and their resident plans and DAGs stay as they are
        if (b && tasks_.tasks.empty() && tasksExist()) {
            sched::TaskList t = lowerTasks();
            if (t.stride > stride_) throw std::logic_error("setDataflow: choose the dataflow schedule before SetInput (it lays the pool out with its own temporaries)");
            tasks_ = std::move(t);
        }
        opt_.dataflow = b;
        return;
    }
    opt_.dataflow = b;
    rebuildRelevel();
}

// Opt-in: shared XORs on the dataflow schedule.  The task list is then lowered in XorMode::Shared -- a pair task and an AND
// per XOR -- and goes to the engine through bce_dag_create_pairs.  Part of the pool layout and of the lowering: before SetInput.
void Circuit::setDataflowShared(bool b) {
    if (inputs_set_ && b != opt_.dataflow_shared) throw std::logic_error("setDataflowShared: choose the dataflow schedule of the shared XOR lowering before SetInput");
    if (b == opt_.dataflow_shared) return;
    opt_.dataflow_shared = b;
    tasks_ = {};          // the list depends on the flag where the units are shared
    rebuildRelevel();
}

void Circuit::createDag(bce_dag** g) {
    const auto create = tasksHavePairs() ? bce_dag_create_pairs : bce_dag_create;
    ck(create(cc, (uint32_t)tasks_.tasks.size(), tasks_.tasks.data(), tasks_.prio.data(), g), "Clock(dataflow DAG)");
}

// verify: the checks of clockSteps inside the persistent kernel (setDataflow + setDeviceVerify + setVerify).  The plaintext
// pass's bits become the expected values of the DAG's checks (sched::task_checks: the same (register, gate) pairs as the
// step plan's lists), ONE bce_dag_run follows in which every workgroup checks and repairs its task's output before it
// releases the consumers -- where Gate::Evaluate does it, src/gate.cpp:153-160 -- and the report is read once.
void Circuit::clockDag(bool verify) {
    const auto [lo, hi] = instanceRange();
    const uint32_t K = hi - lo;
    if (tasks_.stride > stride_) throw std::logic_error("dataflow schedule needs more scratch slots than the pool stride");
    if (steps_.steps.empty()) rebuildRelevel();
    if (verify) for (size_t l = 0; l < levels_.size(); ++l) plainRound(l);
    if (verify) check_report_ = bce_check_report{};
    bce_dag*& dag = verify ? vdag_ : dag_;   // a DAG of its own: the verify-off runs keep theirs
    if (!dag) {
        createDag(&dag);
        if (verify) {
            task_checks_ = sched::task_checks(tasks_, units_, net_);
            ck(bce_dag_set_checks(cc, dag, (uint32_t)task_checks_.tasks.size(), task_checks_.tasks.data(), 1), "Clock(check list)");
        }
    }
    if (K) {
        if (verify) {
            const std::vector<uint8_t> expect = armChecks(lo, hi, task_checks_.wires);
            if (!expect.empty()) ck(bce_dag_set_expected(cc, dag, K, expect.data()), "Clock(expected bits)");
        }
        ck(bce_dag_run(cc, dag, K, stride_, lo * stride_), "Clock(dataflow run)");
        ++stats_.sublaunches;
        if (verify) reportChecks(nullptr, &task_checks_.gates);
    }
    finishReleveled(lo, hi, verify);
    stats_.levels = 1;
}

// NOT wires the OUTPUT gates read, OUTPUT gates (decrypt), gate counts, in verify mode the OUTPUT gates against the plaintext
// pass: common end of the two DAG-level schedules
void Circuit::finishReleveled(unsigned lo, unsigned hi, bool verify) {
    evalStrided(steps_.output_nots, lo, hi - lo, "Clock(output NOTs)");
    decryptOutputs(lo, hi, nullptr);
    countGates(nullptr);
    if (verify) compareOutputs(lo, hi);
}

// descriptors address instance 0; a strided call replicates them K times from instance `lo` on
std::vector<bce_gate_desc> Circuit::rebased(std::vector<bce_gate_desc> descs, unsigned lo) const {
    for (auto& d : descs) { d.in0 += lo * stride_; d.in1 += lo * stride_; d.out += lo * stride_; }
    return descs;
}
void Circuit::evalStrided(const std::vector<bce_gate_desc>& descs, unsigned lo, uint32_t K, const char* what) {
    if (descs.empty() || !K) return;
    const std::vector<bce_gate_desc> d = rebased(descs, lo);
    ck(bce_eval_gates_keyed(cc, (uint32_t)d.size(), d.data(), K, stride_, instance_keys_.empty() ? nullptr : instance_keys_.data() + lo), what);
    ++stats_.sublaunches;
}

// retire the OUTPUT gates among `gates` (src/circuit.cpp:796-807): decrypt, or take the plaintext pass's bit
void Circuit::decryptOutputs(unsigned lo, unsigned hi, const std::vector<int>* gates) {
    std::vector<uint32_t> oslots;
    std::vector<std::pair<unsigned, int>> obits;
    const size_t n = gates ? gates->size() : allGates.size();
    for (size_t k = 0; k < n; ++k) {
        const GateRec& g = allGates[gates ? (*gates)[k] : k];
        if (g.op != GateEnum::OUTPUT) continue;
        if (!opt_.encrypted && !opt_.plaintext) std::cerr << "Error either encrypted or plaintext flag must be set" << std::endl;
        for (unsigned i = lo; i < hi; ++i) {
            if (opt_.encrypted) { oslots.push_back(i * stride_ + g.in[0]); obits.push_back({i, g.out_bit}); }
            else circuitOut[i][g.out_bit] = plain_[i][g.in[0]];
        }
    }
    if (!oslots.empty()) {
        std::vector<uint8_t> res(oslots.size());
        if (instance_keys_.empty()) {
            ck(bce_decrypt_bits(cc, oslots.data(), (uint32_t)oslots.size(), res.data()), "Clock(Decrypt)");
        } else {   // one gather; every output bit under its instance's key set
            std::vector<uint32_t> sets(oslots.size());
            for (size_t k = 0; k < oslots.size(); ++k) sets[k] = instance_keys_[obits[k].first];
            ck(bce_decrypt_bits_keyed(cc, oslots.data(), (uint32_t)oslots.size(), sets.data(), res.data()), "Clock(Decrypt)");
        }
        for (size_t k = 0; k < oslots.size(); ++k) circuitOut[obits[k].first][obits[k].second] = res[k];
    }
}

// counters, once per evaluation (src/circuit.cpp:722-749)
void Circuit::countGates(const std::vector<int>* gates) {
    const size_t n = gates ? gates->size() : allGates.size();
    for (size_t k = 0; k < n; ++k) {
        switch (allGates[gates ? (*gates)[k] : k].op) {
            case GateEnum::OUTPUT: ++n_output_gates; break;
            case GateEnum::NOT: ++n_not_gates; break;
            case GateEnum::AND: ++n_and_gates; break;
            case GateEnum::OR: ++n_or_gates; break;
            case GateEnum::XOR: ++n_xor_gates; break;
            default: break;
        }
    }
}

// ---- Clock -------------------------------------------------------------------------------------
void Circuit::managerRound(size_t) {
    // Readiness was resolved once in finalizeNetlist(); the per-round work the reference does here
    // (src/circuit.cpp:575-683: scanning waitingGates for every active wire) has no counterpart.
}

// the plaintext pass of one gate level, for this rank's instances (and, under gate sharding, its gates)
void Circuit::plainRound(size_t level) {
    const Level& L = levels_[level];
    const auto [lo, hi] = instanceRange();
    auto mine = [&](size_t k) { return !gateSharded() || shard_.owner[level][k] == 0xFF || shard_.owner[level][k] == rank_; };
    for (unsigned i = lo; i < hi; ++i) {
        auto& pv = plain_[i];
        for (size_t k = 0; k < L.gates.size(); ++k) {
            if (!mine(k)) continue;
            const GateRec& g = allGates[L.gates[k]];
            switch (g.op) {
                case GateEnum::NOT: pv[g.out] = !pv[g.in[0]]; break;
                case GateEnum::AND: pv[g.out] = pv[g.in[0]] && pv[g.in[1]]; break;
                case GateEnum::OR: pv[g.out] = pv[g.in[0]] || pv[g.in[1]]; break;
                case GateEnum::XOR: pv[g.out] = pv[g.in[0]] ^ pv[g.in[1]]; break;
                default: break;
            }
        }
    }
}

void Circuit::executeRound(size_t level) {
    const Level& L = levels_[level];
    const auto [lo, hi] = instanceRange();
    auto mine = [&](size_t k) { return !gateSharded() || shard_.owner[level][k] == 0xFF || shard_.owner[level][k] == rank_; };

    const sched::XorMode xm = xorMode();   // the rounds spell a Shared XOR as the reference does
    const bool xor_one = xm == sched::XorMode::Fast || xm == sched::XorMode::Single, xor_single = xm == sched::XorMode::Single;
    if (opt_.plaintext) plainRound(level);
    if (opt_.encrypted) {
        requireEngine("Clock");
        const uint32_t tmp0 = (uint32_t)wire_names_.size();
        if (opt_.batched) {
            // stage A: AND / OR gates and the two ANDs of every XOR; stage B: the OR of every XOR
            std::vector<bce_gate_desc> A, B;
            uint32_t x = 0;
            for (size_t k = 0; k < L.gates.size(); ++k) {
                const GateRec& g = allGates[L.gates[k]];
                const bool me = mine(k);
                if (g.op == GateEnum::XOR && xor_one) {
                    if (me) A.push_back({(uint32_t)(xor_single ? BCE_XOR : BCE_XOR_FAST), (uint32_t)g.in[0], (uint32_t)g.in[1], (uint32_t)g.out, 0, 0});
                } else if (g.op == GateEnum::XOR) {
                    const uint32_t t1 = tmp0 + 2 * x, t2 = t1 + 1;
                    ++x;
                    if (!me) continue;
                    bce_gate_desc q[3];
                    sched::xor_lower({0, (uint32_t)g.in[0], (uint32_t)g.in[1], (uint32_t)g.out, 0, 0}, t1, t2, q);
                    A.insert(A.end(), q, q + 2);
                    B.push_back(q[2]);
                } else if (!me) {
                    continue;
                } else if (g.op == GateEnum::AND || g.op == GateEnum::OR) {
                    A.push_back({(uint32_t)(g.op == GateEnum::AND ? BCE_AND : BCE_OR), (uint32_t)g.in[0], (uint32_t)g.in[1], (uint32_t)g.out, 0, 0});
                } else if (g.op == GateEnum::NOT) {
                    A.push_back({BCE_OP_NOT, (uint32_t)g.in[0], (uint32_t)g.in[0], (uint32_t)g.out, 0, 0});
                }
            }
            evalStrided(A, lo, hi - lo, "Clock(stage A)");
            evalStrided(B, lo, hi - lo, "Clock(stage B)");
        } else {
            // reference shape: one Gate::Evaluate per gate (src/circuit.cpp:698-710)
            // plaintext was done above for every instance and the level's checks follow below: encrypted only
            GateEvalParams p;
            p.encrypted_flag = true; p.cc = cc; p.xor_fast = xm == sched::XorMode::Fast; p.xor_single = xor_single;
            for (unsigned i = lo; i < hi; ++i) {
                uint32_t x = 0;
                for (size_t k = 0; k < L.gates.size(); ++k) {
                    const GateRec& g = allGates[L.gates[k]];
                    uint32_t xi = (g.op == GateEnum::XOR) ? x++ : 0;
                    if (!mine(k) || g.op == GateEnum::OUTPUT) continue;
                    Gate ge;
                    ge.name = g.name; ge.op = g.op;
                    for (int q = 0; q < g.nin; ++q) { ge.encin.push_back(i * stride_ + g.in[q]); ge.ready.push_back(true); }
                    ge.encout.assign(1, i * stride_ + g.out);
                    ge.tmp = {i * stride_ + tmp0 + 2 * xi, i * stride_ + tmp0 + 2 * xi + 1};
                    ge.Evaluate(p);
                }
            }
        }
        if (opt_.verify) {
            // decrypt every output of the level, compare with the plaintext pass, repair mismatches
            std::vector<uint32_t> slots;
            std::vector<uint8_t> expect;
            std::vector<const char*> names;
            for (unsigned i = lo; i < hi; ++i)
                for (size_t k = 0; k < L.gates.size(); ++k) {
                    const GateRec& g = allGates[L.gates[k]];
                    if (!mine(k)) continue;
                    int w = g.op == GateEnum::OUTPUT ? g.in[0] : g.out;
                    slots.push_back(i * stride_ + w);
                    expect.push_back(plain_[i][w]);
                    names.push_back(op_name(g.op));
                }
            std::vector<uint8_t> got(slots.size());
            if (!slots.empty()) ck(bce_decrypt_bits(cc, slots.data(), (uint32_t)slots.size(), got.data()), "Clock(verify)");
            for (size_t k = 0; k < slots.size(); ++k) {
                if (got[k] == expect[k]) continue;
                std::cerr << "Bad " << names[k] << " fixing" << std::endl;
                ++stats_.verify_fixes;
                if (std::strcmp(names[k], "OUTPUT") != 0)
                    ck(bce_encrypt_bits(cc, &expect[k], &slots[k], 1, (1ull << 40) + enc_counter_++, encrypt_mode_), "Clock(fix)");
            }
        }
    }
    if (gateSharded()) exchangeWires(shard_.publish[level]);   // wires of this level whose consumers sit on other ranks

    countGates(&L.gates);
    decryptOutputs(lo, hi, &L.gates);
}

Outputs Circuit::Clock() {
    if (done) throw std::logic_error("done ckt clocked! should reset");  // the reference exits (src/circuit.cpp:538-541)
    if (!inputs_set_) throw std::logic_error("Clock: SetInput has not been called (no active wires)");
    if (!opt_.plaintext && !opt_.encrypted) throw std::logic_error("Error either encrypted or plaintext flag must be set");
    auto t_total = Clock_t::now();
    double management = 0, execution = 0;
    uint64_t boots0 = 0;
    if (opt_.encrypted) {
        requireEngine("Clock");
        ck(bce_pool_reserve(cc, instances_ * stride_), "Clock(pool)");
        bce_timing t;
        ck(bce_timing_get(cc, &t), "Clock");
        boots0 = t.bootstraps;
    }
    size_t done_gates = 0;
    // gate-level rounds (the reference's Clock loop), the bootstrap-depth step schedule or the dataflow kernel: run_mode.hpp
    const RunMode mode = runMode();
    keysCombinationSupported("Clock");
    if (!instance_keys_.empty() && mode.path != RunPath::Steps)
        throw Unsupported("Clock: setInstanceKeys runs the bootstrap-depth step schedule only (encrypted, batched, relevel on, no plaintext pass)");
    const bool releveled = mode.path != RunPath::Rounds;
    if (releveled) {
        auto t0 = Clock_t::now();
        if (mode.path == RunPath::Dag) clockDag(mode.device_checks);
        else clockSteps(mode.device_checks);
        execution += ms_since(t0);
        done_gates = allGates.size();
    }
    for (size_t l = 0; l < levels_.size() && inputs_set_ && !releveled; ++l) {
        auto t0 = Clock_t::now();
        managerRound(l);
        management += ms_since(t0);
        t0 = Clock_t::now();
        executeRound(l);
        execution += ms_since(t0);
        done_gates += levels_[l].gates.size();
        ++stats_.levels;
        if (!quiet_) std::cout << "\rProcessing: " << done_gates << " of " << allGates.size() << std::flush;
    }
    if (opt_.encrypted) {
        auto t0 = Clock_t::now();
        bce_timing t;
        ck(bce_timing_get(cc, &t), "Clock");  // synchronizes
        stats_.bootstraps = t.bootstraps - boots0;
        execution += ms_since(t0);
    }
    gatherOutputs();
    if (done_gates == allGates.size()) done = true;
    stats_.total_ms = ms_since(t_total);
    stats_.management_ms = management;
    stats_.execution_ms = execution;
    if (!quiet_) {
        std::cout << std::endl << "### Total time " << (unsigned)std::max(1.0, stats_.total_ms) << " msec" << std::endl;
        std::cout << std::endl << "efficiency " << float(std::max(1.0, execution)) / float(std::max(1.0, stats_.total_ms)) * 100.0 << "%" << std::endl;
    }
    return getOutputs(0);
}

Outputs Circuit::getOutputs(unsigned instance) const {
    // one vector per output value (Bristol Fashion circuits may have several; the reference has one, src/circuit.cpp:183-185)
    Outputs o(std::max<size_t>(1, out_bus_bits_.size()));
    if (instance >= circuitOut.size()) return o;
    const auto& bits = circuitOut[instance];
    size_t pos = 0;
    for (size_t b = 0; b < out_bus_bits_.size(); ++b) {
        const size_t w = std::min<size_t>(out_bus_bits_[b], bits.size() - std::min(bits.size(), pos));
        o[b].assign(bits.begin() + pos, bits.begin() + pos + w);
        pos += w;
    }
    if (out_bus_bits_.empty()) o[0].assign(bits.begin(), bits.end());
    return o;
}

void Circuit::getCounts(uint32_t out[6]) const {
    out[0] = n_input_gates; out[1] = n_output_gates; out[2] = n_not_gates;
    out[3] = n_and_gates; out[4] = n_or_gates; out[5] = n_xor_gates;
}

bce_circuit_info Circuit::info() const {
    bce_circuit_info I{};
    I.n_gates = (uint32_t)allGates.size();
    I.n_input_gates = (uint32_t)inputGates.size();
    I.n_wires = (uint32_t)wire_names_.size();
    I.n_inputs = n_buses_;
    I.n_input_bits[0] = n_in_bits_.size() > 0 ? n_in_bits_[0] : 0;   // every bus: bce_circuit_get_buses()
    I.n_input_bits[1] = n_in_bits_.size() > 1 ? n_in_bits_[1] : 0;
    I.n_output_bits = n_output_bits.empty() ? 0 : n_output_bits[0];
    I.n_levels = (uint32_t)levels_.size();
    I.n_relevel_steps = (uint32_t)steps_.steps.size();
    I.slot_stride = stride_;
    for (const auto& L : levels_) {
        uint32_t a = 0, b = 0;
        for (int gi : L.gates) {
            // an XOR: two ANDs in stage A, their OR in stage B (3), or a pair in stage A and an AND in stage B (2, shared)
            const uint32_t w = sched::gate_weight(sched_op(allGates[gi].op), xorMode());
            a += w >= 2 ? w - 1 : w;
            b += w >= 2;
        }
        if (a) ++I.n_sublaunches;
        if (b) ++I.n_sublaunches;
        I.max_frontier = std::max(I.max_frontier, std::max(a, b));
        I.n_bootstraps += a + b;
    }
    return I;
}

void Circuit::dumpNetList() const {
    std::cout << "Netlist " << std::endl;
    NetList nl;
    for (size_t w = 0; w < wire_names_.size(); ++w) {
        NameList& f = nl[wire_names_[w]];
        for (uint32_t e = fan_off_[w]; e < fan_off_[w + 1]; ++e) f.push_back(allGates[fan_gate_[e]].name);
    }
    for (const auto& it : nl) {
        std::cout << it.first;
        for (const auto& g : it.second) std::cout << " " << g;
        std::cout << std::endl;
    }
}

void Circuit::dumpGates() const {
    std::cout << "Inputlist " << std::endl;
    for (const auto& l : inputGates) std::cout << l.name << std::endl;
    std::cout << "Alllist " << std::endl;
    for (const auto& g : allGates) std::cout << g.name << std::endl;
}

void Circuit::dumpGateCount() const {
    std::cout << "Number of input gates " << n_input_gates << std::endl;
    std::cout << "Number of output gates " << n_output_gates << std::endl;
    std::cout << "Number of not gates " << n_not_gates << std::endl;
    std::cout << "Number of and gates " << n_and_gates << std::endl;
    std::cout << "Number of or gates " << n_or_gates << std::endl;
    std::cout << "Number of xor gates " << n_xor_gates << std::endl;
}

}  // namespace bce
