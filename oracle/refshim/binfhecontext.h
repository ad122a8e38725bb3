/*
 * binfhecontext.h -- TEST INFRASTRUCTURE ONLY: a stand-in for OpenFHE's header of the same name.
 *
 * The reference's circuit runtime, assembler and test benches reach OpenFHE through a small surface only:
 * BinFHEContext::{GenerateBinFHEContext, KeyGen, BTKeyGen, Encrypt, Decrypt, EvalNOT, EvalBinGate}, the enums
 * BINFHE_PARAMSET / BINFHE_METHOD / BINGATE, the types LWECiphertext / LWEPrivateKey / LWEPlaintext and the
 * macros OPENFHE_DEBUG_FLAG, OPENFHE_DEBUG, OPENFHE_DEBUGEXP, TIC, TOC, TOC_MS, TimeVar.  This file provides that
 * surface and nothing else, so that the UNMODIFIED reference sources compile (oracle/Makefile, target `ref`) and their
 * own Circuit / assemble_bristol / TB_* programs become the ground truth of the tests.
 *
 * Two back ends, chosen at compile time:
 *   (default)            bits:   a ciphertext is its plaintext bit.  Free; for the test benches and the round structure.
 *   -DREFSHIM_ORACLE     oracle: a ciphertext is an LWE row of libbinfhe_oracle.so (binfhe_oracle.h).
 *
 * Oracle back end, how it lines up with the engine (csrc/prng.hpp, DESIGN.md "PRNG spec", csrc/engine.cpp
 * bce_encrypt_bits, csrc/circuit.cpp Circuit::SetInput):
 *   * KeyGen + BTKeyGen = bo_keygen(seed); seed = the integer in $BCE_REF_SEED as 32 little-endian bytes, which is what
 *     BinFHEContext.KeyGen(seed) / set_encrypt_seed(seed) of the Python package pass down.
 *   * Encrypt(sk, bit) = the engine's BOOTSTRAPPED mode: a fresh encryption drawn from the ChaCha20 stream
 *     (seed, domain ENC = 5, index), n uniform masks then one Gaussian, followed by one refresh bootstrap (bo_bootstrap).
 *     The index is base + (number of Encrypt calls since the base was set).  The engine's Circuit::SetInput uses
 *     base = (epoch << 44) | (instance << 24) with epoch = number of Reset() calls so far, the one ReadFile makes
 *     included (so 2 for the caller's first Reset), and
 *     numbers the LOADs of one SetInput 0, 1, ... in file order -- the order in which the reference's SetInput calls
 *     Encrypt.  refshim_set_encrypt_index(base) is how our driver (ref_run.cpp) names the base; $BCE_REF_ENC_BASE is the
 *     start value for programs that do not.
 *   * EvalBinGate / EvalNOT / Decrypt are bo_eval_bingate / bo_eval_not / bo_decrypt.
 *
 * Call trace, appended to the file $BCE_REF_TRACE names (both back ends), one record per call:
 *     E id bit lvl        Encrypt -> ciphertext id          lvl = omp_get_level(): 0 in SetInput and in the serial
 *     D id bit lvl        Decrypt of id gave bit                  part of _ExecuteGates (OUTPUT gates), 1 inside a gate task
 *     N out in            EvalNOT
 *     G op out in0 in1    EvalBinGate, op = AND | OR | ...
 *     C id w0 .. wn       (oracle back end) the LWE row of id: a[0..n), b
 *     M text              a marker our own driver writes (refshim_mark)
 * Ids are handed out, and records written, under one mutex: _ExecuteGates is an OpenMP region.  Gate evaluation is
 * deterministic given the key, so rows do not depend on thread order; only the numbering of ids does, and no reader
 * may rely on it.
 */
#ifndef REFSHIM_BINFHECONTEXT_H
#define REFSHIM_BINFHECONTEXT_H

#include <omp.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef REFSHIM_ORACLE
#include "binfhe_oracle.h"
#endif

#define OPENFHE_DEBUG_FLAG(x) do { } while (0)
#define OPENFHE_DEBUG(x) do { } while (0)
#define OPENFHE_DEBUGEXP(x) do { } while (0)
using TimeVar = std::chrono::steady_clock::time_point;
#define TIC(t) t = std::chrono::steady_clock::now()
#define TOC_MS(t) (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - (t)).count())
#define TOC(t) TOC_MS(t)

namespace lbcrypto {

// binfhe-constants.h, v1.0.x order
enum BINFHE_PARAMSET { TOY, MEDIUM, STD128_AP, STD128_APOPT, STD128, STD128_OPT, STD192, STD192_OPT, STD256, STD256_OPT };
enum BINFHE_METHOD { INVALID_METHOD = 0, AP, GINX };
enum BINGATE { OR, AND, NOR, NAND, XOR_FAST, XNOR_FAST, XOR, XNOR };

using LWEPlaintext = int64_t;

struct LWECiphertextImpl {
    uint64_t id = 0;
    int bit = 0;                  // bits back end: the value
    std::vector<uint64_t> row;    // oracle back end: a[0..n), b
};
using LWECiphertext = std::shared_ptr<const LWECiphertextImpl>;
struct LWEPrivateKeyImpl {};
using LWEPrivateKey = std::shared_ptr<const LWEPrivateKeyImpl>;

namespace refshim {
struct Trace {
    std::mutex mu;
    FILE* f = nullptr;
    uint64_t next_id = 0;
    uint64_t enc_index = 0;
    Trace() {
        if (const char* p = std::getenv("BCE_REF_TRACE")) f = std::fopen(p, "a");
        if (const char* b = std::getenv("BCE_REF_ENC_BASE")) enc_index = std::strtoull(b, nullptr, 0);
    }
    ~Trace() { if (f) std::fclose(f); }
};
inline Trace& trace() { static Trace t; return t; }
inline const char* gate_name(BINGATE g) {
    static const char* n[] = {"OR", "AND", "NOR", "NAND", "XOR_FAST", "XNOR_FAST", "XOR", "XNOR"};
    return n[(int)g];
}
}  // namespace refshim

// extensions for our own driver only (the reference never calls them)
inline void refshim_set_encrypt_index(uint64_t base) {
    auto& t = refshim::trace();
    std::lock_guard<std::mutex> l(t.mu);
    t.enc_index = base;
}
inline void refshim_mark(const std::string& text) {
    auto& t = refshim::trace();
    std::lock_guard<std::mutex> l(t.mu);
    if (t.f) { std::fprintf(t.f, "M %s\n", text.c_str()); std::fflush(t.f); }
}

class BinFHEContext {
    struct State {
#ifdef REFSHIM_ORACLE
        bo_ctx* o = nullptr;
        ~State() { if (o) bo_ctx_destroy(o); }
#endif
    };
    std::shared_ptr<State> st_;

    // hands out the id and writes the record (and the row) under the mutex
    LWECiphertext finish(std::shared_ptr<LWECiphertextImpl> c, const std::string& head, const std::string& tail) const {
        auto& t = refshim::trace();
        std::lock_guard<std::mutex> l(t.mu);
        c->id = t.next_id++;
        if (t.f) {
            std::fprintf(t.f, "%s %llu%s\n", head.c_str(), (unsigned long long)c->id, tail.c_str());
            if (!c->row.empty()) {
                std::fprintf(t.f, "C %llu", (unsigned long long)c->id);
                for (uint64_t w : c->row) std::fprintf(t.f, " %llu", (unsigned long long)w);
                std::fputc('\n', t.f);
            }
        }
        return c;
    }

public:
    void GenerateBinFHEContext(BINFHE_PARAMSET set, BINFHE_METHOD method) {
        st_ = std::make_shared<State>();
#ifdef REFSHIM_ORACLE
        st_->o = bo_ctx_create((int)set, (int)method);   // same enum values as BO_TOY.. / BO_AP, BO_GINX
        if (!st_->o) throw std::runtime_error("refshim: bad oracle parameters");
#else
        (void)set; (void)method;
#endif
    }
    LWEPrivateKey KeyGen() const { return std::make_shared<LWEPrivateKeyImpl>(); }
    void BTKeyGen(const LWEPrivateKey&) {
#ifdef REFSHIM_ORACLE
        uint8_t seed[32] = {0};
        const char* s = std::getenv("BCE_REF_SEED");
        uint64_t v = s ? std::strtoull(s, nullptr, 0) : 0;
        for (int i = 0; i < 8; ++i) seed[i] = (uint8_t)(v >> (8 * i));
        bo_keygen(st_->o, seed);
#endif
    }
    LWECiphertext Encrypt(const LWEPrivateKey&, LWEPlaintext m) const {
        auto c = std::make_shared<LWECiphertextImpl>();
        c->bit = (int)(m & 1);
#ifdef REFSHIM_ORACLE
        uint64_t index;
        {
            auto& t = refshim::trace();
            std::lock_guard<std::mutex> l(t.mu);
            index = t.enc_index++;
        }
        const size_t W = words();
        std::vector<uint64_t> fresh(W);
        c->row.resize(W);
        bo_encrypt(st_->o, c->bit, index, fresh.data());
        bo_bootstrap(st_->o, fresh.data(), c->row.data());   // BOOTSTRAPPED: OpenFHE v1.0.x's default output mode
#endif
        return finish(c, "E", " " + std::to_string(c->bit) + " " + std::to_string(omp_get_level()));
    }
    void Decrypt(const LWEPrivateKey&, const LWECiphertext& ct, LWEPlaintext* res) const {
#ifdef REFSHIM_ORACLE
        *res = bo_decrypt(st_->o, ct->row.data());
#else
        *res = ct->bit;
#endif
        auto& t = refshim::trace();
        std::lock_guard<std::mutex> l(t.mu);
        if (t.f) std::fprintf(t.f, "D %llu %d %d\n", (unsigned long long)ct->id, (int)*res, omp_get_level());
    }
    LWECiphertext EvalNOT(const LWECiphertext& a) const {
        auto c = std::make_shared<LWECiphertextImpl>();
        c->bit = !a->bit;
#ifdef REFSHIM_ORACLE
        c->row.resize(words());
        bo_eval_not(st_->o, a->row.data(), c->row.data());
#endif
        return finish(c, "N", " " + std::to_string(a->id));
    }
    LWECiphertext EvalBinGate(BINGATE g, const LWECiphertext& a, const LWECiphertext& b) const {
        auto c = std::make_shared<LWECiphertextImpl>();
        switch (g) {
            case OR: c->bit = a->bit | b->bit; break;
            case AND: c->bit = a->bit & b->bit; break;
            case NOR: c->bit = !(a->bit | b->bit); break;
            case NAND: c->bit = !(a->bit & b->bit); break;
            case XOR_FAST: case XOR: c->bit = a->bit ^ b->bit; break;
            default: c->bit = !(a->bit ^ b->bit); break;
        }
#ifdef REFSHIM_ORACLE
        if ((int)g > (int)XNOR_FAST) throw std::runtime_error("refshim: gate outside the oracle's set");
        c->row.resize(words());
        bo_eval_bingate(st_->o, (int)g, a->row.data(), b->row.data(), c->row.data());
#endif
        return finish(c, std::string("G ") + refshim::gate_name(g), " " + std::to_string(a->id) + " " + std::to_string(b->id));
    }

private:
#ifdef REFSHIM_ORACLE
    size_t words() const {
        uint64_t p[BO_P_COUNT];
        bo_get_params(st_->o, p);
        return (size_t)p[BO_P_n] + 1;
    }
#endif
};

}  // namespace lbcrypto
#endif
