// ctx_params_selftest.cpp -- csrc/ctx_params.cpp alone: compiled with it by the host compiler (no HIP runtime, no kernels, no
// library) under AddressSanitizer and UndefinedBehaviorSanitizer, with a kernel_class that answers what this file scripts.
// Sweeps valid and rejected shapes out to the widest arguments the checks let through (Q up to 2^40 - 1, baseG up to 2^31,
// qKS up to 2^32 - 1), so that every shift count and narrowing cast of the derivation runs under the sanitizers, and checks
// that what kernel_class says (no kernel, LDS does not fit, no folded build, LDS bytes) reaches the caller.
// Run by tests/test_ctx_params_standalone.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/ctx_params.hpp"
#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/host_math.hpp"

using namespace bce;

namespace {

struct Script {
    const char* error = nullptr;
    const char* lds_error = nullptr;
    bool fold_build = true;
    size_t lds_bytes = 70000;
    u32 wg_per_cu_full = 2;
} g_script;
int g_class_calls = 0;

int g_failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);  \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            ++g_failures;                                                    \
        }                                                                    \
    } while (0)

// the largest prime = 1 mod m below `bound`
u64 prime_below(u64 bound, u64 m) {
    u64 q = bound - bound % m + 1;
    while (q >= bound || !is_prime_u64(q)) q -= m;
    return q;
}

const Shape kStd128Opt{502, 1024, 1024, 134215681ull, 1u << 14, 1u << 7, 1u << 7, 32, BCE_GINX};

}  // namespace

// the scripted rule: the family follows the width and the doubles request, everything else is what g_script says
KernelClass bce::kernel_class(const DevParams& P) {
    ++g_class_calls;
    KernelClass k{};
    k.family = !P.is64 ? (P.logN == 10 && P.dG == 4 ? KernelFamily::SplitTransform : KernelFamily::WavePerTransform)
                       : P.fp64 ? KernelFamily::Fp64 : KernelFamily::Int64;
    k.error = g_script.error;
    k.lds_error = g_script.lds_error;
    k.fold_build = g_script.fold_build;
    k.dag = false;
    k.fp64 = P.fp64;
    k.occupancy_target = P.occupancy_target;
    k.wg_per_cu_lone = 1;
    k.wg_per_cu_full = g_script.wg_per_cu_full;
    k.lds_bytes = g_script.lds_bytes;
    return k;
}

int main() {
    CtxKnobs all_off;
    all_off.variant = 3; all_off.fuse_tail = false; all_off.occupancy2 = true; all_off.fp64 = false; all_off.xcd_gate = false;
    all_off.fold = false; all_off.fwd_units = false; all_off.fwd_mfma = false;
    CtxKnobs gate_us;
    gate_us.xcd_gate_us = EnvNumber{true, 0xFFFFFFFFu};
    const CtxKnobs knob_sets[] = {CtxKnobs{}, all_off, gate_us};
    u64 report[BCE_D_COUNT];

    // ---- valid shapes, out to the widest arguments ---------------------------------------------------------------------
    CHECK(is_prime_u64(kStd128Opt.Q) && (kStd128Opt.Q - 1) % 2048 == 0, "the STD128_OPT modulus");
    const u64 bounds[] = {1ull << 20, 1ull << 27, 1ull << 28, (1ull << 28) + 4096 * 40, 1ull << 31, 1ull << 32, (1ull << 32) + 4096 * 40,
                          1ull << 39, (1ull << 39) + 4096 * 40, 1ull << 40};
    const u32 gadget_bases[] = {2, 1u << 7, 1u << 13, 1u << 16, 1u << 31};
    const u64 ks_moduli[] = {0, 1, 2, 65536, 65537, 1ull << 29, 0xFFFFFFFFull};
    const u32 ks_bases[] = {2, 0xFFFFFFFFu};
    const u32 dims[] = {1, 502, 0xFFFFFFFFu};
    int ok = 0, refused = 0;
    for (u32 N : {512u, 1024u, 2048u})
        for (u64 bound : bounds) {
            const u64 Q = prime_below(bound, 2ull * N);
            for (u32 baseG : gadget_bases)
                for (u64 qKS : ks_moduli)
                    for (u32 baseKS : ks_bases) {
                        const u32 n = dims[(ok + refused) % 3];
                        const int method = (ok + refused) & 1 ? BCE_AP : BCE_GINX;
                        const u64 q = (ok + refused) % 3 == 0 ? 8 : (ok + refused) % 3 == 1 ? N : 2ull * N;
                        const u32 baseR = method == BCE_AP ? ((ok + refused) & 2 ? 2u : 1u << 31) : ((ok + refused) & 2 ? 0u : 32u);
                        const Shape s{n, N, q, Q, qKS, baseKS, baseG, baseR, method};
                        const CtxParams cp = derive_params(s, knob_sets[(ok + refused) % 3], (ok + refused) % 5 ? 256 : 0);
                        // the one refusal a shape that passes validate_shape can meet here: the key-switch gather's bound
                        const u64 ks = qKS ? qKS : Q;
                        const bool expect_ok = ks <= (1ull << 29);
                        CHECK((cp.status.code == BCE_OK) == expect_ok, "N %u Q %llu qKS %llu: status %d (%s)", N, (unsigned long long)Q,
                              (unsigned long long)qKS, cp.status.code, cp.status.message);
                        if (cp.status.code != BCE_OK) { ++refused; CHECK(cp.status.message[0] != 0, "a refusal without a message"); continue; }
                        ++ok;
                        CHECK(cp.P.Q64 == Q && cp.P.N == N && (1u << cp.P.logN) == N && (1ull << cp.P.gBits) == baseG, "shape fields");
                        CHECK(cp.P.is64 == (Q >= (1ull << 28) ? 1u : 0u) && cp.T.twf.size() == N && (cp.T.tw64.size() == N) == (cp.P.is64 != 0), "tables");
                        CHECK(pow_mod(cp.psi, N, Q) == Q - 1, "psi is a primitive 2N-th root");
                        params_report(cp, report);
                        u32 lone = 0, full = 0;
                        launch_capacity(cp.P, &lone, &full);
                        CHECK(report[BCE_D_capacity_full] == full && report[BCE_D_psi] == cp.psi, "report");
                    }
        }
    CHECK(ok > 500 && refused > 100, "the sweep ran %d accepted and %d refused shapes", ok, refused);

    // ---- rejected arguments: a status and a message, never a trap --------------------------------------------------------
    {
        int rejected = 0;
        const auto reject = [&](Shape s, int code) {
            const int calls = g_class_calls;
            const CtxParams cp = derive_params(s, CtxKnobs{}, 256);
            CHECK(cp.status.code == code && cp.status.message[0] != 0, "status %d (%s), expected %d", cp.status.code, cp.status.message, code);
            CHECK(validate_shape(s).code == code && g_class_calls == calls, "validate_shape agrees, before any derivation");
            ++rejected;
        };
        Shape s;
        for (int m : {0, 3, -1}) { s = kStd128Opt; s.method = m; reject(s, BCE_ERR_ARG); }
        for (u32 N : {0u, 1u, 256u, 1000u, 4096u, 0x80000000u, 0xFFFFFFFFu}) { s = kStd128Opt; s.N = N; reject(s, BCE_ERR_UNSUPPORTED); }
        for (u64 q : {0ull, 3ull, 4ull, 1000ull, 4096ull, 1ull << 63, ~0ull}) { s = kStd128Opt; s.q = q; reject(s, BCE_ERR_ARG); }
        for (u64 Q : {0ull, 1ull, 2ull, 2049ull * 3, 134215681ull + 2, (1ull << 61) - 1, ~0ull}) { s = kStd128Opt; s.Q = Q; reject(s, BCE_ERR_ARG); }
        { u64 Q = (1ull << 40) + 1; while (!is_prime_u64(Q)) Q += 2048; s = kStd128Opt; s.Q = Q; reject(s, BCE_ERR_UNSUPPORTED); }
        for (u32 g : {0u, 1u, 3u, 96u, 0xFFFFFFFFu}) { s = kStd128Opt; s.baseG = g; reject(s, BCE_ERR_ARG); }
        s = kStd128Opt; s.n = 0; reject(s, BCE_ERR_ARG);
        for (u32 b : {0u, 1u}) { s = kStd128Opt; s.baseKS = b; reject(s, BCE_ERR_ARG); }
        for (u32 b : {0u, 1u}) { s = kStd128Opt; s.method = BCE_AP; s.baseR = b; reject(s, BCE_ERR_ARG); }
        Shape none;
        CHECK(!tabulated_shape(-1, BCE_GINX, none) && !tabulated_shape(BCE_STD256_OPT + 1, BCE_GINX, none), "unknown sets");
        for (int p = BCE_TOY; p <= BCE_STD256_OPT; ++p) {
            CHECK(tabulated_shape(p, BCE_AP, s) && validate_shape(s).code == BCE_OK, "set %d", p);
            CHECK(derive_params(s, CtxKnobs{}, 256).status.code == BCE_OK, "set %d", p);
        }
        CHECK(rejected == 35, "%d rejected shapes", rejected);
    }
    // qKS beyond 32 bits and beyond the gather's bound: refused by the derivation, after the kernel class had its say
    {
        Shape s = kStd128Opt;
        s.qKS = 1ull << 32;
        CtxParams cp = derive_params(s, CtxKnobs{}, 256);
        CHECK(cp.status.code == BCE_ERR_UNSUPPORTED && !std::strcmp(cp.status.message, "qKS must fit 32 bits"), "%s", cp.status.message);
        s.qKS = ~0ull;
        CHECK(derive_params(s, CtxKnobs{}, 256).status.code == BCE_ERR_UNSUPPORTED, "qKS = 2^64 - 1");
        s.qKS = (1ull << 29) + 1;
        cp = derive_params(s, CtxKnobs{}, 256);
        CHECK(cp.status.code == BCE_ERR_ARG && std::strstr(cp.status.message, "key-switch gather"), "%s", cp.status.message);
    }

    // ---- what kernel_class says reaches the caller -------------------------------------------------------------------------
    Shape wide = kStd128Opt;   // a 64-bit shape: STD192's modulus class
    wide.N = 2048; wide.Q = prime_below(1ull << 37, 4096); wide.baseG = 1u << 13;
    {
        static const char kNoKernel[] = "scripted: no kernel", kNoLds[] = "scripted: LDS";
        g_script = Script{};
        g_script.error = kNoKernel;
        for (const Shape& s : {kStd128Opt, wide}) {
            const CtxParams cp = derive_params(s, CtxKnobs{}, 256);
            CHECK(cp.status.code == BCE_ERR_UNSUPPORTED && cp.status.message == kNoKernel, "error: %d %s", cp.status.code, cp.status.message);
        }
        {   // ... and speaks before the key-switch modulus does
            Shape s = kStd128Opt;
            s.qKS = 1ull << 32;
            CHECK(derive_params(s, CtxKnobs{}, 256).status.message == kNoKernel, "precedence");
        }
        g_script = Script{};
        g_script.lds_error = kNoLds;
        CtxParams cp = derive_params(wide, CtxKnobs{}, 256);
        CHECK(cp.status.code == BCE_ERR_UNSUPPORTED && cp.status.message == kNoLds, "lds_error: %d %s", cp.status.code, cp.status.message);
        {   // the gather's bound speaks before it
            Shape s = wide;
            s.qKS = (1ull << 29) + 1;
            CHECK(derive_params(s, CtxKnobs{}, 256).status.code == BCE_ERR_ARG, "precedence");
        }
        cp = derive_params(kStd128Opt, CtxKnobs{}, 256);     // the 32-bit path never asked (as before this module existed)
        CHECK(cp.status.code == BCE_OK, "lds_error on a 32-bit shape: %d %s", cp.status.code, cp.status.message);
    }
    {
        g_script = Script{};
        CtxParams cp = derive_params(kStd128Opt, CtxKnobs{}, 256);
        CHECK(cp.P.fold == 1 && cp.P.fwd_units == 1 && cp.P.fwd_mfma == 1 && cp.P.w14 != 0 && !cp.T.fwd.table.empty(), "fold %u units %u mfma %u", cp.P.fold, cp.P.fwd_units, cp.P.fwd_mfma);
        CHECK(forward_transforms_per_step(cp.P) == 6, "folded: 2 dG - 2");
        g_script.fold_build = false;
        cp = derive_params(kStd128Opt, CtxKnobs{}, 256);
        CHECK(cp.P.fold == 0 && cp.P.fold_ninv == 0 && cp.P.fwd_units == 0 && cp.P.fwd_mfma == 0, "fold_build = false: fold %u", cp.P.fold);
        CHECK(forward_transforms_per_step(cp.P) == 8, "plain: 2 dG");
        // the matrix-pipe body retreats where two of its workgroups exceed a CU's LDS: 2 x 81920 fits, one byte more does not
        g_script = Script{};
        g_script.lds_bytes = kLdsBytesPerCu / 2;
        CHECK(derive_params(kStd128Opt, CtxKnobs{}, 256).P.fwd_mfma == 1, "two workgroups fit exactly");
        g_script.lds_bytes = kLdsBytesPerCu / 2 + 1;
        cp = derive_params(kStd128Opt, CtxKnobs{}, 256);
        CHECK(cp.P.fwd_mfma == 0 && cp.P.w14 == 0 && cp.P.w14s == 0 && cp.P.fwd_units == 1, "the retreat: mfma %u", cp.P.fwd_mfma);
        // the granted requests are stored back
        g_script = Script{};
        CtxKnobs k;
        k.occupancy2 = true;
        CHECK(derive_params(kStd128Opt, k, 256).P.occupancy_target == 2 && derive_params(kStd128Opt, CtxKnobs{}, 256).P.occupancy_target == 3, "occupancy");
        CHECK(derive_params(wide, CtxKnobs{}, 256).P.fp64 == 1 && derive_params(wide, all_off, 256).P.fp64 == 0, "fp64");
    }

    // ---- launch choice: every argument at its extremes ---------------------------------------------------------------------
    {
        DevParams P{};
        int n = 0;
        for (u32 cus : {0u, 1u, 256u, 0xFFFFFFFFu})
            for (u32 depth : {0u, 1u, 0xFFFFFFFFu})
                for (u64 items : {0ull, 1ull, 100000ull, ~0ull})
                    for (int wg : {0, 1, 2})
                        for (u32 us : {0u, 20u, 0xFFFFFFFFu}) {
                            P.cu_count = cus; P.is64 = n & 1;
                            DagKnobs k;
                            if (n % 3 == 0) { k.gate_us = EnvNumber{true, 0xFFFFFFFFu}; k.gate_backlog = EnvNumber{true, 0}; k.wps = '4'; k.place = 0; k.debug = 'd'; k.gate = '0'; k.tickets = true; }
                            const DagLaunchChoice L = dag_launch_choice(P, 1 + (n & 1), n % 5 ? 1000 : ~(size_t)0 / 2, DagLimits{wg, n & 2, us, us}, k, depth, items);
                            CHECK((L.wps == 2 || L.wps == 4) && L.grid == cus * (u32)(L.wps / 2) && L.policy < 16, "wps %d grid %u", L.wps, L.grid);
                            ++n;
                        }
    }

    if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
    std::printf("ctx_params selftest ok: %d shapes derived, %d refused\n", ok, refused);
    return 0;
}
