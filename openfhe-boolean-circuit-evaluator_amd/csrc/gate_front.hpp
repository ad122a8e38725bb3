// gate_front.hpp -- the front end every blind-rotation body shares (included inside namespace bce by kernels.hip and
// kernels64.hip): EvalBinGate's LWE preparation, BootstrapGateCore's test polynomial and the decode of one AddToAcc step.
// A new gate kind is threaded through here once.  Reference: OpenFHE binfhe-base-scheme.cpp EvalBinGate / BootstrapGateCore,
// rgsw-acc-cggi.cpp / rgsw-acc-dm.cpp EvalAcc.
#pragma once

// word j of a polynomial in LDS: four words of padding after every 64 (bank-conflict-free strided access)
__device__ __forceinline__ u32 phys(u32 j) { return j + ((j >> 6) << 2); }

// ---- key sets (include/bce_gpu.h, "key sets") ---------------------------------------------------------------------------
// The one way a body finds its keys: instance `inst` of a launch runs under set map[inst] when the launch carries a map, else
// under the selected set.  inst is uniform per workgroup; the map and the context's table are read through the constant
// address space (nothing writes them while a kernel runs), so the id and the three bases are scalar loads into SGPRs.
// a pointer into device memory that no kernel writes while this one runs, as a constant-address-space pointer (uniform
// loads through it are scalar).  The one cast; as_constant (dag_sched.hpp) adds what the persistent loop needs on top of it.
template <typename C, typename S>
__device__ __forceinline__ C* to_constant(const S* p) { return (C*)(uintptr_t)p; }
typedef const __attribute__((address_space(4))) KeySetDev ConstKeySetDev;
typedef const __attribute__((address_space(4))) u32 ConstMapWord;
template <typename PT>
__device__ __forceinline__ ConstKeySetDev& key_set(const PT& P, u32 inst) {
    const u32 k = __builtin_amdgcn_readfirstlane(inst);
    ConstMapWord* const map = to_constant<ConstMapWord>(P.keyset_map);
    const u32 id = map ? map[k] : P.keyset_sel;
    return to_constant<ConstKeySetDev>(P.keysets)[id];
}

// gate constant q1 of BootstrapGateCore (OR 5q/8, AND 7q/8, NOR q/8, NAND 3q/8)
__device__ __forceinline__ u32 gate_const(u32 op, u32 q) {
    const u32 e = q >> 3;
    switch (op) {
        case BCE_OR: case BCE_XOR_FAST: return 5 * e;
        case BCE_NOR: case BCE_XNOR_FAST: return e;
        case BCE_NAND: return 3 * e;
        default: return 7 * e;  // AND, REFRESH
    }
}

// ---- XOR in one bootstrap (BCE_XOR, include/bce_gpu.h) -----------------------------------------------------------------
// Level of its test polynomial at t = (b - j) mod q: +1 on [q/8, 3q/8), -1 on [5q/8, 7q/8), 0 elsewhere (times 2(Q/8 + 1)).
// The levels sit where every other gate's are, 0 and 2(Q/8 + 1), once the tail leaves its Q/8 + 1 out: tail_offset.
constexpr u32 kXorGate = BCE_XOR & 0xFFu;   // the gate byte of BCE_XOR (bit 16 of the word tells it from the bare code, on the host)
__device__ __forceinline__ int xor_level(u32 t, u32 q) {
    const u32 e = q >> 3;
    return (t >= e && t < 3 * e) ? 1 : (t >= 5 * e && t < 7 * e) ? -1 : 0;
}

// EvalBinGate's LWE preparation into av[0..n]: ct1 + ct2 with the folded EvalNOTs (-a, q/4 - b), 2(ct1 - ct2) for the fast
// XORs, ct + q/4 for a refresh (Bootstrap()).  T threads; the caller's barrier follows.  q (here and below): the body's own
// copy of P.q, read once at its top -- a second read behind a barrier is a second scalar load, held in another register.
template <u32 T, typename PT>
__device__ __forceinline__ void lwe_prepare(const PT& P, const bce_gate_desc& g, u32 soff, u32 q, u32* av, u32 tid) {
    const u32 op = g.op & 0xFFu;   // bits 8..15: the second gate of a pair (BCE_PAIR), the tail's business
    const u32 qm = q - 1, n = P.n;
    const u32* in0 = P.pool + (size_t)(g.in0 + soff) * P.pool_stride;
    const u32* in1 = P.pool + (size_t)(g.in1 + soff) * P.pool_stride;
    const bool two = op <= kXorGate;
    for (u32 i = tid; i <= n; i += T) {
        u32 v0 = in0[i];
        if (g.neg0) v0 = ((i == n ? (q >> 2) : 0u) - v0) & qm;
        u32 v = v0;
        if (two) {
            u32 v1 = in1[i];
            if (g.neg1) v1 = ((i == n ? (q >> 2) : 0u) - v1) & qm;
            v = (op == BCE_XOR_FAST || op == BCE_XNOR_FAST) ? (2u * (v0 - v1)) & qm : (v0 + v1) & qm;
        } else if (i == n) {
            v = (v0 + (q >> 2)) & qm;
        }
        av[i] = v;
    }
}

// The values a test polynomial takes, in a body's coefficient word W: pos = Q/8 + 1 and its negative, and for BCE_XOR twice
// those and 0.  u32, u64: residues mod Q (mod = Q); double: signed (mod = 0).
template <typename W>
struct GateLevels {
    W pos, neg, mod;
    __device__ __forceinline__ W pos2() const { return 2 * pos; }
    __device__ __forceinline__ W neg2() const { return mod - 2 * pos; }
};
template <typename W, typename PT>
__device__ __forceinline__ GateLevels<W> gate_levels(const PT& P, W mod) {
    const W pos = sizeof(W) == 4 ? (W)P.Q8p1 : (W)P.Q8p1_64;
    return {pos, mod - pos, mod};
}

// BootstrapGateCore: acc = (0, m(X)), m sparse (every 2N/q-th coefficient), b = av[n].  mod: see GateLevels; acc0, acc1: the
// two components in LDS (phys layout), N coefficients, T threads.
template <u32 T, u32 N, typename W, typename PT>
__device__ __forceinline__ void test_polynomial(const PT& P, u32 op, u32 q, u32 b, W mod, W* acc0, W* acc1, u32 tid) {
    const u32 qm = q - 1;
    const u32 q1 = gate_const(op, q), q2 = (q1 + (q >> 1)) & qm;
    const GateLevels<W> lv = gate_levels(P, mod);
    for (u32 j = tid; j < N; j += T) {
        W v = 0;
        if (j % P.factor == 0) {
            const u32 t = (b - j / P.factor) & qm;
            if (op == kXorGate) {
                const int l = xor_level(t, q);
                v = l > 0 ? lv.pos2() : l < 0 ? lv.neg2() : (W)0;
            } else {
                const bool in = (q1 < q2) ? (t >= q1 && t < q2) : !(t >= q2 && t < q1);
                v = in ? lv.neg : lv.pos;
            }
        }
        acc0[phys(j)] = 0;
        acc1[phys(j)] = v;
    }
}

// One AddToAcc step, from the prepared LWE coefficient a = av[i]; 0 where the step adds nothing.
// GINX (one step per coefficient): the exponent of the monomial, in [0, 2N); X^0 - 1 = 0.
template <typename PT>
__device__ __forceinline__ u32 ginx_exponent(const PT& P, u32 q, u32 a) { return ((q - a) & (q - 1)) * P.factor; }
// AP (one step per coefficient and digit): base-baseR digit k of -a, which selects the RGSW ciphertext
// (i * baseR + digit) * dR + k of the key; digit 0 is skipped (rgsw-acc-dm.cpp EvalAcc).
template <typename PT>
__device__ __forceinline__ u32 ap_digit(const PT& P, u32 q, u32 a, u32 k) {
    u32 aI = (q - a) & (q - 1);
    for (u32 t = 0; t < k; ++t) aI /= P.baseR;
    return aI % P.baseR;
}
