// fused_tail.hpp -- the tail of EvalBinGate run by the workgroup that finished the blind rotation (included inside
// namespace bce by kernels.hip and kernels64.hip): transpose + sample extract, ModSwitch(Q -> qKS) (RoundqQ), LWE
// KeySwitch as a row gather, ModSwitch(qKS -> q) into the pool.  Reference: OpenFHE binfhe-base-scheme.cpp EvalBinGate /
// lwe-pke.cpp ModSwitch, KeySwitch as called from src/gate.cpp:133,146,172,200-202.
#pragma once

// LWEEncryptionScheme::RoundqQ restated with the same three IEEE double operations
// (compiled with -ffp-contract=off): floor(0.5 + double(v) * double(q) / double(Q)) mod q
__device__ __forceinline__ u32 round_qQ(u64 v, u32 q, u64 Qfrom) {
    double t = (double)v * (double)q;
    t = t / (double)Qfrom;
    u64 r = (u64)floor(0.5 + t);
    return (u32)(r >= q ? r - q : r);
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
// what the tail adds to acc[1][0] before the switch to qKS (CW: the tail's coefficient word)
template <typename CW, typename PT>
__device__ __forceinline__ u64 tail_offset(const PT& P, u32 op) {
    if ((op & 0xFFu) == kXorGate) return 0;
    return sizeof(CW) == 8 ? (u64)P.Q8p1_64 : (u64)P.Q8p1;
}

// ---- two gates from one blind rotation (BCE_PAIR, include/bce_gpu.h) ---------------------------------------------
// BootstrapGateCore's test polynomial depends on the gate only through (b - q1) mod q, so the polynomial of gate op2 is
// X^e times that of gate op (mod X^N + 1), e = ((q1 - q1') mod q) * (2N / q), and the monomial commutes with the blind
// rotation: the second output of a pair is the tail applied to X^e * acc.  The rotation is an index and a sign on the
// tail's own reads of the accumulator.
// e in [0, 2N) for the second output of descriptor word `op`; 0 for its first output and for a plain descriptor.
template <typename PT>
__device__ __forceinline__ u32 pair_rotation(const PT& P, u32 op) {
    const u32 hi = (op >> 8) & 0xFFu;
    if (hi == 0) return 0;
    return ((gate_const(op & 0xFFu, P.q) - gate_const(hi - 1, P.q)) & (P.q - 1)) * P.factor;
}
// coefficient i of X^e * p (p: N words below Q): s p[i - e'] for i >= e', -s p[N + i - e'] below, e' = e mod N, s = -1 iff e >= N;
// `flip` negates once more (the transpose of the sample extraction)
template <typename CW>
__device__ __forceinline__ u64 rotated_coef(const CW* p, u32 i, u32 e, u32 N, u64 Q, bool flip) {
    const u32 es = e & (N - 1);
    const bool wrap = i < es;
    const u64 src = p[wrap ? N + i - es : i - es];
    const bool neg = (wrap != (e >= N)) != flip;
    return neg ? (src ? Q - src : 0) : src;
}

// ---- tail of EvalBinGate fused into the blind-rotation kernel (saturated launches) ------------------------------
// After the last inverse transform the workgroup that ran the blind rotation also extracts the LWE sample,
// switches it to qKS, gathers its N*dKS key-switching rows and writes the refreshed ciphertext: the same arithmetic
// as k_tail_gather / k_tail_finish below (one workgroup per bootstrap, S = 1), but its row gather -- memory-bound,
// 2 MB per bootstrap for STD128 -- runs while the CU's other workgroup keeps the vector ALUs busy, instead of as a
// separate kernel between two dependent blind-rotation launches.
//   coef : [2][N] coefficient-form accumulator in LDS        rowidx : [N * dKS] row numbers in LDS
//   red  : [SL][Gv * VW] u64 partial sums in LDS (SL row slices, one per RW = ceil(Gv / 64) waves)
//   off  : added to acc[1][0] (tail_offset)
//   rot  : the tail runs on X^rot * acc (pair_rotation; 0 = the accumulator itself)
// T threads (a multiple of 64); every thread of the workgroup must call it.
template <typename KT, u32 T, typename CW, typename PT>
__device__ __forceinline__ void fused_tail(const PT& P, const CW* coef, u32* rowidx, u64* red, u32* out, u32 boot,
                                           u32* __restrict__ dbg_lweN, u32* __restrict__ dbg_ks, u64 off, u32 rot = 0) {
    constexpr u32 VW = 16 / sizeof(KT), W = T / 64;
    const u32 N = P.N, n = P.n, qKS = P.qKS, B = P.baseKS, D = P.dKS;
    const u64 Q = sizeof(CW) == 8 ? (u64)P.Q64 : (u64)P.Q;            // coefficient words: u32 (Q < 2^28) or u64
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // transpose (X -> X^-1) of acc[0]: a'_0 = a_0, a'_{N-i} = -a_i; ModSwitch(Q -> qKS); digits -> row numbers
    for (u32 i = tid; i < N; i += T) {
        const u64 v = rotated_coef(coef, i == 0 ? 0 : N - i, rot, N, Q, i != 0);
        u32 at = round_qQ(v, qKS, Q);
        if (dbg_lweN) dbg_lweN[(size_t)boot * (N + 1) + i] = at;
        for (u32 j = 0; j < D; ++j) {
            rowidx[i * D + j] = (i * B + at % B) * D + j;
            at /= B;
        }
    }
    __syncthreads();
    const KT* __restrict__ ksk = reinterpret_cast<const KT*>(P.ksk);
    const u32 G = (n + VW) / VW;                  // 16-byte groups holding elements 0..n
    const u32 Gv = G < T ? G : T;                 // (n + 1 <= T * VW for every parameter set this kernel serves)
    const u32 RW = (Gv + 63) / 64, SL = W / RW;   // waves per row, row slices
    const u32 slice = wave / RW, group = (wave - slice * RW) * 64 + lane;
    const u32 LR = N * D;
    if (slice < SL && group < Gv) {
        u64 tot[VW];
#pragma unroll
        for (u32 e = 0; e < VW; ++e) tot[e] = 0;
        const u32 CH = P.ks_chunk;                // rows whose elements can be summed in 32 bits
#ifndef BCE_FUSED_U
#define BCE_FUSED_U 8
#endif
        constexpr u32 U = BCE_FUSED_U;            // rows in flight per lane
        u32 r = slice;
        while (r < LR) {
            u32 run[VW];
#pragma unroll
            for (u32 e = 0; e < VW; ++e) run[e] = 0;
            const u32 rend = (LR - r > CH * SL) ? r + CH * SL : LR;
            auto add_row = [&](uint4 v) {
                if constexpr (sizeof(KT) == 2) {
                    run[0] += v.x & 0xFFFFu; run[1] += v.x >> 16; run[2] += v.y & 0xFFFFu; run[3] += v.y >> 16;
                    run[4] += v.z & 0xFFFFu; run[5] += v.z >> 16; run[6] += v.w & 0xFFFFu; run[7] += v.w >> 16;
                } else {
                    run[0] += v.x; run[1] += v.y; run[2] += v.z; run[3] += v.w;
                }
            };
            for (; r + (U - 1) * SL < rend; r += U * SL) {
                uint4 v[U];
#pragma unroll
                for (u32 u = 0; u < U; ++u) {
                    const u32 row = __builtin_amdgcn_readfirstlane(rowidx[r + u * SL]);
                    v[u] = reinterpret_cast<const uint4*>(ksk + (size_t)row * P.ksk_stride)[group];
                }
#pragma unroll
                for (u32 u = 0; u < U; ++u) add_row(v[u]);
            }
            for (; r < rend; r += SL) {
                const u32 row = __builtin_amdgcn_readfirstlane(rowidx[r]);
                add_row(reinterpret_cast<const uint4*>(ksk + (size_t)row * P.ksk_stride)[group]);
            }
#pragma unroll
            for (u32 e = 0; e < VW; ++e) tot[e] += run[e];
        }
#pragma unroll
        for (u32 e = 0; e < VW; ++e) red[(size_t)slice * Gv * VW + group * VW + e] = tot[e];
    }
    __syncthreads();
    // KeySwitch: a' = -sum_rows A[row], b' = b - sum_rows B[row] (mod qKS), b = acc[1][0] + off (Q/8 + 1; BCE_XOR: 0) mod-switched;
    // then ModSwitch(qKS -> q) into the pool
    for (u32 k = tid; k <= n; k += T) {
        u64 sum = 0;
        for (u32 sl = 0; sl < SL; ++sl) sum += red[(size_t)sl * Gv * VW + k];
        const u32 sm = (u32)(sum % qKS);
        u32 base = 0;
        if (k == n) {
            u64 b = rotated_coef(coef + N, 0, rot, N, Q, false) + off;
            b = b >= Q ? b - Q : b;
            base = round_qQ(b, qKS, Q);
            if (dbg_lweN) dbg_lweN[(size_t)boot * (N + 1) + N] = base;
        }
        const u32 v = base >= sm ? base - sm : base + qKS - sm;
        if (dbg_ks) dbg_ks[(size_t)boot * (n + 1) + k] = v;
        out[k] = round_qQ(v, P.q, qKS);
    }
}

