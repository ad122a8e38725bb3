// fused_tail.hpp -- the tail of EvalBinGate (included inside namespace bce by kernels.hip and kernels64.hip, after
// gate_front.hpp): transpose + sample extract, ModSwitch(Q -> qKS) (RoundqQ), LWE KeySwitch as a row gather,
// ModSwitch(qKS -> q) into the pool.  Its geometry and its three stages are defined once here, for the form fused into the
// blind-rotation kernels (fused_tail) and for the separate kernels (k_tail_gather / k_tail_finish, kernels.hip).
// Reference: OpenFHE binfhe-base-scheme.cpp EvalBinGate / lwe-pke.cpp ModSwitch, KeySwitch as called from
// src/gate.cpp:133,146,172,200-202.
#pragma once

// LWEEncryptionScheme::RoundqQ restated with the same three IEEE double operations
// (compiled with -ffp-contract=off): floor(0.5 + double(v) * double(q) / double(Q)) mod q
__device__ __forceinline__ u32 round_qQ(u64 v, u32 q, u64 Qfrom) {
    double t = (double)v * (double)q;
    t = t / (double)Qfrom;
    u64 r = (u64)floor(0.5 + t);
    return (u32)(r >= q ? r - q : r);
}

// what the tail adds to acc[1][0] before the switch to qKS (CW: the tail's coefficient word)
template <typename CW, typename PT>
__device__ __forceinline__ u64 tail_offset(const PT& P, u32 op) {
    if ((op & 0xFFu) == kXorGate) return 0;
    return sizeof(CW) == 8 ? (u64)P.Q8p1_64 : (u64)P.Q8p1;
}
// the modulus of the tail's coefficient words: u32 (Q < 2^28) or u64
template <typename CW, typename PT>
__device__ __forceinline__ u64 tail_modulus(const PT& P) { return sizeof(CW) == 8 ? (u64)P.Q64 : (u64)P.Q; }

// ---- two gates from one blind rotation (BCE_PAIR, include/bce_gpu.h) ---------------------------------------------
// BootstrapGateCore's test polynomial depends on the gate only through (b - q1) mod q, so the polynomial of gate op2 is
// X^e times that of gate op (mod X^N + 1), e = ((q1 - q1') mod q) * (2N / q), and the monomial commutes with the blind
// rotation: the second output of a pair is the tail applied to X^e * acc.  The rotation is an index and a sign on the
// tail's own reads of the accumulator.
// 1 + the code of the second gate of descriptor word `op`; 0: no pair (bit 16 is BCE_XOR's)
__device__ __forceinline__ u32 pair_second(u32 op) { return (op >> 8) & 0xFFu; }
// e in [0, 2N) for the second output of descriptor word `op`; 0 for its first output and for a plain descriptor.
template <typename PT>
__device__ __forceinline__ u32 pair_rotation(const PT& P, u32 op) {
    const u32 hi = pair_second(op);
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

// ---- geometry of the row gather ------------------------------------------------------------------------------------------
// A lane reads 16 bytes of a key-switching row per load: VW elements (8 u16 or 4 u32; the padded row stride keeps the last
// load in bounds).  G such groups hold elements 0..n, the vector pass covers Gv of them with RW waves per row, and the
// workgroup's waves form SL row slices that take rows slice, slice + SL, ...  Scratch in LDS: the row numbers (u32, padded
// to 16 bytes) and behind them [SL][Gv * VW] u64 partial sums.
struct TailGeom {
    u32 VW, G, Gv, RW, SL;
    __host__ __device__ constexpr TailGeom(u32 n, bool ksk_u16, u32 threads)
        : VW(ksk_u16 ? 8 : 4), G((n + VW) / VW), Gv(G < threads ? G : threads), RW((Gv + 63) / 64), SL(threads / 64 / RW) {}
    __host__ __device__ constexpr u32 red_words() const { return SL * Gv * VW; }
    // min_red: u64 words a caller needs behind the row numbers for a reduction of its own (k_tail_gather's scalar pass)
    __host__ __device__ constexpr size_t lds_bytes(size_t rows, size_t min_red = 0) const {
        return ((rows + 3) & ~(size_t)3) * sizeof(u32) + (red_words() > min_red ? red_words() : min_red) * sizeof(u64);
    }
    // The fused form serves a parameter set iff the vector pass holds every element (it has no scalar pass) and the scratch
    // for `rows` = N dKS row numbers fits the `avail` bytes its kernel has dead by then.  (Gv <= threads, so RW <= threads / 64
    // and SL >= 1 always.)
    static constexpr bool fused_fits(u32 n, bool ksk_u16, u32 threads, size_t rows, size_t avail) {
        const TailGeom t(n, ksk_u16, threads);
        return (size_t)n + 1 <= (size_t)threads * t.VW && t.lds_bytes(rows) <= avail;
    }
};
// n = 511, u16 rows, 512 threads, N = 1024, dKS = 5: 20,480 bytes of row numbers + 8 slices x 64 groups x 8 elements x 8 bytes
static_assert(TailGeom(511, true, 512).lds_bytes(1024 * 5) == 53248, "LDS rule of the fused tail");

// ---- the three stages ----------------------------------------------------------------------------------------------------
// coef: [2][N] coefficient-form accumulator (LDS or global); rot: the tail runs on X^rot * acc (pair_rotation; 0 = the
// accumulator itself); dbg_row: row of this output in the debug buffers (which may be null).
// Stage 1, coefficients i0 + ii for ii = tid, tid + stride, ... < ni.  Transpose (X -> X^-1) of acc[0]: a'_0 = a_0,
// a'_{N-i} = -a_i; ModSwitch(Q -> qKS); digits -> row numbers rowidx[ii * dKS + j] = (i * baseKS + digit_j) * dKS + j.
template <typename CW, typename PT>
__device__ __forceinline__ void tail_row_numbers(const PT& P, const CW* coef, u32 rot, u32 i0, u32 ni, u32 tid, u32 stride,
                                                 u32* rowidx, u32* __restrict__ dbg_lweN, u32 dbg_row) {
    const u32 N = P.N, qKS = P.qKS, B = P.baseKS, D = P.dKS;
    const u64 Q = tail_modulus<CW>(P);
    for (u32 ii = tid; ii < ni; ii += stride) {
        const u32 i = i0 + ii;
        const u64 v = rotated_coef(coef, i == 0 ? 0 : N - i, rot, N, Q, i != 0);
        u32 at = round_qQ(v, qKS, Q);
        if (dbg_lweN) dbg_lweN[(size_t)dbg_row * (N + 1) + i] = at;
        for (u32 j = 0; j < D; ++j) {
            rowidx[ii * D + j] = (i * B + at % B) * D + j;
            at /= B;
        }
    }
}

// Stage 2: red[slice][group * VW + e] = sum over the slice's rows of the LR in rowidx of K[row][group * VW + e].  U rows in
// flight per lane; u32 running sums are folded into the u64 totals every ks_chunk rows (ks_chunk * qKS <= 2^32: no wrap).
// ksk: the key-switching key of the bootstrap's key set (key_set, gate_front.hpp).
template <typename KT, u32 U, typename PT>
__device__ __forceinline__ void tail_gather_rows(const PT& P, const KT* __restrict__ ksk, const TailGeom& tg, u32 wave, u32 lane,
                                                 const u32* rowidx, u32 LR, u64* red) {
    constexpr u32 VW = 16 / sizeof(KT);
    const u32 Gv = tg.Gv, SL = tg.SL, slice = wave / tg.RW, group = (wave - slice * tg.RW) * 64 + lane;
    if (slice >= SL || group >= Gv) return;
    auto load_row = [&](u32 r) {
        const u32 row = __builtin_amdgcn_readfirstlane(rowidx[r]);
        return reinterpret_cast<const uint4*>(ksk + (size_t)row * P.ksk_stride)[group];
    };
    u64 tot[VW];
#pragma unroll
    for (u32 e = 0; e < VW; ++e) tot[e] = 0;
    const u32 CH = P.ks_chunk;
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
            for (u32 u = 0; u < U; ++u) v[u] = load_row(r + u * SL);
#pragma unroll
            for (u32 u = 0; u < U; ++u) add_row(v[u]);
        }
        for (; r < rend; r += SL) add_row(load_row(r));
#pragma unroll
        for (u32 e = 0; e < VW; ++e) tot[e] += run[e];
    }
#pragma unroll
    for (u32 e = 0; e < VW; ++e) red[(size_t)slice * Gv * VW + group * VW + e] = tot[e];
}
// element k of the vector pass, summed over the slices
__device__ __forceinline__ u64 tail_slice_sum(const TailGeom& tg, const u64* red, u32 k) {
    u64 sum = 0;
    for (u32 sl = 0; sl < tg.SL; ++sl) sum += red[(size_t)sl * tg.Gv * tg.VW + k];
    return sum;
}

// Stage 3, output word k given sum = sum_rows K[row][k].  KeySwitch: a' = -sum_rows A[row], b' = b - sum_rows B[row]
// (mod qKS), b = acc[1][0] + off (tail_offset) mod-switched; then ModSwitch(qKS -> q): the word of the pool.
template <typename CW, typename PT>
__device__ __forceinline__ u32 tail_finish_word(const PT& P, u64 sum, u32 k, const CW* coef, u32 rot, u64 off,
                                                u32* __restrict__ dbg_lweN, u32* __restrict__ dbg_ks, u32 dbg_row) {
    const u32 N = P.N, n = P.n, qKS = P.qKS;
    const u64 Q = tail_modulus<CW>(P);
    const u32 sm = (u32)(sum % qKS);
    u32 base = 0;
    if (k == n) {
        u64 b = rotated_coef(coef + N, 0, rot, N, Q, false) + off;
        b = b >= Q ? b - Q : b;
        base = round_qQ(b, qKS, Q);
        if (dbg_lweN) dbg_lweN[(size_t)dbg_row * (N + 1) + N] = base;
    }
    const u32 v = base >= sm ? base - sm : base + qKS - sm;
    if (dbg_ks) dbg_ks[(size_t)dbg_row * (n + 1) + k] = v;
    return round_qQ(v, P.q, qKS);
}

// ---- tail of EvalBinGate fused into the blind-rotation kernel (saturated launches) ------------------------------
// After the last inverse transform the workgroup that ran the blind rotation also extracts the LWE sample, switches it to
// qKS, gathers its N*dKS key-switching rows and writes the refreshed ciphertext: the stages above with one workgroup per
// bootstrap (S = 1), but the row gather -- memory-bound, 2 MB per bootstrap for STD128 -- runs while the CU's other
// workgroup keeps the vector ALUs busy, instead of as a separate kernel between two dependent blind-rotation launches.
//   coef : [2][N] coefficient-form accumulator in LDS        rowidx, red : TailGeom's scratch in LDS
// T threads (a multiple of 64); every thread of the workgroup must call it.
#ifndef BCE_FUSED_U
#define BCE_FUSED_U 8   // rows in flight per lane (tools/fused_u_sweep.sh)
#endif
template <typename KT, u32 T, typename CW, typename PT>
__device__ __forceinline__ void fused_tail(const PT& P, const KT* __restrict__ ksk, const CW* coef, u32* rowidx, u64* red, u32* out, u32 boot,
                                           u32* __restrict__ dbg_lweN, u32* __restrict__ dbg_ks, u64 off, u32 rot = 0) {
    const u32 N = P.N, n = P.n, tid = threadIdx.x, lane = tid & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    tail_row_numbers(P, coef, rot, 0u, N, tid, T, rowidx, dbg_lweN, boot);
    __syncthreads();
    const TailGeom tg(n, sizeof(KT) == 2, T);
    tail_gather_rows<KT, BCE_FUSED_U>(P, ksk, tg, wave, lane, rowidx, N * P.dKS, red);
    __syncthreads();
    for (u32 k = tid; k <= n; k += T)
        out[k] = tail_finish_word(P, tail_slice_sum(tg, red, k), k, coef, rot, off, dbg_lweN, dbg_ks, boot);
}
// The outputs of gate g from the coefficient-form accumulator `coef`: slot g.out, and for a pair descriptor (BCE_PAIR) the
// tail a second time, on X^e * acc, into slot out + 1 (debug rows: a second block of gridDim.x rows).  The pair branch is
// workgroup-uniform, its barrier frees rowidx / red.  PERSIST: the dataflow kernel runs the same pass
// (bce_dag_create_pairs) -- g came from D.tasks[t] through the constant address space, so the test is scalar, and both rows
// are stored before the worker's drain / barrier / release (dag_worker); its debug pointers are null and the row index
// stays `boot`.
template <u32 T, bool PERSIST, typename CW, typename PT>
__device__ __forceinline__ void fused_tail_outputs(const PT& P, const bce_gate_desc& g, u32 inst, u32 soff, const CW* coef, u32* rowidx,
                                                   u64* red, u32 boot, u32* __restrict__ dbg_lweN, u32* __restrict__ dbg_ks) {
    u32* outp = P.pool + (size_t)(g.out + soff) * P.pool_stride;
    const u64 off = tail_offset<CW>(P, g.op);
    const void* const ksk = key_set(P, inst).ksk;   // the instance's key set
    const uint16_t* const k16 = static_cast<const uint16_t*>(ksk);
    const u32* const k32 = static_cast<const u32*>(ksk);
    if (P.ksk_u16) fused_tail<uint16_t, T>(P, k16, coef, rowidx, red, outp, boot, dbg_lweN, dbg_ks, off);
    else fused_tail<u32, T>(P, k32, coef, rowidx, red, outp, boot, dbg_lweN, dbg_ks, off);
    if (pair_second(g.op)) {
        __syncthreads();
        const u32 e = pair_rotation(P, g.op), row = PERSIST ? boot : boot + gridDim.x;
        if (P.ksk_u16) fused_tail<uint16_t, T>(P, k16, coef, rowidx, red, outp + P.pool_stride, row, dbg_lweN, dbg_ks, off, e);
        else fused_tail<u32, T>(P, k32, coef, rowidx, red, outp + P.pool_stride, row, dbg_lweN, dbg_ks, off, e);
    }
}
