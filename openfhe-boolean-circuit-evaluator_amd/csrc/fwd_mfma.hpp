// fwd_mfma.hpp -- host-only tables of the matrix-pipe body of the forward transforms (kernels.hip, ntt_forward_quarter3<true>).
//
// In the merged Cooley-Tukey order of this engine (tw[m + i] = psi^brv(m + i), the stage on position bit B uses
// tw[2^(9-B) + (p >> (B + 1))]) the twiddle of a butterfly of the six stages on bits 9..4 of an N = 1024 transform does not
// depend on the low four position bits.  Viewing a digit row as X[h = p >> 4][j = p & 15], those stages are therefore ONE
// 64 x 64 matrix applied to each of the 16 columns:  Y[h'][j] = sum_h M6[h'][h] X[h][j]  (mod Q).
// X holds the signed gadget digits s = d - 2^(gBits-1) in [-2^(gBits-1), 2^(gBits-1)) (the transform's input), M6's entries are
// split into four 7-bit limbs, and the four limb products S_i = limb_i(M6) X are exact i8 x i8 -> i32 matrix products
// (v_mfma_i32_16x16x64_i8, signed operands):
//     Y = S0 + 2^7 S1 + 2^14 (S2 + 2^7 S3)  (mod Q).
// (With the raw digits d as the operand the same holds after adding C[h'] = -2^(gBits-1) sum_h M6[h'][h] mod Q; the tables keep
// C for the test that ties the two forms together.  The kernel uses the signed form: no per-row constant at all.)
// Nothing here needs a device: a CPU test checks the tables against a plain model of the six stages.
#pragma once
#include <cstdint>
#include <vector>

#include "host_math.hpp"

namespace bce {

constexpr u32 kFwdMfmaLoads = 4;                              // 16-byte loads per lane and step: the A operands of four tiles
constexpr u32 kFwdMfmaTableWords = 4 * kFwdMfmaLoads * 64 * 4;  // [quarter][tile][lane][4 words] = 16 KiB

// position h (bits 9..4 of a coefficient index) of the K slot k = 16 (lane >> 4) + byte of the B operand: the thread that
// holds coefficients t + 256 r (r = 0..3) stores its four digits as ONE dword at bytes 4 (t >> 4) + r of column t & 15
inline u32 fwd_mfma_h_of_k(u32 k) { return (k >> 2) + 16u * (k & 3u); }

struct FwdMfmaTables {
    bool ok = false;              // the arithmetic conditions below hold (the engine adds: folded key, GINX, even factor)
    u64 psi = 0;
    std::vector<u32> M6;          // [h'][h], entries in [0, Q)
    std::vector<u32> C;           // [h'] balance words of the raw-digit form (not used by the kernel)
    std::vector<u32> table;       // device image, kFwdMfmaTableWords
    u32 w14 = 0, w14s = 0;        // 2^14 mod Q and its Shoup companion
    u64 limb_sum_max = 0;         // bound of |one limb sum|: 64 * 127 * 2^(gBits-1)
    u64 lo_max = 0, hi_max = 0, out_max = 0;   // bounds of Q + S0 + 2^7 S1, of Q + S2 + 2^7 S3, and of the recombined word
};

// Conditions (all on the host, before the body is selected):
//   N = 1024, dG = 4, gBits <= 7 (signed digits and 7-bit limbs fit an i8), Q < 2^28 (four 7-bit limbs);
//   |limb sums|  <= L = 64 * 127 * 2^(gBits-1) <= 64 * 127 * 127 < 2^31          (exact in the i32 accumulator)
//   |S0 + 2^7 S1|, |S2 + 2^7 S3| <= 129 L < Q: the accumulators start at (Q, 0, Q, 0), so that
//   lo = Q + S0 + 2^7 S1 and hi = Q + S2 + 2^7 S3 lie in (0, Q + 129 L] and fit 32 bits;
//   word = lazy Shoup product hi * 2^14 (in [0, 2Q) for ANY 32-bit hi) + lo  < 2Q + lo_max, which must not exceed 13 Q: the
//   bound with which six lazy radix-2 stages (each adds < 2Q to inputs < Q) leave the same positions today.  The remaining
//   four stages and the MAC then see words no larger than before, so ok1..ok5 of the lazy transform cover this body as well.
inline FwdMfmaTables build_fwd_mfma_tables(u64 Q, u32 N, u32 gBits, u32 dG, u64 psi = 0) {
    FwdMfmaTables T;
    if (N != 1024 || dG != 4 || gBits == 0 || gBits > 7 || Q >= (1ull << 28) || Q < 3 || (Q - 1) % (2ull * N) != 0) return T;
    T.psi = psi ? psi : min_primitive_root(Q, 2ull * N);
    if (pow_mod(T.psi, N, Q) != Q - 1) return T;
    // natural-index forward twiddles of the blocks m = 1..32
    std::vector<u64> tw(64, 0);
    for (u32 i = 0; i < 64; ++i) tw[i] = pow_mod(T.psi, bit_reverse(i, 10), Q);
    T.M6.assign(64 * 64, 0);
    for (u32 e = 0; e < 64; ++e) {          // column e of M6 = the six stages applied to the unit vector e
        u64 x[64] = {0};
        x[e] = 1;
        for (int B = 5; B >= 0; --B) {      // bit B of h = position bit B + 4; block m = 2^(5 - B), twiddle index h >> (B + 1)
            const u32 m = 1u << (5 - B);
            for (u32 h = 0; h < 64; ++h) {
                if (h & (1u << B)) continue;
                const u64 w = tw[m + (h >> (B + 1))];
                const u64 X = x[h], Tm = mul_mod(x[h | (1u << B)], w, Q);
                x[h] = (X + Tm) % Q;
                x[h | (1u << B)] = (X + Q - Tm) % Q;
            }
        }
        for (u32 h = 0; h < 64; ++h) T.M6[h * 64 + e] = (u32)x[h];
    }
    T.C.assign(64, 0);
    for (u32 hp = 0; hp < 64; ++hp) {
        u64 s = 0;
        for (u32 h = 0; h < 64; ++h) s = (s + T.M6[hp * 64 + h]) % Q;
        T.C[hp] = (u32)((Q - mul_mod(s, 1ull << (gBits - 1), Q)) % Q);
    }
    const u64 w14 = (1ull << 14) % Q;
    T.w14 = (u32)w14;
    T.w14s = (u32)(((u128)w14 << 32) / Q);
    T.limb_sum_max = 64ull * 127ull * (1ull << (gBits - 1));
    T.hi_max = Q + 129ull * T.limb_sum_max;
    T.lo_max = T.hi_max;
    T.out_max = 2 * Q + T.lo_max;
    T.ok = T.limb_sum_max < (1ull << 31) && 129ull * T.limb_sum_max < Q && T.lo_max < (1ull << 32) && T.out_max <= 13 * Q;
    // device image: quarter q (output rows h' = 16 q ..), tile v, lane l: the A operand of tile v -- row l & 15 of the
    // tile = (o = (l & 15) >> 2, limb = l & 3) of output row h' = 16 q + 4 v + o, K slots 16 (l >> 4) + (0..15), one byte each;
    // a lane's four accumulator registers (rows 4 (l >> 4) + reg) are then the four limbs of ONE output word.
    T.table.assign(kFwdMfmaTableWords, 0);
    for (u32 q = 0; q < 4; ++q)
        for (u32 l = 0; l < 64; ++l) {
            for (u32 v = 0; v < 4; ++v) {
                const u32 hp = 16 * q + 4 * v + ((l & 15u) >> 2), limb = l & 3u;
                for (u32 b = 0; b < 16; ++b) {
                    const u32 byte = (T.M6[hp * 64 + fwd_mfma_h_of_k(16 * (l >> 4) + b)] >> (7 * limb)) & 127u;
                    T.table[((q * kFwdMfmaLoads + v) * 64 + l) * 4 + (b >> 2)] |= byte << (8 * (b & 3u));
                }
            }
        }
    return T;
}

}  // namespace bce
