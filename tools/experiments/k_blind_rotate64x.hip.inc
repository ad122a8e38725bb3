// ARCHIVED EXPERIMENT (round 2) -- not compiled into the library.
// An all-16-wave re-cut of the STD192/AP blind rotation (drop into namespace bce::wd of csrc/kernels64.hip, launch with
// 1,024 threads and the LDS size of kernel_class64().lds_bytes).  Bit-exact at every stage
// (tests/test_gpu_engine.py::test_q64_custom_context_bit_exact_stages[...2048...AP] passed with it), and 17 % fewer
// shader cycles per step than the 8-wave kernel (27.6 k vs 33.3 k: inverse passes + digits 11.3 k -> 6.8 k, forward
// phase 13.2 k -> 7.5 k once the digit rows were re-padded and the twiddle blocks m >= 128 transposed), but only 5 %
// less TIME (26.7 ms vs 28.1 ms per 256-bootstrap launch): the clock the chip holds under the denser fp64 stream fell
// from 2.35 to 2.07 GHz.  The mixed 16-wave build that ships (k_blind_rotate64d, Body::Split16: 25.9 ms) is simpler and 3 %
// faster.  Touching the step's key rows early with dword loads to warm L2 made it 17 % slower (31.2 ms).
// =======================================================================================
// k_blind_rotate64x -- N = 2048, three gadget digits, AP/DM accumulator (BASELINE config 5): every phase on 16 waves
// =======================================================================================
// One workgroup of 1,024 threads (four waves per SIMD on the one workgroup a CU's LDS holds) per bootstrap.
// Thread (c, t) = (tid >> 9, tid & 511) owns the evaluation positions 4t .. 4t+3 of accumulator component c:
//   * MAC: the last forward stage (bit 0 pairs positions 2j, 2j+1) is applied to the digit rows on the fly, then
//     acc[c][4t+e] = sum_l dct[l][4t+e] * ek[l][c][4t+e]  (rgsw-acc-dm.cpp AddToAcc: the product REPLACES the
//     accumulator, so the evaluation-form accumulator is never stored) and the thread runs inverse pass 0 (bits 0, 1)
//     on its four fresh words;
//   * inverse passes 1..5 (bits 2-3, 4-5, 6-7, 8-9, 10): 4 coefficients per thread, two Gentleman-Sande stages per pass,
//     exchanged through two ping-pong LDS buffers (A = the accumulator's own rows, B = digit rows 0, 1, dead during the
//     inverse transform) in REGISTER-MAJOR layouts -- register r of thread t at r * stride + t: conflict-free stores --
//     whose row strides (513, 516, 528, 512, 512 doubles) make the next pass's reads conflict-free too;
//   * after pass 5 a thread holds coefficients t + 512 r (bits 10, 9 in registers): N^-1, SignedDigitDecompose and the
//     first two FORWARD stages on each digit in registers;
//   * forward stages on bits 8..5 and 4..1 as 12 half-transforms on waves 0..11 (forward_half_hi / _lo).
// No reduction inside the inverse transform (sums stay below 2^11 * 0.6 Q < 2^49), as in k_blind_rotate64d.
constexpr u32 XS0 = 513, XS1 = 516, XS2 = 528, XS3 = 512, XS4 = 512;

// Layouts private to this kernel.
//  * digit rows: 2 pad doubles per 32 (physx) -- with the usual 4 per 64 the pass on bits 4..1 (lanes = p[10:5], p[0])
//    hits every bank twice; with this padding its reads, the digit stores (lanes = consecutive t), the reads of the pass on
//    bits 8..5 (lanes = p[4:0]) and the 16-byte MAC reads at 4t are all conflict-free.
//  * LDS twiddle mirror: blocks m <= 64 in natural order; blocks m = 128, 256, 512 TRANSPOSED (entry (L << sh) | tt at
//    m + tt * 64 + L, sh = log2(m) - 6), because their readers hold the LOW index bits in registers and the high ones on
//    the lanes: natural order is a 2^sh-way bank conflict for them (the 32-bit kernels do the same, kernels.hip tw_pos).
__device__ __forceinline__ u32 physx(u32 j) { return j + ((j >> 5) << 1); }
template <u32 M>
__device__ __forceinline__ u32 twx(u32 idx) {   // position of natural entry M + idx in the mirror
    if constexpr (M < 128) {
        return M + idx;
    } else {
        constexpr u32 sh = (M == 128) ? 1 : (M == 256 ? 2 : 3);
        static_assert(M == 128 || M == 256 || M == 512, "mirror holds blocks up to 512");
        return M + ((idx & ((1u << sh) - 1u)) << 6) + (idx >> sh);
    }
}
// inverse twiddle of stage B for stage index i: -tw[(2m - 1) - i] (sign in the operand), from the mirror
template <int B>
__device__ __forceinline__ double2 itwx(const double2* twl, u32 i) {
    constexpr u32 m = 1u << (10 - B);
    return twl[twx<m>((m - 1) - i)];
}

// two Gentleman-Sande stages on 4 values whose register index is the 2-bit field (B+1, B) of the position:
// stage B pairs (0,1) [fa] and (2,3) [fb], stage B+1 pairs (0,2), (1,3) [fc]; inverse twiddle = -f, sign in the operand
__device__ __forceinline__ void inv_pass4d(double (&x)[4], double2 fa, double2 fb, double2 fc, double Q) {
    const double a0 = x[0] + x[1], a1 = modmul_q(x[1] - x[0], fa.x, fa.y, Q);
    const double a2 = x[2] + x[3], a3 = modmul_q(x[3] - x[2], fb.x, fb.y, Q);
    x[0] = a0 + a2; x[2] = modmul_q(a2 - a0, fc.x, fc.y, Q);
    x[1] = a1 + a3; x[3] = modmul_q(a3 - a1, fc.x, fc.y, Q);
}
// pass K = 1..4 (stages on bits 2K, 2K+1): reads the register-major image of pass K-1 (row stride SP), writes its own (SK)
template <int K, u32 SP, u32 SK>
__device__ __forceinline__ void inv_pass_x(const double* src, double* dst, const double2* twl, u32 t, double Q) {
    constexpr u32 sh = 2 * K, shp = 2 * (K - 1);
    const u32 G = t >> sh, L = t & ((1u << sh) - 1u);
    const u32 rs = (L >> shp) & 3u, lo = L & ((1u << shp) - 1u);
    double x[4];
#pragma unroll
    for (u32 r = 0; r < 4; ++r) x[r] = src[rs * SP + ((((G << 2) | r) << shp) | lo)];
    const double2 fa = itwx<2 * K>(twl, 2 * G), fb = itwx<2 * K>(twl, 2 * G + 1), fc = itwx<2 * K + 1>(twl, G);
    inv_pass4d(x, fa, fb, fc, Q);
#pragma unroll
    for (u32 r = 0; r < 4; ++r) dst[r * SK + t] = x[r];
}
// half of a forward transform, stages on bits 8..5: 128 virtual lanes v = (p[10:9] << 5) | p[4:0], registers = p[8:5]
__device__ __forceinline__ void forward_half_hi(double* poly, const double2* twl, u32 v, double Q) {
    const u32 hi = v >> 5, base = (hi << 9) | (v & 31u);
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = poly[physx(base | ((u32)r << 5))];
#pragma unroll
    for (int B = 8; B >= 5; --B) {
        const int rb = B - 5;
        const u32 m = 1u << (10 - B);   // 4 .. 32: natural order
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (r & (1 << rb)) continue;
            const double2 w = twl[m + ((hi << (8 - B)) | (u32)(r >> (rb + 1)))];
            const double X = x[r];
            const double Tm = modmul_q(x[r | (1 << rb)], w.x, w.y, Q);
            x[r] = X + Tm;
            x[r | (1 << rb)] = X - Tm;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) poly[physx(base | ((u32)r << 5))] = x[r];
}
// stages on bits 4..1: v = (p[10:5] << 1) | p[0], registers = p[4:1]; blocks m = 64 (natural), 128, 256, 512 (transposed)
template <int B>
__device__ __forceinline__ void fwd_lo_stage(double (&x)[16], const double2* twl, u32 hi, double Q) {
    constexpr int rb = B - 1;
    constexpr u32 m = 1u << (10 - B);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (r & (1 << rb)) continue;
        const double2 w = twl[twx<m>((hi << (4 - B)) | (u32)(r >> (rb + 1)))];
        const double X = x[r];
        const double Tm = modmul_q(x[r | (1 << rb)], w.x, w.y, Q);
        x[r] = X + Tm;
        x[r | (1 << rb)] = X - Tm;
    }
}
__device__ __forceinline__ void forward_half_lo(double* poly, const double2* twl, u32 v, double Q) {
    const u32 hi = v >> 1, base = (hi << 5) | (v & 1u);
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = poly[physx(base | ((u32)r << 1))];
    fwd_lo_stage<4>(x, twl, hi, Q);
    fwd_lo_stage<3>(x, twl, hi, Q);
    fwd_lo_stage<2>(x, twl, hi, Q);
    fwd_lo_stage<1>(x, twl, hi, Q);
#pragma unroll
    for (int r = 0; r < 16; ++r) poly[physx(base | ((u32)r << 1))] = x[r];
}

#ifndef BCE_X_PREFETCH
#define BCE_X_PREFETCH 0   // key rows (of 6) requested before the inverse passes; the rest at the start of the MAC
#endif
__global__ __launch_bounds__(1024) void k_blind_rotate64x(DevParams P, const bce_gate_desc* __restrict__ descs, u32 n_desc,
                                                         u32 slot_stride, u64* __restrict__ acc_out) {
    constexpr int LOGN = 11;
    using C = Cfg<LOGN>;
    constexpr int N = C::N, NP = C::NP;
    constexpr u32 R = 6, T = 1024;
    extern __shared__ __align__(16) double smemd[];
    double* bufA = smemd;            // [2][NP] exchange buffer A
    double* dct = bufA + 2 * NP;     // [R][NP]; rows 0, 1 are exchange buffer B during the inverse passes
    u32* av = reinterpret_cast<u32*>(dct + R * NP);
    const double2* __restrict__ tw = P.tw64d;
    double2* twl = reinterpret_cast<double2*>(av + ((P.n + 1 + 3) & ~3u));
    for (u32 i = threadIdx.x; i < 1024u; i += T) {   // mirror in this kernel's layout (twx)
        const u32 m = i < 2 ? 1u : (1u << (31 - __builtin_clz(i)));
        const u32 idx = i - m;
        u32 pos = i;
        if (m >= 128u) {
            const u32 sh = m == 128u ? 1u : (m == 256u ? 2u : 3u);
            pos = m + ((idx & ((1u << sh) - 1u)) << 6) + (idx >> sh);
        }
        twl[pos] = tw[i];
    }

    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 c = tid >> 9, t = tid & 511u;
    const double Q = P.Qd, invQ = P.invQd;
    const u32 q = P.q, qm = q - 1, n = P.n;
    const bce_gate_desc g = descs[blockIdx.x % n_desc];
    const u32 soff = (blockIdx.x / n_desc) * slot_stride;
    {   // EvalBinGate LWE prep with folded EvalNOT
        const u32* in0 = P.pool + (size_t)(g.in0 + soff) * P.pool_stride;
        const u32* in1 = P.pool + (size_t)(g.in1 + soff) * P.pool_stride;
        const bool two = g.op <= BCE_XNOR_FAST;
        for (u32 i = tid; i <= n; i += T) {
            u32 v0 = in0[i];
            if (g.neg0) v0 = ((i == n ? (q >> 2) : 0u) - v0) & qm;
            u32 v = v0;
            if (two) {
                u32 v1 = in1[i];
                if (g.neg1) v1 = ((i == n ? (q >> 2) : 0u) - v1) & qm;
                v = (g.op == BCE_XOR_FAST || g.op == BCE_XNOR_FAST) ? (2u * (v0 - v1)) & qm : (v0 + v1) & qm;
            } else if (i == n) {
                v = (v0 + (q >> 2)) & qm;
            }
            av[i] = v;
        }
    }
    __syncthreads();
    {   // BootstrapGateCore: acc = (0, NTT(m)); m is built and transformed in digit row 0 (scratch)
        const u32 b = av[n];
        const u32 q1 = gate_const(g.op, q), q2 = (q1 + (q >> 1)) & qm;
        const double pos = (double)P.Q8p1_64, neg = -pos;
        for (u32 j = tid; j < (u32)N; j += T) {
            double v = 0.0;
            if (j % P.factor == 0) {
                const u32 tt = (b - j / P.factor) & qm;
                const bool in = (q1 < q2) ? (tt >= q1 && tt < q2) : !(tt >= q2 && tt < q1);
                v = in ? neg : pos;
            }
            dct[phys(j)] = v;
        }
    }
    __syncthreads();
    if (wave == 0) ntt_forward_wave<LOGN>(dct, Tw{tw, nullptr}, lane, Q);
    __syncthreads();

    // step-invariant per-thread twiddles that live in the block the LDS mirror does not hold (m = 1024)
    const double2 w0a = tw[1024 + 2 * t], w0b = tw[1024 + 2 * t + 1];          // forward stage on bit 0, pairs (0,1), (2,3)
    const double2 f0a = tw[2047 - 2 * t], f0b = tw[2047 - (2 * t + 1)];        // inverse stage on bit 0
    const double2 f1 = tw[1023 - t];                                             // inverse stage on bit 1 (block m = 512)
    double* const A = bufA + c * NP;
    double* const B = dct + c * NP;
    {   // inverse pass 0 of the initial accumulator
        double a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = c ? modred(dct[phys(4 * t + e)], invQ, Q) : 0.0;
        __syncthreads();   // digit row 0 is exchange buffer B from here on
        inv_pass4d(a, f0a, f0b, f1, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) A[e * XS0 + t] = a[e];
    }
    block_sync_lds();

    const double2 ninv = make_double2(P.Ninvd, P.Ninvd_q);
    constexpr size_t rgsw = (size_t)R * 2 * N;
    const double* __restrict__ bsk = reinterpret_cast<const double*>(P.bsk64);
    const double dlo = -(double)((P.Q64 + 1) / 2), dhi = (double)((P.Q64 - 3) / 2);
    const double Bd = (double)(1u << P.gBits), invB = 1.0 / Bd, halfB = 0.5 * Bd;
    double doff = 0.0;
    {
        double pw = halfB;
        for (u32 l = 0; l < 3; ++l) { doff += pw; pw *= Bd; }
    }
    // passes 1..5 of the inverse transform: A holds pass 0's image; leaves coefficient (r << 9) | t in x[r], UNSCALED.
    // (t, A, B are passed in: inside the step loop they are derived from an opaque copy of the thread id, so that the ~60
    // step-invariant twiddles and addresses of the passes are NOT hoisted out of the loop and spilled)
    auto inverse_rest = [&](double (&x)[4], u32 tt, double* Ab, double* Bb) {
        inv_pass_x<1, XS0, XS1>(Ab, Bb, twl, tt, Q);
        block_sync_lds();
        inv_pass_x<2, XS1, XS2>(Bb, Ab, twl, tt, Q);
        block_sync_lds();
        inv_pass_x<3, XS2, XS3>(Ab, Bb, twl, tt, Q);
        block_sync_lds();
        inv_pass_x<4, XS3, XS4>(Bb, Ab, twl, tt, Q);
        block_sync_lds();
#pragma unroll
        for (u32 r = 0; r < 4; ++r) x[r] = Ab[((((r & 1u) << 1) | (tt >> 8)) * XS4) + (((r >> 1) << 8) | (tt & 255u))];
        const double2 f = itwx<10>(twl, 0);
#pragma unroll
        for (u32 r = 0; r < 2; ++r) {
            const double X = x[r], Y = x[r + 2];
            x[r] = X + Y;
            x[r + 2] = modmul_q(Y - X, f.x, f.y, Q);
        }
    };

    const u32 nsteps = n * P.dR;
    BCE_PROF_INIT();
    for (u32 step = 0; step < nsteps; ++step) {
        const u32 i = step / P.dR, k = step - i * P.dR;
        u32 aI = (q - av[i]) & qm;
        for (u32 tt = 0; tt < k; ++tt) aI /= P.baseR;
        const u32 a0 = aI % P.baseR;
        if (a0 == 0) continue;      // rgsw-acc-dm.cpp EvalAcc: digit 0 is skipped; A still holds pass 0 of the accumulator
        const double* bk = bsk + (((size_t)i * P.baseR + a0) * P.dR + k) * rgsw;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(bk), 0, (int)(rgsw * sizeof(double)), 0x00020000);
        u32 tid_v = tid;
        asm volatile("" : "+v"(tid_v));   // opaque per step: everything derived from it stays inside the step loop
        const u32 tv = tid_v & 511u, cv = tid_v >> 9, wv = tid_v >> 6, lv = tid_v & 63u;
        double* const Av = bufA + cv * NP;
        double* const Bv = dct + cv * NP;
        const u32 voff = (cv * N + 4u * tv) * 8u;
        double2 kb[R][2];
        auto request = [&](auto lo_c, auto hi_c) {
#pragma unroll
            for (u32 l = decltype(lo_c)::value; l < decltype(hi_c)::value; ++l) {
                kb[l][0] = key_row(rsrc, voff, l * (2 * N * 8));
                kb[l][1] = key_row(rsrc, voff + 16u, l * (2 * N * 8));
            }
        };
        constexpr u32 PRE = BCE_X_PREFETCH;
        request(std::integral_constant<u32, 0>{}, std::integral_constant<u32, PRE>{});
#ifndef BCE_X_NOTOUCH
        // The 128-register budget has no room for the step's 48 registers of key rows across the transforms (spills, see
        // profiles/r02_w16_sweep.log), so the rows are only TOUCHED here: one dword per row and thread (a wave covers the 16 cache
        // lines of its row segment), kept alive until the MAC, where the real 16-byte loads then hit L2 instead of HBM.
        u32 touch[R];
#pragma unroll
        for (u32 l = PRE; l < R; ++l) touch[l] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, l * (2 * N * 8), 0);
#endif
        {   // (1) inverse passes, N^-1, digits, forward stages on bits 10 and 9 -> dct[2l + c]
            double x[4], u[4];
            inverse_rest(x, tv, Av, Bv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double d = modmul_q(x[r], ninv.x, ninv.y, Q);
                d = d > dhi ? d - Q : d;
                d = d < dlo ? d + Q : d;
                u[r] = d + doff;
            }
            const double2 w10 = twl[1], w9a = twl[2], w9b = twl[3];
#pragma unroll
            for (u32 l = 0; l < 3; ++l) {
                double v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double fl = floor(u[r] * invB);
                    v[r] = fma(-fl, Bd, u[r]) - halfB;  // digit in [-B/2, B/2)
                    u[r] = fl;
                }
#pragma unroll
                for (int r = 0; r < 2; ++r) {  // bit 10: (r, r+2), twiddle tw[1]
                    const double Tm = modmul_q(v[r + 2], w10.x, w10.y, Q);
                    v[r + 2] = v[r] - Tm; v[r] = v[r] + Tm;
                }
                {   // bit 9: (0,1) with tw[2], (2,3) with tw[3]
                    const double T0 = modmul_q(v[1], w9a.x, w9a.y, Q);
                    v[1] = v[0] - T0; v[0] = v[0] + T0;
                    const double T1 = modmul_q(v[3], w9b.x, w9b.y, Q);
                    v[3] = v[2] - T1; v[2] = v[2] + T1;
                }
#pragma unroll
                for (u32 r = 0; r < 4; ++r) dct[(2 * l + cv) * NP + physx((r << 9) | tv)] = v[r];
            }
        }
        BCE_PROF_MARK(0);
        block_sync_lds();
        BCE_PROF_MARK(1);
        // (2) forward stages on bits 8..5 and 4..1: 12 half-transforms on waves 0..11
        if (wv < 12) forward_half_hi(dct + (wv % 6u) * NP, twl, (wv / 6u) * 64u + lv, Q);
        block_sync_lds();
        if (wv < 12) forward_half_lo(dct + (wv % 6u) * NP, twl, (wv / 6u) * 64u + lv, Q);
        BCE_PROF_MARK(2);
        block_sync_lds();
        BCE_PROF_MARK(3);
        // (3) forward stage on bit 0 on the fly, RGSW multiply-accumulate (replaces acc), inverse pass 0 -> A
#ifndef BCE_X_NOTOUCH
#pragma unroll
        for (u32 l = PRE; l < R; ++l) asm volatile("" ::"v"(touch[l]));
#endif
        request(std::integral_constant<u32, PRE>{}, std::integral_constant<u32, R>{});
        {
            double sp[4] = {0.0, 0.0, 0.0, 0.0};
            const u32 pp = physx(4u * tv);
#pragma unroll
            for (u32 l = 0; l < R; ++l) {
                const double2 d01 = *reinterpret_cast<const double2*>(dct + l * NP + pp);
                const double2 d23 = *reinterpret_cast<const double2*>(dct + l * NP + pp + 2);
                const double T0 = modmul_q(d01.y, w0a.x, w0a.y, Q), T1 = modmul_q(d23.y, w0b.x, w0b.y, Q);
                sp[0] += modmul(d01.x + T0, kb[l][0].x, invQ, Q);
                sp[1] += modmul(d01.x - T0, kb[l][0].y, invQ, Q);
                sp[2] += modmul(d23.x + T1, kb[l][1].x, invQ, Q);
                sp[3] += modmul(d23.x - T1, kb[l][1].y, invQ, Q);
            }
            double a[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = modred(sp[e], invQ, Q);
            inv_pass4d(a, f0a, f0b, f1, Q);
#pragma unroll
            for (int e = 0; e < 4; ++e) Av[e * XS0 + tv] = a[e];
        }
        BCE_PROF_MARK(4);
        block_sync_lds();
        BCE_PROF_MARK(5);
    }
    {   // accumulator back to COEFFICIENT form (its pass 0 is already in A)
        double x[4];
        inverse_rest(x, t, A, B);
        u64* out = acc_out + ((size_t)blockIdx.x * 2 + c) * N;
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
            const double y = modmul_q(x[r], ninv.x, ninv.y, Q);
            const double v = y < 0.0 ? y + Q : y;
            const double hi = floor(v * (1.0 / 4294967296.0));
            out[(r << 9) | t] = ((u64)(u32)hi << 32) | (u64)(u32)fma(-hi, 4294967296.0, v);
        }
    }
}

