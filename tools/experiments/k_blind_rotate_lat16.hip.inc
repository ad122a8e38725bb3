// ARCHIVED EXPERIMENT (round 2) -- not part of the build.  16-wave (1,024-thread) build of the split-transform kernel for
// launches that leave every workgroup a CU of its own; drops into csrc/kernels.hip before fused_tail_fits(), launcher
// fragment at the end of this file.  Bit-exact (tests/test_gpu_engine.py::test_std128_every_blind_rotation_kernel_bit_exact
// with BCE_VARIANT=4 passed), but SLOWER than the 8-wave build: 2.41 ms vs 1.87 ms per lone bootstrap
// (profiles/r02_lat16_experiment.log).  Per-wave phase counters of the same log say why: (1) the 128 one-KiB key-row
// requests of a step, issued at its top by 16 waves, queue on the CU's L1 fill path (128 KiB per step at 64 B/clk =
// 2 k cycles): the youngest waves spend 3.4 k cycles per step just ISSUING them and the inverse waves 0.6..1.4 k;
// (2) the forward phase takes the same 3.6 k cycles with three half-row transforms per SIMD as with a whole + a half
// row on two waves -- it is not bound by how many waves issue, but by the LDS traffic of the transforms (data +
// twiddles: ~190 KiB per step, half of it twiddles, a quarter of the LDS cycles bank conflicts); (3) the lane-pair MAC
// reads every digit row twice.  The issue-rate model that predicted -17 % (4.4 cycles per wave-instruction with four
// waves per SIMD) does not describe a lone workgroup.
// ---- 16-wave build of the split-transform kernel for launches that leave every workgroup a CU of its own ----------
// A lone 512-thread workgroup runs two waves per SIMD, and two waves cannot keep a SIMD issuing: its forward phase
// and its MAC run at 5.5..7 cycles per wave-instruction where four resident waves reach 4.4 (profiles/
// r02_fold_phase_per_wave.log).  This build gives the one bootstrap of a CU 1,024 threads (GINX, folded key only):
//   * inverse transforms: unchanged, on waves 0..7 (4 coefficients per thread is what keeps them at 5 radix-4 passes);
//     pass 0 runs there as well (it cannot ride on the MAC thread, which is a different thread here);
//   * forward phase: the six digit rows as 12 half-row transforms on waves 0..11 (three per SIMD);
//   * MAC: every item (component, 4 consecutive positions) on a PAIR of adjacent lanes -- the even lane sums the rows
//     against key+, the odd lane against key-; each multiplies its sum by its own monomial, the odd lane's product
//     crosses to the even lane with one DPP quad permutation per word, and the even lane writes the accumulator.
// Four workgroup barriers per step (after the MAC as well: the inverse threads read words other waves wrote).
// Same accumulator words as every other kernel (exact arithmetic mod Q, canonical output).
__global__ __launch_bounds__(1024) void k_blind_rotate_lat16(DevParams P, const bce_gate_desc* __restrict__ descs, u32 n_desc,
                                                            u32 slot_stride, u32* __restrict__ acc_out, u32* __restrict__,
                                                            u32* __restrict__) {
    constexpr int LOGN = 10, DG = 4;
    using C = Cfg<LOGN>;
    constexpr int N = C::N, NP = C::NP;
    constexpr u32 R = 2 * DG, T = 1024, XB = 1280;
    extern __shared__ __align__(16) u32 smem[];
    uint2* twf = reinterpret_cast<uint2*>(smem);
    u32* acc = reinterpret_cast<u32*>(twf + N);  // [2][NP]
    u32* dct = acc + 2 * NP;                     // [R][NP]: rows 0, 1 = second accumulator buffer, rows 2..7 = digits
    u32* xab = dct + R * NP;                     // [2 polynomials][2 buffers][XB]
    u32* av = xab + 4 * XB;

    const u32 tid = threadIdx.x;
    const u32 lane = tid & 63;
    const u32 wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const u32 Q = P.Q, q = P.q, qm = q - 1, n = P.n;
    const bce_gate_desc g = descs[blockIdx.x % n_desc];
    const u32 soff = (blockIdx.x / n_desc) * slot_stride;
    bootstrap_prologue<LOGN, true, T>(P, g, soff, twf, acc, av, tid, lane, wave);

    const bool inv = wave < 8;                   // wave-uniform: the inverse-transform half of the workgroup
    const u32 c = (wave >> 2) & 1u;              // inverse-transform group = accumulator component
    SplitInv<false> S;
    split_inv_setup(S, twf, tid & 255u);
    u32* const xa = xab + c * 2 * XB;
    u32* const xb = xa + XB;
    const uint2 ninv = make_uint2(P.Ninv, P.Ninv_s), wlast = make_uint2(P.Winv_last, P.Winv_last_s);
    constexpr u32 rgsw = R * 2 * N;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(P.bsk), 0, (int)(n * 2 * rgsw * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t psi_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(P.psi_tab), 0, N * 4, 0x00020000);
    const u32 gb = P.gBits, Qh = Q >> 1;
    u32 off = 0;
    for (u32 l = 0; l < (u32)DG; ++l) off |= 1u << (l * gb + gb - 1);
    const u32 offm = off - Q, bias = Q - (1u << (gb - 1));
    // MAC item of this lane pair: component mc, positions mp0..mp0+3; key+ on the even lane, key- on the odd one
    const u32 item = tid >> 1, mkey = tid & 1u;
    const u32 mc = item >> 8, mp0 = (item & 255u) * 4, mpp = phys(mp0);
    const u32 kvoff = item * 16u + mkey * (rgsw * 4u);   // byte offset of this lane's 16 bytes inside a row of its key
    const u32 dig0 = phys(S.t);
    const uint2 w9 = twf[1], w8a = twf[2], w8b = twf[3];

    BCE_PROF_INIT();
    u32 cb = 0;   // word offset (from `acc`) of the accumulator buffer the step reads; it writes the other one
    for (u32 step = 0; step < n; ++step) {
        const u32 ap = ((q - av[step]) & qm) * P.factor;
        if (ap == 0) continue;
        const u32 rowb = step * (2 * rgsw * 4);
        uint4 kr[R];
#pragma unroll
        for (u32 l = 0; l < R; ++l) kr[l] = bsk_row(rsrc, kvoff, rowb + l * (2 * N * 4));
        BCE_PROF_MARK(8);
        // (1) waves 0..7: inverse transform (passes 0..4), digits 1..3 with their first two forward stages -> dct rows 2..7
        if (inv) {
            u32 x[4], u[4];
            {
                const uint4 v = *reinterpret_cast<const uint4*>(acc + cb + c * NP + S.a0);
                u32 a[4] = {v.x, v.y, v.z, v.w};
                split_pass0(S, twf, a, xa, Q, P.mu32);
            }
            split_inverse_rest(S, twf, xa, xb, Q, P.mu32, ninv, wlast, x, [](auto) {});
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = x[r] + ((x[r] < Qh) ? off : offm);
#pragma unroll
            for (u32 l = 1; l < (u32)DG; ++l) {
                u32 v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = __builtin_amdgcn_ubfe(u[r], l * gb, gb) + bias;
                fwd_bfly(v[0], v[2], w9, Q);
                fwd_bfly(v[1], v[3], w9, Q);
                fwd_bfly(v[0], v[1], w8a, Q);
                fwd_bfly(v[2], v[3], w8b, Q);
#pragma unroll
                for (int r = 0; r < 4; ++r) dct[(2 * l + c) * NP + dig0 + 272 * r] = v[r];
            }
        } else {
            block_sync_lds();   // the barrier inside split_inverse_rest
        }
        BCE_PROF_MARK(0);
        block_sync_lds();
        BCE_PROF_MARK(1);
        // (2) twelve half-row transforms on waves 0..11
        if (wave < 12) ntt_forward_half_low8(dct + (2 + wave % 6u) * NP, wave / 6u, twf, lane, Q);
        BCE_PROF_MARK(2);
        block_sync_lds();
        BCE_PROF_MARK(3);
        // (3) MAC on lane pairs
        {
            u64 sm[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 l = 0; l < R; ++l) {
                const uint4 d = *reinterpret_cast<const uint4*>((l < 2 ? acc + cb : dct) + l * NP + mpp);
                sm[0] += (u64)d.x * kr[l].x; sm[1] += (u64)d.y * kr[l].y; sm[2] += (u64)d.z * kr[l].z; sm[3] += (u64)d.w * kr[l].w;
            }
            // this lane's monomials psi^(+-(2k+1)a') - 1 at its 4 positions (see ginx_mac_tail)
            const bool odd = ap & 1u;
            const u32 a4 = ap & 3u;
            const u32 a4k = mkey ? (4u - a4) & 3u : a4;
            const uint2 Ik = make_uint2(a4k == 0 ? P.I4[0] : a4k == 1 ? P.I4[1] : a4k == 2 ? P.I4[2] : P.I4[3],
                                        a4k == 0 ? P.I4s[0] : a4k == 1 ? P.I4s[1] : a4k == 2 ? P.I4s[2] : P.I4s[3]);
            const u32 k0 = __brev(mp0) >> (32 - LOGN);
            const u32 ex = ((2 * k0 + 1) * ap) & (2 * N - 1);
            u32 m[4];
            m[0] = psi_pow<LOGN>(psi_rsrc, mkey ? (2 * N - ex) & (2 * N - 1) : ex, Q);
            m[2] = csub(mul_shoup_lazy(m[0], Ik, Q), Q);
            m[1] = odd ? Q - m[0] : m[0];
            m[3] = odd ? Q - m[2] : m[2];
            const uint4 a4v = *reinterpret_cast<const uint4*>(acc + cb + mc * NP + mpp);
            const u32 aold[4] = {a4v.x, a4v.y, a4v.z, a4v.w};
            u32 anew[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u32 r = barrett_lazy3((u64)(u32)(sm[e] >> 32) * P.c32 + (u32)sm[e], Q, P.red_shift, P.red_mu);       // < 3Q
                const u32 t = barrett_lazy3((u64)r * (m[e] - 1) + (mkey ? 0u : aold[e]), Q, P.red_shift, P.red_mu);      // < 3Q
                const u32 o = (u32)__builtin_amdgcn_mov_dpp((int)t, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]: the partner lane's word
                const u32 sum = t + o;                                                         // < 6Q
                anew[e] = sum - __umulhi(sum, P.mu32) * Q;                                     // [0, 2Q)
            }
            if (!mkey) *reinterpret_cast<uint4*>(acc + (2 * NP - cb) + mc * NP + mpp) = make_uint4(anew[0], anew[1], anew[2], anew[3]);
            cb = 2 * NP - cb;
        }
        BCE_PROF_MARK(4);
        block_sync_lds();
        BCE_PROF_MARK(5);
    }
    BCE_PROF_FLUSH();
    if (inv) {
        u32 x[4];
        {
            const uint4 v = *reinterpret_cast<const uint4*>(acc + cb + c * NP + S.a0);
            u32 a[4] = {v.x, v.y, v.z, v.w};
            split_pass0(S, twf, a, xa, Q, P.mu32);
        }
        split_inverse_rest(S, twf, xa, xb, Q, P.mu32, ninv, wlast, x, [](auto) {});
        u32* out = acc_out + ((size_t)blockIdx.x * 2 + c) * N + S.t;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[256 * r] = x[r];
    } else {
        block_sync_lds();
    }
}


// ---- launcher fragment (launch_blind_rotate, in front of the split-transform branch) ----
/*
        // a folded GINX key and a CU per workgroup: the 16-wave build (BCE_VARIANT=2 keeps the 8-wave one, 4 forces this one)
        const bool w16 = P.fold && !ap && ((x1 && P.variant != 2) || P.variant == 4);
        if (w16) {
            if (kernel_id) *kernel_id = BCE_BR_SPLIT_X1;
            if (tail_fused) *tail_fused = false;
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_blind_rotate_lat16), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_lat);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_blind_rotate_lat16, grid, dim3(1024), lds_lat, s, P, d, n_desc, slot_stride, acc_out, nullptr, nullptr);
            return hipGetLastError();
        }
*/
