// ctx_params.cpp -- see ctx_params.hpp.  Host-only: compiled into the library, and alone by the host compiler for
// tests/integration/ctx_params_selftest.cpp (with a scripted kernel_class).
#include "ctx_params.hpp"

#include <algorithm>
#include <cstring>

#include "host_math.hpp"

namespace bce {

namespace {

struct ParamRow { u32 bits, cyclo, n; u64 q, qKS; u32 baseKS, baseG, baseR; };
// OpenFHE v1.0.x GenerateBinFHEContext table: {numberBits, cyclOrder, latticeParam, mod, modKS(0 = PRIME), baseKS, gadgetBase, baseRK}
const ParamRow kParamTable[] = {
    {27, 1024, 64, 512, 0, 25, 1u << 9, 23},              // TOY
    {28, 2048, 422, 1024, 1u << 14, 1u << 7, 1u << 10, 32},  // MEDIUM
    {27, 2048, 512, 1024, 1u << 14, 1u << 7, 1u << 9, 32},   // STD128_AP
    {27, 2048, 502, 1024, 1u << 14, 1u << 7, 1u << 9, 32},   // STD128_APOPT
    {27, 2048, 512, 1024, 1u << 14, 1u << 7, 1u << 7, 32},   // STD128
    {27, 2048, 502, 1024, 1u << 14, 1u << 7, 1u << 7, 32},   // STD128_OPT
    {37, 4096, 1024, 1024, 1u << 19, 28, 1u << 13, 32},      // STD192
    {37, 4096, 805, 1024, 1u << 15, 32, 1u << 13, 32},       // STD192_OPT
    {29, 4096, 1024, 2048, 1u << 14, 1u << 7, 1u << 8, 46},  // STD256
    {29, 4096, 990, 2048, 1u << 14, 1u << 7, 1u << 8, 46},   // STD256_OPT
};

template <class T>
u64 fnv1a64(const std::vector<T>& v) {
    u64 h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

u64 bits_of(double d) {
    u64 b;
    std::memcpy(&b, &d, 8);
    return b;
}

}  // namespace

bool tabulated_shape(int paramset, int method, Shape& out) {
    if (paramset < 0 || paramset > BCE_STD256_OPT) return false;
    const ParamRow& r = kParamTable[paramset];
    const u64 Q = previous_prime(first_prime(r.bits, r.cyclo), r.cyclo);
    out = Shape{r.n, r.cyclo / 2, r.q, Q, r.qKS, r.baseKS, r.baseG, r.baseR, method};
    return true;
}

CtxStatus validate_shape(const Shape& s) {
    const u32 n = s.n, N = s.N, baseKS = s.baseKS, baseG = s.baseG, baseR = s.baseR;
    const u64 q = s.q, Q = s.Q;
    const int method = s.method;
    if (method != BCE_AP && method != BCE_GINX) return {BCE_ERR_ARG, "bad method (expect AP=1 or GINX=2)"};
    if (N < 512 || N > 2048 || (N & (N - 1))) return {BCE_ERR_UNSUPPORTED, "ring dimension N must be 512, 1024 or 2048"};
    if ((q & (q - 1)) || q > 2 * (u64)N || q < 8) return {BCE_ERR_ARG, "LWE modulus q must be a power of two dividing 2N"};
    if (!is_prime_u64(Q) || (Q - 1) % (2ull * N)) return {BCE_ERR_ARG, "Q must be a prime = 1 mod 2N"};
    if (Q >= (1ull << 40)) return {BCE_ERR_UNSUPPORTED, "ring modulus Q must be below 2^40"};
    if (baseG < 2 || (baseG & (baseG - 1))) return {BCE_ERR_ARG, "gadget base baseG must be a power of two, at least 2"};
    // digit_count divides by log(base), and a base of 0 gives a loop of no digits that "succeeds"
    if (n == 0) return {BCE_ERR_ARG, "LWE dimension n must be at least 1"};
    if (baseKS < 2) return {BCE_ERR_ARG, "key-switching base baseKS must be at least 2"};
    if (method == BCE_AP && baseR < 2) return {BCE_ERR_ARG, "refreshing base baseR must be at least 2 (AP)"};
    return {};
}

CtxParams derive_params(const Shape& s, const CtxKnobs& knobs, u32 cu_count) {
    CtxParams out;
    if ((out.status = validate_shape(s)).code != BCE_OK) return out;
    const auto fail = [&out](int code, const char* message) -> CtxParams& { out.status = {code, message}; return out; };
    const u32 n = s.n, N = s.N, baseKS = s.baseKS, baseG = s.baseG, baseR = s.baseR;
    const u64 q = s.q, Q = s.Q, qKS = s.qKS ? s.qKS : Q;
    u32 logN = 0, gBits = 0;
    while ((1u << logN) < N) ++logN;
    while ((1u << gBits) < baseG) ++gBits;
    const u32 dG = digit_count((double)Q, (double)baseG);
    const bool is64 = Q >= (1ull << 28);

    DevParams& P = out.P;
    HostTables& T = out.T;
    P.n = n; P.N = N; P.logN = logN; P.q = (u32)q; P.Q = (u32)Q; P.qKS = (u32)qKS;
    P.baseKS = baseKS; P.dKS = digit_count((double)qKS, (double)baseKS);
    P.ksk_stride = (n + 1 + 63) & ~63u;
    P.ksk_u16 = qKS <= 65536 ? 1 : 0;
    P.gBits = gBits; P.dG = dG; P.baseR = baseR; P.dR = digit_count((double)q, (double)baseR);
    P.method_ap = s.method == BCE_AP ? 1 : 0;
    P.factor = (u32)(2 * N / q);
    P.factor_even = (P.factor & 1u) ? 0 : 1;   // every STD128 set (q = N); the GINX MAC tail then needs no parity selects
    P.Q8p1 = (u32)(Q / 8 + 1);
    int bq = bit_length(Q);
    P.red_shift = (u32)std::max(2 * bq + 3 - 32, 0);
    P.red_mu = is64 ? 0 : (u32)((((u128)1) << (32 + P.red_shift)) / Q);
    u64 ninv = pow_mod(N, Q - 2, Q);
    P.Ninv = (u32)ninv;
    P.Ninv_s = is64 ? 0 : (u32)(((u128)ninv << 32) / Q);
    P.mu32 = (u32)((((u64)1) << 32) / Q);
    P.c32 = (u32)((((u64)1) << 32) % Q);
    {
        // lazy forward NTT: inputs < 2Q, every stage adds < 2Q -> outputs < B*Q with B = 2*logN+2.
        // needs (1) B*Q < 2^32, (2) R*B*Q*Q < 2^64 for the 64-bit MAC sums, (3) the folded sum
        // (x>>32)*c32 + 2^32 below the Barrett input bound 2^(32+red_shift)
        const u128 B = 2 * logN + 2, R = 2 * dG;
        const u128 sum = R * B * Q * Q;
        const bool ok1 = B * Q < ((u128)1 << 32);
        const bool ok2 = sum < ((u128)1 << 64);
        const u128 folded = (sum >> 32) * P.c32 + ((u128)1 << 32);
        const bool ok3 = folded < ((u128)1 << (32 + P.red_shift));
        // (4) MAC keeps rp, rn < 3Q and acc < 2Q: 3Q*Q + 3Q*Q + 2Q below the Barrett bound, 3Q < 2^32
        const bool ok4 = (u128)6 * Q * Q + 2 * Q < ((u128)1 << (32 + P.red_shift)) && (u128)3 * Q < ((u128)1 << 32);
        // (5) Montgomery form of the MAC tail (split-transform kernels): rp', rn' = REDC(sum) < sum / 2^32 + Q; the monomial
        // factors are lazy in [0, 2Q); y = rp' M+ + rn' M- must fit 64 bits and REDC(y) < y / 2^32 + Q must stay <= 2Q, so that
        // REDC(y) + acc (< 2Q) < 4Q < 2^32 and one conditional subtraction of 2Q returns it to [0, 2Q)
        const u128 rmax = (sum >> 32) + 1 + Q, ymax = 2 * rmax * 2 * Q;
        const bool ok5 = ymax < ((u128)1 << 64) && (ymax >> 32) + 1 + Q <= 2 * (u128)Q && (u128)4 * Q < ((u128)1 << 32);
        P.lazy = (is64 || (ok1 && ok2 && ok3 && ok4 && ok5)) ? 1 : 0;   // (the 64-bit kernels have no other form)
    }
    P.is64 = is64 ? 1 : 0;
    P.Q64 = Q;
    P.variant = knobs.variant;   // development knob, see DevParams::variant
    P.cu_count = cu_count;
    P.fuse_tail = knobs.fuse_tail ? 1 : 0;  // development / parity knob: 0 keeps the separate tail kernels
    // The kernel family and what follows from it (kernels.hpp, kernel_class).  Two requests go in and come back as granted:
    // BCE_OCCUPANCY (development knob: 2 or 3 workgroups per CU of the one-wave-per-transform kernel) and the double-precision
    // formulation of the 64-bit path (kernels64.hip, namespace wd): exact for Q < 2^39; BCE_FP64=0 keeps the integer kernel
    // (development / parity knob)
    P.occupancy_target = knobs.occupancy2 ? 2 : 3;
    P.fp64 = (is64 && Q < (1ull << 39) && knobs.fp64) ? 1 : 0;
    const KernelClass kc = kernel_class(P);
    P.occupancy_target = kc.occupancy_target;
    P.fp64 = kc.fp64;
    if (kc.error) return fail(BCE_ERR_UNSUPPORTED, kc.error);
    if (qKS > 0xFFFFFFFFull) return fail(BCE_ERR_UNSUPPORTED, "qKS must fit 32 bits");
    const u64 psi = out.psi = min_primitive_root(Q, 2ull * N);

    // twiddle tables, OpenFHE ordering: tw[brv(i)] = psi^i
    T.twf.resize(N);
    T.psi.resize(N);
    u64 p = 1;
    for (u32 i = 0; i < N; ++i) {
        T.psi[i] = is64 ? 0 : (u32)p;
        u32 r = bit_reverse(i, (int)logN);
        // device layout: blocks m >= 64 transposed to [slot][lane] (kernels.hip tw_pos)
        u32 pos = r;
        if (r >= 64) {
            const u32 sb = 31u - (u32)__builtin_clz(r), sh = sb - 6, ii = r - (1u << sb);
            pos = (1u << sb) + ((ii & ((1u << sh) - 1u)) << 6) + (ii >> sh);
        }
        T.twf[pos] = is64 ? make_uint2(0, 0) : make_uint2((u32)p, (u32)(((u128)p << 32) / Q));
        p = mul_mod(p, psi, Q);
    }
    const u64 r2modq = is64 ? 0 : (u64)((((u128)1) << 64) % Q);     // R^2 mod Q, R = 2^32
    T.psi_r2.resize(N);
    for (u32 i = 0; i < N; ++i) T.psi_r2[i] = is64 ? 0 : (u32)mul_mod(T.psi[i], r2modq, Q);
    {
        const u64 ch = (((u64)1) << 32) / qKS;
        if (ch < 8) return fail(BCE_ERR_ARG, "qKS too large for the key-switch gather (needs qKS <= 2^29)");
        P.ks_chunk = (u32)std::min<u64>(ch & ~(u64)7, 1u << 20);
    }
    if (!is64) {
        u32 inv = (u32)Q;                                  // Newton: inv = Q^-1 mod 2^32 (Q odd)
        for (int i = 0; i < 5; ++i) inv *= 2u - (u32)Q * inv;
        P.qinv_neg = 0u - inv;
        P.r2_off = (u32)(Q - r2modq);
    }
    {
        u64 I = pow_mod(psi, N / 2, Q), v = 1;
        for (int k = 0; k < 4; ++k) {
            P.I4[k] = (u32)v;
            P.I4s[k] = is64 ? 0 : (u32)(((u128)v << 32) / Q);
            v = mul_mod(v, I, Q);
        }
        const u64 wl = mul_mod(P.I4[3], ninv, Q);  // -I * N^-1 (I^3 = -I)
        P.Winv_last = (u32)wl;
        P.Winv_last_s = is64 ? 0 : (u32)(((u128)wl << 32) / Q);
    }
    P.xcd_gate_ticks = 10000;   // 100 us
    T.xcd_gate = !is64 && knobs.xcd_gate;   // on by default (32-bit path); BCE_XCD_GATE=0: A/B runs
    if (knobs.xcd_gate_us.set && T.xcd_gate) P.xcd_gate_ticks = knobs.xcd_gate_us.value * 100u;
    P.Q8p1_64 = Q / 8 + 1;
    P.mu64 = (u64)((((u128)1) << 64) / Q);
    P.c64 = (u64)((((u128)1) << 64) % Q);
    P.Ninv64 = ninv;
    P.Ninv64_s = (u64)(((u128)ninv << 64) / Q);
    if (is64) {
        T.tw64.resize(N);
        u64 pw = 1;
        for (u32 i = 0; i < N; ++i) {
            T.tw64[bit_reverse(i, (int)logN)] = make_ulonglong2(pw, (u64)(((u128)pw << 64) / Q));
            pw = mul_mod(pw, psi, Q);
        }
        if (kc.lds_error) return fail(BCE_ERR_UNSUPPORTED, kc.lds_error);
        P.Qd = (double)Q;
        P.invQd = 1.0 / (double)Q;
        P.Ninvd = (double)ninv;
        P.Ninvd_q = (double)ninv / (double)Q;
        T.tw64d.resize(N);
        for (u32 i = 0; i < N; ++i) T.tw64d[i] = make_double2((double)T.tw64[i].x, (double)T.tw64[i].x / (double)Q);
    }
    // Lowest gadget digit folded into the key (kernels.hip, FOLD): needs a kernel that has the variant and an EXACT
    // SignedDigitDecompose -- every centred residue d in [-(Q - Q/2), Q/2) must equal sum_l r_l B^l with dG digits
    // r_l in [-B/2, B/2) (then the carry the reference drops after the last digit is always zero).  TOY (27-bit Q,
    // B = 2^9, 3 digits) fails it for the top 0.1 % of residues; STD128* (B = 2^7, 4 digits) and STD192* (37-bit Q,
    // B = 2^13, 3 digits) pass.  BCE_FOLD=0 keeps the plain key (development / parity knob).
    {
        const u128 Bg = (u128)1 << gBits;
        u128 span = 0, pw = 1;
        for (u32 l = 0; l < dG; ++l) { span += pw; pw *= Bg; }
        const u128 hi = (Bg / 2 - 1) * span, lo = (Bg / 2) * span;       // largest / smallest (negated) representable value
        const bool exact = (u128)(Q >> 1) <= hi + 1 && (u128)(Q - (Q >> 1)) <= lo;
        // the folded fp64 kernels multiply a digit by a twiddle in one exact multiplication: |digit| Q <= (B / 2) Q < 2^53
        const bool product_exact = kc.family != KernelFamily::Fp64 || (Bg / 2) * (u128)Q < ((u128)1 << 53);
        P.fold = (exact && kc.fold_build && product_exact && knobs.fold) ? 1 : 0;
        P.fold_ninv = (P.fold && kc.family == KernelFamily::Fp64) ? 1 : 0;
        // forward transforms of the folded N = 1024 GINX kernel as quarter units (kernels.hip); that build is also compiled
        // with the MAC tail of an even factor, so an odd factor keeps the whole-row + half-row bodies and the general tail.
        // BCE_FWD_UNITS=0 keeps them everywhere (development / parity knob, same binary)
        P.fwd_units = (P.fold && !is64 && s.method == BCE_GINX && P.factor_even && knobs.fwd_units) ? 1 : 0;
        // The stages on bits 9..4 of those transforms on the matrix pipe (kernels.hip, ntt_forward_quarter3<true>): a variant of
        // the quarter units, so it needs everything they need (folded key, GINX, even factor, N = 1024, dG = 4) and the
        // arithmetic conditions of fwd_mfma.hpp (gBits <= 7, four 7-bit limbs, exact limb sums, recombined word <= 13Q).
        // Bound chain of the forward phase with this body: recombined words < 2Q + lo_max (< 4Q for STD128*), four lazy stages
        // add < 2Q each -> MAC operands < 12Q, below the 22Q = (2 logN + 2) Q that ok1..ok5 above were checked with.
        // Anything that fails keeps the quarter-unit body; BCE_FWD_MFMA=0 keeps it as well (development / parity knob).
        P.fwd_mfma = 0; P.w14 = P.w14s = 0;
        if (P.fwd_units && knobs.fwd_mfma) {
            T.fwd = build_fwd_mfma_tables(Q, N, gBits, dG, psi);
            if (T.fwd.ok) { P.fwd_mfma = 1; P.w14 = T.fwd.w14; P.w14s = T.fwd.w14s; }
            // The body is a two-workgroups-per-CU build and its byte matrices cost 6 KiB of LDS in front of the (n + 1)-word
            // ciphertext region: where two such workgroups no longer fit a CU (n >= 896) the quarter-unit body stays, which
            // fits up to n = 2431 (beyond that kernel_class reports one workgroup per CU)
            if (P.fwd_mfma && 2 * kernel_class(P).lds_bytes > kLdsBytesPerCu) P.fwd_mfma = P.w14 = P.w14s = 0;
        }
    }
    P.pool_stride = n + 1;
    return out;
}

u32 forward_transforms_per_step(const DevParams& P) { return 2 * P.dG - (P.fold ? 2 : 0); }

void launch_capacity(const DevParams& P, u32* lone, u32* full) {
    const KernelClass k = kernel_class(P);
    *lone = P.cu_count * k.wg_per_cu_lone;
    *full = P.cu_count * k.wg_per_cu_full;
}

void bytes_per_bootstrap_parts(const DevParams& P, u64 out[3]) {
    // w_bsk*[RGSWs touched * (2dG)*2*N] + w_ks*[N*dKS*(n+1)] + w_ct*[3(n+1)] at this build's widths.
    // GINX touches 2 RGSW ciphertexts per LWE coefficient, AP one per non-zero base-baseR digit
    // (dR * (baseR-1)/baseR on average).
    const size_t wbytes = P.is64 ? 8 : 4;
    const double rgsws = P.method_ap ? (double)P.n * P.dR * (P.baseR - 1) / P.baseR : 2.0 * P.n;
    out[0] = (u64)((double)wbytes * rgsws * (2 * P.dG) * 2 * P.N);
    out[1] = (P.ksk_u16 ? 2ull : 4ull) * P.N * P.dKS * (P.n + 1);
    out[2] = 4ull * 3 * (P.n + 1);
}

void params_report(const CtxParams& cp, u64* out) {
    const DevParams& P = cp.P;
    const HostTables& T = cp.T;
    std::fill(out, out + BCE_D_COUNT, 0);
    out[BCE_D_n] = P.n; out[BCE_D_N] = P.N; out[BCE_D_logN] = P.logN; out[BCE_D_q] = P.q; out[BCE_D_Q] = P.Q; out[BCE_D_qKS] = P.qKS;
    out[BCE_D_baseKS] = P.baseKS; out[BCE_D_dKS] = P.dKS; out[BCE_D_ksk_stride] = P.ksk_stride; out[BCE_D_ksk_u16] = P.ksk_u16;
    out[BCE_D_ks_chunk] = P.ks_chunk; out[BCE_D_gBits] = P.gBits; out[BCE_D_dG] = P.dG; out[BCE_D_baseR] = P.baseR; out[BCE_D_dR] = P.dR;
    out[BCE_D_method_ap] = P.method_ap; out[BCE_D_factor] = P.factor; out[BCE_D_Q8p1] = P.Q8p1; out[BCE_D_red_shift] = P.red_shift;
    out[BCE_D_red_mu] = P.red_mu; out[BCE_D_Ninv] = P.Ninv; out[BCE_D_Ninv_s] = P.Ninv_s; out[BCE_D_Winv_last] = P.Winv_last;
    out[BCE_D_Winv_last_s] = P.Winv_last_s; out[BCE_D_mu32] = P.mu32; out[BCE_D_lazy] = P.lazy; out[BCE_D_c32] = P.c32;
    out[BCE_D_occupancy_target] = P.occupancy_target; out[BCE_D_variant] = P.variant; out[BCE_D_cu_count] = P.cu_count;
    out[BCE_D_xcd_gate_ticks] = P.xcd_gate_ticks; out[BCE_D_fuse_tail] = P.fuse_tail; out[BCE_D_fold_ninv] = P.fold_ninv;
    out[BCE_D_fold] = P.fold; out[BCE_D_fwd_units] = P.fwd_units; out[BCE_D_factor_even] = P.factor_even;
    for (int k = 0; k < 4; ++k) { out[BCE_D_I4_0 + k] = P.I4[k]; out[BCE_D_I4s_0 + k] = P.I4s[k]; }
    out[BCE_D_qinv_neg] = P.qinv_neg; out[BCE_D_r2_off] = P.r2_off; out[BCE_D_is64] = P.is64; out[BCE_D_Q64] = P.Q64;
    out[BCE_D_Q8p1_64] = P.Q8p1_64; out[BCE_D_mu64] = P.mu64; out[BCE_D_c64] = P.c64; out[BCE_D_Ninv64] = P.Ninv64;
    out[BCE_D_Ninv64_s] = P.Ninv64_s; out[BCE_D_fp64] = P.fp64; out[BCE_D_Qd] = bits_of(P.Qd); out[BCE_D_invQd] = bits_of(P.invQd);
    out[BCE_D_Ninvd] = bits_of(P.Ninvd); out[BCE_D_Ninvd_q] = bits_of(P.Ninvd_q); out[BCE_D_pool_stride] = P.pool_stride;
    out[BCE_D_fwd_mfma] = P.fwd_mfma; out[BCE_D_w14] = P.w14; out[BCE_D_w14s] = P.w14s;
    out[BCE_D_xcd_gate] = T.xcd_gate ? 1 : 0; out[BCE_D_psi] = cp.psi;
    const KernelClass kc = kernel_class(P);
    out[BCE_D_family] = (u64)kc.family; out[BCE_D_fold_build] = kc.fold_build ? 1 : 0; out[BCE_D_dag] = kc.dag ? 1 : 0;
    out[BCE_D_wg_per_cu_lone] = kc.wg_per_cu_lone; out[BCE_D_wg_per_cu_full] = kc.wg_per_cu_full; out[BCE_D_lds_bytes] = kc.lds_bytes;
    out[BCE_D_capacity_lone] = (u64)P.cu_count * kc.wg_per_cu_lone; out[BCE_D_capacity_full] = (u64)P.cu_count * kc.wg_per_cu_full;
    bytes_per_bootstrap_parts(P, out + BCE_D_bytes_bsk);
    out[BCE_D_forward_transforms] = forward_transforms_per_step(P);
    out[BCE_D_fnv_twf] = fnv1a64(T.twf); out[BCE_D_fnv_psi] = fnv1a64(T.psi); out[BCE_D_fnv_psi_r2] = fnv1a64(T.psi_r2);
    out[BCE_D_fnv_tw64] = fnv1a64(T.tw64); out[BCE_D_fnv_tw64d] = fnv1a64(T.tw64d); out[BCE_D_fnv_fwd_mfma] = fnv1a64(T.fwd.table);
}

DagLaunchChoice dag_launch_choice(const DevParams& P, u32 wg_per_cu_full, size_t dag_lds_bytes_wps4, const DagLimits& lim,
                                  const DagKnobs& knobs, u32 depth, u64 items) {
    DagLaunchChoice D;
    D.lazy_ticks = lim.lazy_us * 100u;                     // s_memrealtime: 100 MHz
    D.stall_ticks = lim.stall_ms * 100000u;
    D.policy = lim.placement ? 1u : 0u;
    D.gate_ticks = 15000;        // 150 us: the finish times of bootstraps that started together spread less than that
    D.gate_backlog = 8;          // (64 / 16 / 4 / 1: AES K = 8 at 150 / 153 / 154 / 155 k; with the classes below 157 k, profiles/r03_dataflow_vs_steps.jsonl)
    if (knobs.gate_us.set) D.gate_ticks = knobs.gate_us.value * 100u;
    if (knobs.gate_backlog.set) D.gate_backlog = knobs.gate_backlog.value;
    // one or two workgroups per CU: two run 512 bootstraps per ~3.1 ms, one runs 256 per ~1.9 ms -- with less work per
    // dependency level than the CUs can hold alone, the shorter bootstrap wins
    int wps = lim.wg_per_cu == 1 ? 2 : 4;
    if (lim.wg_per_cu == 0) {
        // lower bound of the run under either residency, in units of one bootstrap with a CU to itself: the DAG's longest
        // chain against the work over the chip's rate.  Two workgroups per CU take 1.6 x as long per bootstrap (3.1 vs
        // 1.93 ms) and deliver 1.26 x the rate (165 vs 131 k/s); the cheaper bound wins (AES-expanded: K <= 2 one per CU,
        // K >= 4 two; md5 K = 16 and adder_64 K = 64 one.  Against the earlier rule "work per level <= 3/4 of the CUs":
        // adder_64 K = 64 97.9 -> 117.9 k/s, AES K = 2 115.7 -> 109.6 k, md5 K = 16 114.0 -> 110.1 k,
        // profiles/r03_dataflow_vs_steps.jsonl)
        const double Dp = (double)std::max<u32>(1, depth), W = (double)items, cus = (double)std::max<u32>(1, P.cu_count);
        const double t1 = std::max(Dp, W / cus), t2 = std::max(1.6 * Dp, W / (1.26 * cus));
        wps = t1 <= t2 ? 2 : 4;
    }
    if (knobs.wps == '2') wps = 2; else if (knobs.wps == '4') wps = 4;
    if (wg_per_cu_full == 1) wps = 2;   // a CU's LDS holds one workgroup (the config-5 kernel; the split-transform kernel at n >= 2432)
    // the persistent kernel's own LDS (mailbox in front of the layout): where two such workgroups do not fit a CU although two
    // of the per-frontier kernel do (n = 888..895 on the matrix-pipe build, 2424..2431 on the quarter-unit build), one per CU
    if (wps == 4 && !P.is64 && 2 * dag_lds_bytes_wps4 > kLdsBytesPerCu) wps = 2;
    if (knobs.place >= 0) D.policy = knobs.place == '0' ? 0u : 1u;
    // development: 'r' = re-arm only, 'd' = dry run (no bootstraps)
    if (knobs.debug == 'd') D.policy |= 2u;
    D.rearm_only = knobs.debug == 'r';
    // the XCD start gate pays where two workgroups per CU share the L2 in the saturated regime (development knob BCE_DAG_GATE=0 / 1)
    if (knobs.gate >= 0 ? knobs.gate != '0' : wps == 4) D.policy |= 4u;
    if (knobs.tickets) D.policy |= 8u;   // development: round 3's claim rule
    D.wps = wps;
    D.grid = P.cu_count * (wps == 2 ? 1u : 2u);
    return D;
}

}  // namespace bce
