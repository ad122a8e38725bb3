// ctx_params_probe.cpp -- asks a PARENT commit's engine what it would decide for a list of shapes, without a device.
// Built and run by make_ctx_params_pins.py only (never part of the library or of a test): it includes the parent's
// engine.cpp, which reaches build_ctx and derive_ctx in their unnamed namespace, and links the parent's other objects.
// On a machine without a GPU build_ctx returns the argument error, or BCE_ERR_NO_DEVICE for a shape it accepts; for those
// derive_ctx runs on an empty context.  The context knobs reach derive_ctx through the environment of the process.
//
// stdin, one case per line:   <id> set <paramset> <method> <cu_count>
//                             <id> custom <n> <N> <q> <Q> <qKS> <baseKS> <baseG> <baseR> <method> <cu_count>
// stdout, one line per case:  <id> TAB <status> TAB <message> TAB <name>=<value> ...      (values only for status 0)
#include "engine.cpp"

#include <cinttypes>
#include <iostream>
#include <sstream>

namespace {

template <class T>
u64 fnv(const std::vector<T>& v) {
    u64 h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}
u64 bits(double d) { u64 b; std::memcpy(&b, &d, 8); return b; }

void put(const char* name, u64 v) { std::printf(" %s=%" PRIu64, name, v); }

void values(bce_ctx* c, const HostTables& T) {
    const DevParams& P = c->P;
#define F(x) put(#x, (u64)P.x)
    F(n); F(N); F(logN); F(q); F(Q); F(qKS); F(baseKS); F(dKS); F(ksk_stride); F(ksk_u16); F(ks_chunk); F(gBits); F(dG); F(baseR); F(dR);
    F(method_ap); F(factor); F(Q8p1); F(red_shift); F(red_mu); F(Ninv); F(Ninv_s); F(Winv_last); F(Winv_last_s); F(mu32); F(lazy); F(c32);
    F(occupancy_target); F(variant); F(cu_count); F(xcd_gate_ticks); F(fuse_tail); F(fold_ninv); F(fold); F(fwd_units); F(factor_even);
    for (int k = 0; k < 4; ++k) put(("I4_" + std::to_string(k)).c_str(), P.I4[k]);
    for (int k = 0; k < 4; ++k) put(("I4s_" + std::to_string(k)).c_str(), P.I4s[k]);
    F(qinv_neg); F(r2_off); F(is64); F(Q64); F(Q8p1_64); F(mu64); F(c64); F(Ninv64); F(Ninv64_s); F(fp64);
    put("Qd", bits(P.Qd)); put("invQd", bits(P.invQd)); put("Ninvd", bits(P.Ninvd)); put("Ninvd_q", bits(P.Ninvd_q));
    F(pool_stride); F(fwd_mfma); F(w14); F(w14s);
#undef F
    put("xcd_gate", T.xcd_gate ? 1 : 0);
    put("psi", c->psi);
    const KernelClass kc = kernel_class(P);
    put("family", (u64)kc.family); put("fold_build", kc.fold_build); put("dag", kc.dag);
    put("wg_per_cu_lone", kc.wg_per_cu_lone); put("wg_per_cu_full", kc.wg_per_cu_full); put("lds_bytes", kc.lds_bytes);
    u32 lone = 0, full = 0;
    bce_launch_capacity(c, &lone, &full);
    put("capacity_lone", lone); put("capacity_full", full);
    u64 parts[3] = {0, 0, 0};
    bce_bytes_per_bootstrap_parts(c, parts);
    put("bytes_bsk", parts[0]); put("bytes_ksk", parts[1]); put("bytes_ct", parts[2]);
    put("forward_transforms", bce_forward_transforms_per_step(c));
    put("fnv_twf", fnv(T.twf)); put("fnv_psi", fnv(T.psi)); put("fnv_psi_r2", fnv(T.psi_r2));
    put("fnv_tw64", fnv(T.tw64)); put("fnv_tw64d", fnv(T.tw64d)); put("fnv_fwd_mfma", fnv(T.fwd.table));
    put("dag_lds_bytes", P.is64 ? 0 : bootstrap_dag_lds_bytes(P, 4));
    // the checks the parent's context makes of itself where the shape is mirrored twice
    if (c->dKS != P.dKS || c->dG != P.dG || c->dR != P.dR || c->logN != P.logN || c->gBits != P.gBits || c->is64 != (P.is64 != 0) ||
        c->qKS != P.qKS || c->Q != P.Q64)
        put("MIRROR_MISMATCH", 1);
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string id, kind;
        u64 n = 0, N = 0, q = 0, Q = 0, qKS = 0, baseKS = 0, baseG = 0, baseR = 0, cu = 0;
        int method = 0;
        if (!(in >> id >> kind)) continue;
        if (kind == "set") {
            int paramset = 0;
            in >> paramset >> method >> cu;
            const ParamRow& r = kParamTable[paramset];
            n = r.n; N = r.cyclo / 2; q = r.q; Q = previous_prime(first_prime(r.bits, r.cyclo), r.cyclo); qKS = r.qKS;
            baseKS = r.baseKS; baseG = r.baseG; baseR = r.baseR;
        } else {
            in >> n >> N >> q >> Q >> qKS >> baseKS >> baseG >> baseR >> method >> cu;
        }
        bce_ctx* none = nullptr;
        int rc = build_ctx((u32)n, (u32)N, q, Q, qKS, (u32)baseKS, (u32)baseG, (u32)baseR, method, 0, &none);
        if (rc == BCE_OK) { std::fprintf(stderr, "a device is visible: run the probe on a machine without one\n"); return 2; }
        if (rc != BCE_ERR_NO_DEVICE) {
            std::printf("%s\t%d\t%s\t\n", id.c_str(), rc, g_create_error.c_str());
            continue;
        }
        bce_ctx* c = new bce_ctx;
        HostTables T;
        g_create_error.clear();
        rc = derive_ctx(c, (u32)n, (u32)N, q, Q, qKS, (u32)baseKS, (u32)baseG, (u32)baseR, method, 0, (u32)cu, T);
        std::printf("%s\t%d\t%s\t", id.c_str(), rc, rc == BCE_OK ? "" : g_create_error.c_str());
        if (rc == BCE_OK) values(c, T);
        std::printf("\n");
        delete c;
    }
    return 0;
}
