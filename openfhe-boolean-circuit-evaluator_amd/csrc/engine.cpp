// engine.cpp -- host side of the C ABI in include/bce_gpu.h.
//
// Replaces what the reference obtains from lbcrypto::BinFHEContext (OpenFHE):
// GenerateBinFHEContext / KeyGen / BTKeyGen (src/circuit.cpp:88-91), Encrypt / Decrypt
// (src/circuit.cpp:506,800) and the per-gate EvalBinGate / EvalNOT calls
// (src/gate.cpp:112,133,172,198-202), the latter batched per ready frontier.
// There is no CPU compute path here: without a HIP device every call fails loudly.
// This file: the context (its tables on the device, keys, pool and LWE I/O; what it decides about itself is ctx_params.cpp),
// one frontier of gates, timing and the debug entry points.  The schedules built on it live in engine_plan.cpp (bce_plan, bce_check_*) and engine_dag.cpp (bce_dag).
#include <sys/random.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/bce_circuit.h"
#include "ctx_params.hpp"
#include "desc.hpp"
#include "engine_internal.hpp"
#include "host_math.hpp"
#include "keygen.hpp"
#include "prng.hpp"

using namespace bce;

std::mutex bce::g_live_mu;
std::unordered_set<const bce_ctx*> bce::g_live;

static_assert(sizeof(bce_check_report) == 48 && sizeof(bce_check_entry) == 24, "layout of the check structs (include/bce_gpu.h; the kernel writes them)");

namespace {

thread_local std::string g_create_error;

// 32 bytes from the operating system's entropy pool (getrandom, then /dev/urandom).  There is no fixed
// fallback value: a context that cannot get entropy fails to draw keys / encryption randomness.
bool os_entropy(uint8_t out[32]) {
    size_t got = 0;
    while (got < 32) {
        const ssize_t r = getrandom(out + got, 32 - got, 0);
        if (r <= 0) break;
        got += (size_t)r;
    }
    if (got == 32) return true;
    FILE* f = std::fopen("/dev/urandom", "rb");
    if (!f) return false;
    const size_t n = std::fread(out, 1, 32, f);
    std::fclose(f);
    return n == 32;
}

// Stream, and the tables of derive_params on the device
int upload_ctx(bce_ctx* c, const HostTables& T) {
    DevParams& P = c->P;
    if (hipSetDevice(c->device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return BCE_ERR_HIP; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "hipStreamCreate failed"; return BCE_ERR_HIP; }
    // `what` names the table in the message of a failure
    const auto up = [](auto& dst, const auto& v, const char* what) -> bool {
        if (upload_vector(dst, v) == hipSuccess) return true;
        g_create_error = std::string("hipMalloc(") + what + ") failed";
        return false;
    };
    if (!up(c->d_twf, T.twf, "twiddles") || !up(c->d_psi, T.psi, "psi table") || !up(c->d_psi_r2, T.psi_r2, "psi table")) return BCE_ERR_HIP;
    P.tw_f = c->d_twf.get();
    P.psi_tab = c->d_psi.get();
    P.psi_tab_r2 = c->d_psi_r2.get();
    P.xcd_gate = nullptr;
    if (T.xcd_gate) {
        if (c->d_xcd_gate.alloc(16 * 32) != hipSuccess) { g_create_error = "hipMalloc(xcd gate) failed"; return BCE_ERR_HIP; }
        P.xcd_gate = c->d_xcd_gate.get();
    }
    if (c->is64) {
        if (!up(c->d_tw64, T.tw64, "twiddles64") || !up(c->d_tw64d, T.tw64d, "twiddles64d")) return BCE_ERR_HIP;
        P.tw64 = c->d_tw64.get();
        P.tw64d = c->d_tw64d.get();
    }
    P.fwd_mfma_tab = nullptr;
    if (P.fwd_mfma) {
        if (!up(c->d_fwd_mfma, T.fwd.table, "forward matrix table")) return BCE_ERR_HIP;
        P.fwd_mfma_tab = c->d_fwd_mfma.get();
    }
    // the key-set table: every entry null until a set gets its buffers (alloc_keys)
    if (c->d_keysets.alloc(BCE_MAX_KEYSETS) != hipSuccess || hipMemset(c->d_keysets.get(), 0, BCE_MAX_KEYSETS * sizeof(KeySetDev)) != hipSuccess) {
        g_create_error = "hipMalloc(key-set table) failed";
        return BCE_ERR_HIP;
    }
    P.keysets = c->d_keysets.get();
    P.keyset_sel = 0;
    P.keyset_map = nullptr;
    c->enc_seed_ok = os_entropy(c->enc_seed);
    return BCE_OK;
}

// validate; query the device; derive (ctx_params.cpp); copy the result into a context; upload
int build_ctx(const Shape& s, int device, bce_ctx** out) {
    if (!out) return BCE_ERR_ARG;
    *out = nullptr;
    if (const CtxStatus st = validate_shape(s); st.code != BCE_OK) { g_create_error = st.message; return st.code; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_error = "no HIP device visible: the engine has no CPU fallback";
        return BCE_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { g_create_error = "bad device ordinal"; return BCE_ERR_ARG; }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const CtxParams cp = derive_params(s, read_ctx_knobs(), (u32)cus);
    if (cp.status.code != BCE_OK) { g_create_error = cp.status.message; return cp.status.code; }

    // partially built contexts are released through bce_ctx_destroy (frees whatever was allocated)
    struct CtxDeleter { void operator()(bce_ctx* p) const { bce_ctx_destroy(p); } };
    std::unique_ptr<bce_ctx, CtxDeleter> c(new bce_ctx);
    { std::lock_guard<std::mutex> lk(g_live_mu); g_live.insert(c.get()); }
    const DevParams& P = c->P = cp.P;
    c->n = P.n; c->N = P.N; c->logN = P.logN; c->q = s.q; c->Q = s.Q; c->qKS = P.qKS; c->psi = cp.psi;
    c->baseKS = P.baseKS; c->dKS = P.dKS; c->baseG = s.baseG; c->gBits = P.gBits; c->dG = P.dG; c->baseR = P.baseR; c->dR = P.dR;
    c->method = s.method; c->device = device;
    c->is64 = P.is64 != 0;
    c->wbytes = c->is64 ? 8 : 4;
    c->keysets[0] = std::make_unique<KeySet>();
    if (const int rc = upload_ctx(c.get(), cp.T)) return rc;
    *out = c.release();
    return BCE_OK;
}

u64 rgsw_rows_total(const bce_ctx* c);
// evaluation-form key words -> what the kernels read: rows l >= 1 of every RGSW ciphertext minus B^l times row 0
// when the lowest gadget digit is folded (P.fold); IEEE doubles for the double-precision 64-bit kernels (exact, Q < 2^39)
int bsk_words_to_kernel_layout(bce_ctx* c) {
    if (c->P.fold) HIP_TRY(c, launch_fold_gadget(c->P, c->keys().d_bsk.get(), rgsw_rows_total(c) / (2ull * c->dG), +1, c->stream));
    if (!c->P.fp64) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return BCE_OK; }
    HIP_TRY(c, launch_words_u64_f64(reinterpret_cast<u64*>(c->keys().d_bsk.get()), (size_t)c->keys().bsk_polys * c->N, 1, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BCE_OK;
}

u64 rgsw_rows_total(const bce_ctx* c) {
    const u64 R = 2ull * c->dG;
    return c->method == BCE_GINX ? (u64)c->n * 2 * R : (u64)c->n * c->baseR * c->dR * R;
}

int alloc_keys(bce_ctx* c) {
    if (c->keys().d_bsk.get() && c->keys().d_ksk.get() && c->keys().d_s8.get()) return BCE_OK;   // (and the table holds their row)
    if (!c->keys().d_bsk.get()) {
        c->keys().bsk_polys = rgsw_rows_total(c) * 2;
        HIP_TRY(c, c->keys().d_bsk.alloc(c->wbytes * c->keys().bsk_polys * c->N));
    }
    if (!c->keys().d_ksk.get()) {
        size_t rows = (size_t)c->N * c->baseKS * c->dKS;
        HIP_TRY(c, c->keys().d_ksk.alloc(rows * c->P.ksk_stride * (c->P.ksk_u16 ? 2 : 4)));
    }
    if (!c->keys().d_s8.get()) HIP_TRY(c, c->keys().d_s8.alloc(((size_t)c->n + 63) / 64 * 64));
    // the set's row of the device table: written when the set gets its buffers (they never move), after the work in flight
    const KeySetDev row{c->keys().d_bsk.get(), c->keys().d_ksk.get(), c->keys().d_s8.get()};
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->d_keysets.get() + c->selected, &row, sizeof row, hipMemcpyHostToDevice));
    return BCE_OK;
}

// host KSK rows (u32, canonical [row][n+1]) -> padded device layout
int upload_ksk(bce_ctx* c, const u32* ksk) {
    const size_t rows = (size_t)c->N * c->baseKS * c->dKS, W = c->n + 1, S = c->P.ksk_stride;
    if (c->P.ksk_u16) {
        std::vector<uint16_t> buf(rows * S, 0);
        for (size_t r = 0; r < rows; ++r)
            for (size_t k = 0; k < W; ++k) buf[r * S + k] = (uint16_t)ksk[r * W + k];
        HIP_TRY(c, hipMemcpy(c->keys().d_ksk.get(), buf.data(), buf.size() * 2, hipMemcpyHostToDevice));
    } else {
        std::vector<u32> buf(rows * S, 0);
        for (size_t r = 0; r < rows; ++r) std::memcpy(&buf[r * S], &ksk[r * W], W * 4);
        HIP_TRY(c, hipMemcpy(c->keys().d_ksk.get(), buf.data(), buf.size() * 4, hipMemcpyHostToDevice));
    }
    return BCE_OK;
}

// the LWE secret as the device-side check reads it (k_lwe_check): int8[n], padded with zeros to a multiple of 64.  The
// buffer is allocated once per key set (alloc_keys), so the device table's pointer to it survives a key import.
int upload_secret(bce_ctx* c) {
    const size_t padded = ((size_t)c->n + 63) / 64 * 64;
    std::vector<int8_t> s8(padded, 0);
    for (u32 k = 0; k < c->n; ++k) s8[k] = (int8_t)c->keys().s[k];
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->keys().d_s8.get(), s8.data(), padded, hipMemcpyHostToDevice));
    return BCE_OK;
}

// Stage a descriptor list into the next ring slot (1,024 descriptors at least).  The caller launches the kernel that reads
// descs_of(slot) and then marks the slot: its event must follow that kernel, not just the copy.  map (may be null): the
// key-set map of a keyed launch, n_map words behind the descriptors in the same copy (map_of).
int stage_descs(bce_ctx* c, const bce_gate_desc* d, size_t n, StagedUpload** slot, const u32* map = nullptr, size_t n_map = 0) {
    StagedUpload& r = c->ring[c->ring_pos];
    c->ring_pos = (c->ring_pos + 1) % bce_ctx::kRing;
    const size_t dbytes = n * sizeof(bce_gate_desc), bytes = dbytes + (map ? n_map * sizeof(u32) : 0);
    HIP_TRY(c, r.reserve(bytes, std::max(bytes, (size_t)1024 * sizeof(bce_gate_desc)), nullptr));
    std::memcpy(r.host(), d, dbytes);
    if (map) std::memcpy(static_cast<char*>(r.host()) + dbytes, map, n_map * sizeof(u32));
    HIP_TRY(c, r.copy(bytes, c->stream));
    *slot = &r;
    return BCE_OK;
}
const bce_gate_desc* descs_of(const StagedUpload* slot) { return static_cast<const bce_gate_desc*>(slot->device()); }
const u32* map_of(const StagedUpload* slot, size_t n) { return reinterpret_cast<const u32*>(descs_of(slot) + n); }
static_assert(sizeof(bce_gate_desc) % sizeof(u32) == 0, "a key-set map behind a descriptor list is aligned");

void drain_timing(bce_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            if (p.kind < BCE_BR_KERNELS) { c->timing.blind_rotate_ms += ms; c->timing.br_ms[p.kind] += ms; }
            else c->timing.tail_ms += ms;
        }
        c->free_events.push_back(p);
    }
    c->pending.clear();
}

// uint64_t words of the ABI <-> words in device memory: u64 as they are (wide), u32 through a staging vector.  The
// accumulators, key words and polynomials of a context are wide when c->is64; LWE words are always 32-bit.
int words_to_device(bce_ctx* c, void* dev, const u64* src, size_t words, bool wide) {
    if (wide) {
        HIP_TRY(c, hipMemcpy(dev, src, words * 8, hipMemcpyHostToDevice));
    } else {
        const std::vector<u32> tmp(src, src + words);
        HIP_TRY(c, hipMemcpy(dev, tmp.data(), words * 4, hipMemcpyHostToDevice));
    }
    return BCE_OK;
}
int words_from_device(bce_ctx* c, u64* dst, const void* dev, size_t words, bool wide) {
    if (wide) {
        HIP_TRY(c, hipMemcpy(dst, dev, words * 8, hipMemcpyDeviceToHost));
    } else {
        std::vector<u32> tmp(words);
        HIP_TRY(c, hipMemcpy(tmp.data(), dev, words * 4, hipMemcpyDeviceToHost));
        std::copy(tmp.begin(), tmp.end(), dst);
    }
    return BCE_OK;
}

int dev_ntt(bce_ctx* c, void* polys, u64 count, int inverse) {
    // count may exceed what one launch indexes comfortably; split in slabs of 2^20 polys
    const u64 slab = 1u << 20;
    for (u64 o = 0; o < count; o += slab) {
        const u32 cnt = (u32)std::min<u64>(slab, count - o);
        HIP_TRY(c, launch_ntt_batch(c->P, static_cast<char*>(polys) + o * c->N * c->wbytes, cnt, inverse, c->stream));
    }
    return BCE_OK;
}

// device copies of what the key samplers read (keygen.hip): secrets, Gaussian CDF table, parameters
struct KeygenDev {
    DevBuf<int32_t> s, z;
    DevBuf<u64> cdf;
    DevBuf<char> ta, zq;
};

int keygen_params(bce_ctx* c, const GaussSampler& gauss, KeygenDev& D, KeygenParams& kp) {
    HIP_TRY(c, upload_vector(D.s, c->keys().s));
    HIP_TRY(c, upload_vector(D.z, c->keys().z));
    HIP_TRY(c, D.cdf.alloc(81));
    HIP_TRY(c, hipMemcpy(D.cdf.get(), gauss.table(), 81 * sizeof(u64), hipMemcpyHostToDevice));
    std::memcpy(kp.seed, c->keys().seed, 32);
    kp.n = c->n; kp.N = c->N; kp.Q = c->Q; kp.q = c->q; kp.qKS = c->qKS;
    kp.qbits = bit_length(c->Q - 1); kp.ksbits = bit_length(c->qKS - 1);
    kp.R = 2 * c->dG; kp.ap = c->method == BCE_AP ? 1 : 0; kp.baseR = c->baseR; kp.dR = c->dR;
    kp.baseKS = c->baseKS; kp.dKS = c->dKS; kp.ksk_stride = c->P.ksk_stride;
    { u64 v = 1; for (u32 i = 0; i < 4; ++i) { kp.gpow[i] = v; v = mul_mod(v, c->baseG, c->Q); } }
    kp.s = D.s.get(); kp.z = D.z.get(); kp.cdf = D.cdf.get();
    return BCE_OK;
}

// Bootstrapping key.  GINX: ek[i][0] = RGSW(s_i == 1), ek[i][1] = RGSW(s_i == -1)
// (rgsw-acc-cggi.cpp KeyGenAcc).  AP: ek[i][v][k] = RGSW(X^{s_i * v * baseR^k * 2N/q}), v >= 1
// (rgsw-acc-dm.cpp KeyGenAcc; the v = 0 slots stay zero and are never read).
// Everything happens on the device: rows (a, e + gadget) are sampled in place (keygen.hip), transformed, and
// b += NTT(a) * NTT(z).  Rows are produced in chunks whose scratch (the masks once more) stays below 1 GiB
// whatever the key size (STD192/AP: 12.9 GB of key).
int keygen_bsk(bce_ctx* c, const KeygenParams& kp, KeygenDev& D) {
    const u32 N = c->N, R = 2 * c->dG;
    const u64 Q = c->Q;
    const size_t wb = c->wbytes;
    const u64 rows = rgsw_rows_total(c);
    const u64 chunk = std::max<u64>(R, std::min<u64>(rows, ((u64)1 << 30) / ((u64)N * wb)) / R * R);
    HIP_TRY(c, D.ta.alloc(chunk * N * wb));
    HIP_TRY(c, D.zq.alloc(N * wb));
    {
        std::vector<u64> zq(N);
        for (u32 k = 0; k < N; ++k) zq[k] = lift_signed(c->keys().z[k], Q);
        if (const int rc = words_to_device(c, D.zq.get(), zq.data(), N, c->is64)) return rc;
    }
    int rc = dev_ntt(c, D.zq.get(), 1, 0);
    if (rc) return rc;
    char* dev = c->keys().d_bsk.get();
    for (u64 r0 = 0; r0 < rows; r0 += chunk) {
        const u64 cnt = std::min(chunk, rows - r0);
        char* dst = dev + r0 * 2 * N * wb;
        HIP_TRY(c, launch_gen_bsk_rows(kp, r0, (u32)cnt, dst, D.ta.get(), c->is64 ? 1 : 0, c->stream));
        if ((rc = dev_ntt(c, dst, cnt * 2, 0))) return rc;
        if ((rc = dev_ntt(c, D.ta.get(), cnt, 0))) return rc;
        // b-column (odd polys) += NTT(a) * NTT(z)
        HIP_TRY(c, launch_pointwise_mac(c->P, dst + N * wb, D.ta.get(), D.zq.get(), (u32)cnt, 2, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BCE_OK;
}

// after a stream synchronisation: verdict of the dependency-driven runs that finished since the last check
int check_dag_runs(bce_ctx* c) {
    int rc = BCE_OK;
    for (int i = 0; i < c->dag_pending; ++i) {
        const bce_ctx::DagStatus& st = c->h_dag_status.get()[i];
        c->dag_last[0] = st.done; c->dag_last[1] = st.lazy_waits; c->dag_last[2] = st.abort; c->dag_last[3] = (u64)c->dag_wps_used[i] / 2;
        c->dag_last[4] = st.busy_ticks; c->dag_last[5] = st.wait_ticks; c->dag_last[6] = st.gate_ticks;
        if (st.abort != 0 || st.done != c->dag_expected[i])
            rc = c->fail(BCE_ERR_STATE, "bce_dag_run: the device scheduler gave up (abort code %u, %u of %llu bootstraps completed, no progress for %u ms)",
                         st.abort, st.done, (unsigned long long)c->dag_expected[i], c->dag_stall_ms);
    }
    c->dag_pending = 0;
    return rc;
}

// map (may be null): the key set of every instance (bce_eval_gates_keyed); null: every instance runs under the selected set
int eval_impl(bce_ctx* c, u32 n_desc, const bce_gate_desc* descs, u32 instances, u32 slot_stride, u64* dbg_acc,
              u64* dbg_lweN, u64* dbg_ks, const u32* map = nullptr) {
    if (n_desc == 0 || instances == 0) return BCE_OK;
    if (!descs) return c->fail(BCE_ERR_ARG, "null descriptor list");
    if (const int rc = map ? need_keys_of_map(c, "bce_eval_gates_keyed", map, instances) : need_keys(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<bce_gate_desc> boot, unary;
    boot.reserve(n_desc);
    const u64 max_slot = (u64)(instances - 1) * slot_stride;
    u32 n_pairs = 0;
    for (u32 i = 0; i < n_desc; ++i) {
        const bce_gate_desc& g = descs[i];
        const DescKind k = desc_kind(g.op);
        if (k.cls == DescClass::None) return c->fail(BCE_ERR_ARG, "descriptor %u: unknown op %u", i, g.op);
        n_pairs += k.pair();
        const u64 hi = top_slot(g, k);
        if (hi + max_slot >= c->pool_slots) return c->fail(BCE_ERR_POOL, "descriptor %u: slot %llu outside the pool (%u slots)", i, (unsigned long long)(hi + max_slot), c->pool_slots);
        (k.boot() ? boot : unary).push_back(g);
    }
    if (!boot.empty()) {
        const size_t nb = boot.size() * (size_t)instances;
        int rc = ensure_acc(c, nb);
        if (rc) return rc;
        StagedUpload* slot = nullptr;
        rc = stage_descs(c, boot.data(), boot.size(), &slot, map, instances);
        if (rc) return rc;
        DevBuf<u32> d_lweN, d_ks;
        // staged outputs of a launch with pairs: the kernels write the second outputs to a second block of nb rows
        const size_t dbg_rows = n_pairs ? 2 * nb : nb;
        if (dbg_lweN) HIP_TRY(c, d_lweN.alloc(dbg_rows * (c->N + 1)));
        if (dbg_ks) HIP_TRY(c, d_ks.alloc(dbg_rows * (c->n + 1)));
        rc = launch_bootstraps(c, descs_of(slot), (u32)boot.size(), instances, slot_stride, c->d_acc.get(), d_lweN.get(), d_ks.get(), true, nullptr, n_pairs != 0, nullptr,
                               map ? map_of(slot, boot.size()) : nullptr);
        if (rc) return rc;
        slot->mark(c->stream);
        if (dbg_acc || dbg_lweN || dbg_ks) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (dbg_acc && (rc = words_from_device(c, dbg_acc, c->d_acc.get(), nb * 2 * c->N, c->is64))) return rc;
            if (dbg_lweN && (rc = words_from_device(c, dbg_lweN, d_lweN.get(), nb * (c->N + 1), false))) return rc;
            if (dbg_ks && (rc = words_from_device(c, dbg_ks, d_ks.get(), nb * (c->n + 1), false))) return rc;
            // ... which the caller gets packed, in descriptor order, from row nb on (bce_debug_eval_stages: one instance)
            if (n_pairs) {
                auto pack = [&](u64* dst, const u32* dev, size_t w) {   // the second block in one copy, then packed on the host
                    std::vector<u64> second(nb * w);
                    const int e = words_from_device(c, second.data(), dev + nb * w, nb * w, false);
                    for (size_t i = 0, row = nb; !e && i < nb; ++i)
                        if (pair_kind(boot[i].op) > 0) std::copy_n(second.data() + i * w, w, dst + row++ * w);
                    return e;
                };
                if (dbg_lweN) rc = pack(dbg_lweN, d_lweN.get(), c->N + 1);
                if (dbg_ks && !rc) rc = pack(dbg_ks, d_ks.get(), c->n + 1);
            }
            if (rc) return rc;
        }
        if (const int rc2 = drain_if_long(c)) return rc2;
    }
    if (!unary.empty()) {
        StagedUpload* slot = nullptr;
        int rc = stage_descs(c, unary.data(), unary.size(), &slot);
        if (rc) return rc;
        HIP_TRY(c, launch_lwe_unary(c->P, descs_of(slot), (u32)unary.size(), instances, slot_stride, c->stream));
        slot->mark(c->stream);
    }
    return BCE_OK;
}

}  // namespace

// ---- shared with engine_plan.cpp and engine_dag.cpp (engine_internal.hpp) ----------------------------------------------
namespace bce {

// report block + mismatch log of the device-side checks: one allocation per context, zeroed
int ensure_check(bce_ctx* c) {
    if (c->d_check_mem.get()) return BCE_OK;
    const size_t bytes = sizeof(bce_check_report) + (size_t)kCheckLogCap * sizeof(bce_check_entry);
    DevBuf<char> mem;
    HIP_TRY(c, mem.alloc(bytes));
    if (hipMemset(mem.get(), 0, bytes) != hipSuccess) return c->fail(BCE_ERR_HIP, "hipMemset(check report) failed");
    c->d_check_mem = std::move(mem);
    return BCE_OK;
}

// accumulators for `boots` bootstraps: at least doubled when they grow, after the work in flight
int ensure_acc(bce_ctx* c, size_t boots) {
    const size_t need = boots * 2 * c->N * c->wbytes;
    HIP_TRY(c, c->d_acc.grow(need, std::max(need, 2 * c->d_acc.capacity()), c->stream));
    return BCE_OK;
}

EventPair get_events(bce_ctx* c, int kind) {
    EventPair p;
    if (!c->free_events.empty()) {
        p = c->free_events.back();
        c->free_events.pop_back();
    } else {
        hipEventCreate(&p.a);
        hipEventCreate(&p.b);
    }
    p.kind = kind;
    return p;
}

// after a launch: keeps the list of event pairs short
int drain_if_long(bce_ctx* c) {
    if (c->pending.size() <= 4096) return BCE_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drain_timing(c);
    return BCE_OK;
}

int sync_stream(bce_ctx* c) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return check_dag_runs(c);
}

// the expected bits of a check list are messages; `who` names the call in the message
int expected_are_messages(bce_ctx* c, const char* who, const uint8_t* expect, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (expect[i] > 3) return c->fail(BCE_ERR_ARG, "%s: expect[%zu] = %u is not a message (0..3)", who, i, expect[i]);
    return BCE_OK;
}

// One frontier of bootstrapped gates whose descriptors already sit on the device: blind rotation (+ the tail kernels
// when the blind-rotation kernel does not carry it).  timed: HIP events around each kernel group + the counters of
// bce_timing; untimed (stream capture of bce_plan_run): launches only, *fused_out says whether the tail was fused.
// pairs: at least one descriptor is a pair (its second tail pass runs in the fused epilogue or as a second tail launch).
int launch_bootstraps(bce_ctx* c, const bce_gate_desc* dd, u32 n, u32 instances, u32 slot_stride, void* d_acc,
                      u32* d_lweN, u32* d_ks, bool timed, bool* fused_out, bool pairs, u64* d_partial, const u32* d_map) {
    const size_t nb = (size_t)n * instances;
    DevParams P = c->P;      // the launch's copy: a keyed launch (d_map: [instances] key-set ids on the device) names its map in it
    P.keyset_map = d_map;
    int kid = 0;
    bool tail_fused = false;
    const bool events = timed && c->events_on;
    EventPair e0{};
    // the timestamps ride on the kernels' own dispatches (LaunchEvents): no event packet between dependent launches
    LaunchEvents le0{};
    if (events) { e0 = get_events(c, 0); le0 = LaunchEvents{e0.a, e0.b}; }
    {   // a launch that fails hands its event pair back (it would otherwise be neither pending nor free)
        const hipError_t e = launch_blind_rotate(P, dd, n, instances, slot_stride, d_acc, c->stream, &kid, d_lweN, d_ks, &tail_fused, le0);
        if (e != hipSuccess) {
            if (events) c->free_events.push_back(e0);
            HIP_TRY(c, e);
        }
    }
    if (events) {
        e0.kind = kid;
        c->pending.push_back(e0);
    }
    if (timed) {
        c->timing.br_launches[kid] += 1;
        c->timing.br_bootstraps[kid] += nb;
    }
    if (!tail_fused) {
        EventPair e1{};
        LaunchEvents le1{};
        if (events) {
            e1 = get_events(c, BCE_BR_KERNELS);  // kind >= BCE_BR_KERNELS: tail
            le1 = LaunchEvents{e1.a, e1.b};
        }
        if (!d_partial) {
            const size_t need = tail_partial_words(P, (u32)nb);   // grows like the accumulators (ensure_acc)
            HIP_TRY(c, c->d_tail_partial.grow(need, std::max(need, 2 * c->d_tail_partial.capacity()), c->stream));
        }
        const hipError_t e = launch_tail(P, dd, n, instances, slot_stride, d_acc, d_partial ? d_partial : c->d_tail_partial.get(), d_lweN, d_ks, c->stream, le1, pairs);
        if (e != hipSuccess) {
            if (events) c->free_events.push_back(e1);
            HIP_TRY(c, e);
        }
        if (events) c->pending.push_back(e1);
    } else if (timed) {
        c->timing.fused_tail_launches += 1;
    }
    if (timed) {
        c->timing.blind_rotate_launches += 1;
        c->timing.bootstraps += nb;
    }
    if (fused_out) *fused_out = tail_fused;
    return BCE_OK;
}

}  // namespace bce

extern "C" {

int bce_ctx_create(int paramset, int method, int device, bce_ctx** out) {
    Shape s;
    if (!tabulated_shape(paramset, method, s)) { g_create_error = "unknown parameter set"; if (out) *out = nullptr; return BCE_ERR_ARG; }
    return build_ctx(s, device, out);
}

int bce_ctx_create_custom(uint32_t n, uint32_t N, uint64_t q, uint64_t Q, uint64_t qKS, uint32_t baseKS, uint32_t baseG,
                          uint32_t baseR, int method, int device, bce_ctx** out) {
    return build_ctx(Shape{n, N, q, Q, qKS, baseKS, baseG, baseR, method}, device, out);
}

int bce_rccl_shutdown(bce_ctx* c);   // rccl_xchg.cpp

// The order is kept in this body rather than in the order of bce_ctx's members: the stream is synchronised first, every
// buffer of the context and of its schedules is released by its owner (devmem.hpp), the stream is destroyed last.
void bce_ctx_destroy(bce_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->rccl_comm) bce_rccl_shutdown(c);
    drain_timing(c);
    {   // schedules nobody destroyed: theirs callers' handles die with the context
        std::unordered_set<bce_plan*> plans;
        std::unordered_set<bce_dag*> dags;
        { std::lock_guard<std::mutex> lk(g_live_mu); plans.swap(c->plans); dags.swap(c->dags); g_live.erase(c); }
        for (bce_plan* p : plans) delete_leftover(p);
        for (bce_dag* g : dags) delete_leftover(g);
    }
    for (auto& p : c->free_events) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    const hipStream_t stream = c->stream;
    delete c;
    if (stream) hipStreamDestroy(stream);
}

hipStream_t bce_internal_stream(bce_ctx* c) { return c->stream; }
void** bce_internal_comm_slot(bce_ctx* c) { return &c->rccl_comm; }
int bce_internal_device(bce_ctx* c) { return c->device; }

int bce_set_error(bce_ctx* c, int code, const char* msg) {  // for the other translation units of the library (keyfile.cpp)
    if (c) c->err = msg ? msg : "";
    return code;
}

const char* bce_last_error(const bce_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int bce_get_params(const bce_ctx* c, uint64_t out[BCE_P_COUNT]) {
    if (!c || !out) return BCE_ERR_ARG;
    out[BCE_P_n] = c->n; out[BCE_P_N] = c->N; out[BCE_P_q] = c->q; out[BCE_P_Q] = c->Q; out[BCE_P_qKS] = c->qKS;
    out[BCE_P_baseKS] = c->baseKS; out[BCE_P_dKS] = c->dKS; out[BCE_P_baseG] = c->baseG; out[BCE_P_dG] = c->dG;
    out[BCE_P_baseR] = c->baseR; out[BCE_P_dR] = c->dR; out[BCE_P_method] = (u64)c->method; out[BCE_P_psi] = c->psi;
    return BCE_OK;
}

uint64_t bce_bsk_words(const bce_ctx* c) { return c ? rgsw_rows_total(c) * 2 * c->N : 0; }
uint64_t bce_ksk_words(const bce_ctx* c) { return c ? (u64)c->N * c->baseKS * c->dKS * (c->n + 1) : 0; }

int bce_keygen(bce_ctx* c, const uint8_t seed_in[32]) {
    if (!c) return BCE_ERR_ARG;
    uint8_t fresh[32];
    const uint8_t* seed = seed_in;
    if (!seed) {  // cc.KeyGen() of the reference: keys from the system's entropy, never from a constant
        if (!os_entropy(fresh)) return c->fail(BCE_ERR_STATE, "bce_keygen: no entropy source (getrandom and /dev/urandom failed)");
        seed = fresh;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = alloc_keys(c);
    if (rc) return rc;
    std::memcpy(c->keys().seed, seed, 32);
    const u32 n = c->n, N = c->N;
    const GaussSampler gauss(3.19);
    c->keys().s.resize(n);
    c->keys().z.resize(N);
    { ChaChaStream st(seed, kDomSK, 0); for (u32 i = 0; i < n; ++i) c->keys().s[i] = draw_ternary(st); }
    { ChaChaStream st(seed, kDomZ, 0); for (u32 i = 0; i < N; ++i) c->keys().z[i] = draw_ternary(st); }
    if ((rc = upload_secret(c))) return rc;

    KeygenDev D;
    KeygenParams kp{};
    if ((rc = keygen_params(c, gauss, D, kp))) return rc;
    // LWE key-switching key: K[i][v][j] = LWE_s(z_i * v * baseKS^j) mod qKS, sampled on the device straight into
    // the padded row layout the tail kernel gathers from
    {
        const u64 rows = (u64)N * c->baseKS * c->dKS;
        HIP_TRY(c, hipMemsetAsync(c->keys().d_ksk.get(), 0, rows * c->P.ksk_stride * (c->P.ksk_u16 ? 2 : 4), c->stream));
        HIP_TRY(c, launch_gen_ksk_rows(kp, rows, c->keys().d_ksk.get(), c->P.ksk_u16 ? 1 : 0, c->stream));
    }
    rc = keygen_bsk(c, kp, D);
    if (!rc) rc = bsk_words_to_kernel_layout(c);
    if (rc) return rc;
    c->keys().have_keys = true;
    return BCE_OK;
}

static int import_keys_impl(bce_ctx* c, const int32_t* s, const int32_t* z, const uint64_t* bsk, uint64_t bsk_words,
                            const uint32_t* ksk, uint64_t ksk_words, bool evaluation_form);

int bce_import_keys(bce_ctx* c, const int32_t* s, const int32_t* z, const uint64_t* bsk, uint64_t bsk_words,
                    const uint32_t* ksk, uint64_t ksk_words) {
    return import_keys_impl(c, s, z, bsk, bsk_words, ksk, ksk_words, false);
}

int bce_import_keys_eval(bce_ctx* c, const int32_t* s, const int32_t* z, const uint64_t* bsk_eval, uint64_t bsk_words,
                         const uint32_t* ksk, uint64_t ksk_words) {
    return import_keys_impl(c, s, z, bsk_eval, bsk_words, ksk, ksk_words, true);
}

static int import_keys_impl(bce_ctx* c, const int32_t* s, const int32_t* z, const uint64_t* bsk, uint64_t bsk_words,
                            const uint32_t* ksk, uint64_t ksk_words, bool evaluation_form) {
    if (!c || !s || !bsk || !ksk) return c ? c->fail(BCE_ERR_ARG, "null key pointer") : BCE_ERR_ARG;
    if (bsk_words != bce_bsk_words(c) || ksk_words != bce_ksk_words(c)) return c->fail(BCE_ERR_ARG, "key sizes do not match the parameter set");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = alloc_keys(c);
    if (rc) return rc;
    c->keys().s.assign(s, s + c->n);
    if (z) c->keys().z.assign(z, z + c->N); else c->keys().z.clear();
    std::memset(c->keys().seed, 0, sizeof c->keys().seed);   // imported keys have no generation seed
    if ((rc = upload_secret(c))) return rc;
    {   // words -> device words, chunked; coefficient-domain words are then transformed in place on the device
        // (evaluation-form words arrive in the engine's own order: OpenFHE's bit-reversed CT order for the minimal
        // primitive 2N-th root, bce_get_params()[BCE_P_psi])
        const u64 chunk = (u64)64 << 20;
        for (u64 o = 0; o < bsk_words; o += chunk) {
            const u64 cnt = std::min(chunk, bsk_words - o);
            for (u64 i = 0; i < cnt; ++i)
                if (bsk[o + i] >= c->Q) return c->fail(BCE_ERR_ARG, "bsk word %llu not reduced mod Q", (unsigned long long)(o + i));
            if ((rc = words_to_device(c, c->keys().d_bsk.get() + o * c->wbytes, bsk + o, cnt, c->is64))) return rc;
        }
        if (!evaluation_form && (rc = dev_ntt(c, c->keys().d_bsk.get(), bsk_words / c->N, 0))) return rc;
        if ((rc = bsk_words_to_kernel_layout(c))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    rc = upload_ksk(c, ksk);
    if (rc) return rc;
    c->keys().have_keys = true;
    return BCE_OK;
}

int bce_export_sk(const bce_ctx* c, int32_t* s, int32_t* z) {
    if (!c || !c->keys().have_keys) return BCE_ERR_NO_KEYS;   // (c->keys(): the selected set, like every call without a map)
    if (s) std::memcpy(s, c->keys().s.data(), c->n * sizeof(int32_t));
    if (z && !c->keys().z.empty()) std::memcpy(z, c->keys().z.data(), c->N * sizeof(int32_t));
    return BCE_OK;
}

static int export_bsk_impl(bce_ctx* c, uint64_t* bsk, bool evaluation_form);
int bce_export_bsk(bce_ctx* c, uint64_t* bsk) { return export_bsk_impl(c, bsk, false); }

static int export_bsk_impl(bce_ctx* c, uint64_t* bsk, bool evaluation_form) {
    if (!c || !bsk) return BCE_ERR_ARG;
    if (!c->keys().have_keys) return c->fail(BCE_ERR_NO_KEYS, "no keys");
    HIP_TRY(c, hipSetDevice(c->device));
    const u64 words = bce_bsk_words(c);
    const u64 per_rgsw = 4ull * c->dG;  // polynomials of one RGSW ciphertext: chunks hold whole ciphertexts (un-folding works per ciphertext)
    const u64 chunk_polys = std::max<u64>(1, ((u64)256 << 20) / ((u64)c->N * c->wbytes) / per_rgsw) * per_rgsw;
    DevBuf<char> tmp;
    HIP_TRY(c, tmp.alloc(chunk_polys * c->N * c->wbytes));
    void* const d_tmp = tmp.get();
    for (u64 p0 = 0; p0 < words / c->N; p0 += chunk_polys) {
        const u64 cnt = std::min(chunk_polys, words / c->N - p0), w = cnt * c->N;
        const char* src = c->keys().d_bsk.get() + p0 * c->N * c->wbytes;
        HIP_TRY(c, hipMemcpyAsync(d_tmp, src, w * c->wbytes, hipMemcpyDeviceToDevice, c->stream));
        if (c->P.fp64) HIP_TRY(c, launch_words_u64_f64(static_cast<u64*>(d_tmp), w, 0, c->stream));  // doubles -> u64 words
        if (c->P.fold) HIP_TRY(c, launch_fold_gadget(c->P, d_tmp, cnt / (4ull * c->dG), -1, c->stream));   // rows l >= 1 += B^l row 0
        if (!evaluation_form) { int rc = dev_ntt(c, d_tmp, cnt, 1); if (rc) return rc; }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (const int rc = words_from_device(c, bsk + p0 * c->N, d_tmp, w, c->is64)) return rc;
    }
    return BCE_OK;
}

int bce_export_bsk_eval(bce_ctx* c, uint64_t* bsk) { return export_bsk_impl(c, bsk, true); }

int bce_export_ksk(bce_ctx* c, uint32_t* ksk) {
    if (!c || !ksk) return BCE_ERR_ARG;
    if (!c->keys().have_keys) return c->fail(BCE_ERR_NO_KEYS, "no keys");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rows = (size_t)c->N * c->baseKS * c->dKS, W = c->n + 1, S = c->P.ksk_stride;
    if (c->P.ksk_u16) {
        std::vector<uint16_t> buf(rows * S);
        HIP_TRY(c, hipMemcpy(buf.data(), c->keys().d_ksk.get(), buf.size() * 2, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < rows; ++r)
            for (size_t k = 0; k < W; ++k) ksk[r * W + k] = buf[r * S + k];
    } else {
        std::vector<u32> buf(rows * S);
        HIP_TRY(c, hipMemcpy(buf.data(), c->keys().d_ksk.get(), buf.size() * 4, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < rows; ++r) std::memcpy(&ksk[r * W], &buf[r * S], W * 4);
    }
    return BCE_OK;
}

int bce_pool_reserve(bce_ctx* c, uint32_t slots) {
    if (!c) return BCE_ERR_ARG;
    if (slots <= c->pool_slots) return BCE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DevBuf<u32> np;
    HIP_TRY(c, np.alloc((size_t)slots * c->P.pool_stride));
    HIP_TRY(c, hipMemset(np.get(), 0, (size_t)slots * c->P.pool_stride * 4));
    if (c->d_pool.get()) HIP_TRY(c, hipMemcpy(np.get(), c->d_pool.get(), (size_t)c->pool_slots * c->P.pool_stride * 4, hipMemcpyDeviceToDevice));
    // published only now, zeroed and holding the old contents: a failure above left the old pool in place
    c->d_pool = std::move(np);
    c->pool_slots = slots;
    c->P.pool = c->d_pool.get();
    return BCE_OK;
}

uint32_t bce_pool_slots(const bce_ctx* c) { return c ? c->pool_slots : 0; }

static int pool_pack(bce_ctx* c, const uint32_t* slots, uint32_t count, void* dev, int to_pool);

int bce_lwe_write(bce_ctx* c, const uint32_t* slots, uint32_t count, const uint64_t* cts) {
    if (!c || !slots || !cts) return BCE_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t W = c->n + 1;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<u32> buf;
    for (u32 i = 0; i < count;) {
        u32 run = 1;  // coalesce runs of consecutive slots into one copy
        while (i + run < count && slots[i + run] == slots[i] + run) ++run;
        if ((u64)slots[i] + run > c->pool_slots) return c->fail(BCE_ERR_POOL, "slot %u outside the pool", slots[i] + run - 1);
        buf.resize((size_t)run * W);
        for (size_t k = 0; k < (size_t)run * W; ++k) {
            const u64 v = cts[(size_t)i * W + k];
            if (v >= c->q) return c->fail(BCE_ERR_ARG, "ciphertext word not reduced mod q");
            buf[k] = (u32)v;
        }
        HIP_TRY(c, hipMemcpy(c->d_pool.get() + (size_t)slots[i] * c->P.pool_stride, buf.data(), buf.size() * 4, hipMemcpyHostToDevice));
        i += run;
    }
    return BCE_OK;
}

int bce_lwe_read(bce_ctx* c, const uint32_t* slots, uint32_t count, uint64_t* cts) {
    if (!c || !slots || !cts) return BCE_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t W = c->n + 1;
    { const int rc = sync_stream(c); if (rc) return rc; }
    // one bulk copy when the request is dense enough, else per slot
    u32 lo = ~0u, hi = 0;
    for (u32 i = 0; i < count; ++i) {
        if (slots[i] >= c->pool_slots) return c->fail(BCE_ERR_POOL, "slot %u outside the pool", slots[i]);
        lo = std::min(lo, slots[i]);
        hi = std::max(hi, slots[i]);
    }
    if (count == 0) return BCE_OK;
    std::vector<u32> buf;
    if ((u64)(hi - lo + 1) <= 4ull * count + 64) {
        buf.resize((size_t)(hi - lo + 1) * W);
        HIP_TRY(c, hipMemcpy(buf.data(), c->d_pool.get() + (size_t)lo * W, buf.size() * 4, hipMemcpyDeviceToHost));
        for (u32 i = 0; i < count; ++i)
            for (size_t k = 0; k < W; ++k) cts[i * W + k] = buf[(size_t)(slots[i] - lo) * W + k];
    } else {
        // scattered slots (the outputs of K instances sit one pool stride apart): gather on the device, one copy
        const size_t words = (size_t)count * W;
        const size_t cap = std::max(words, (size_t)64 * W);   // (the stream was synchronised above)
        HIP_TRY(c, c->d_io.grow(words, cap, nullptr));
        HIP_TRY(c, c->h_io.grow(words, cap, nullptr));
        { const int rc = pool_pack(c, slots, count, c->d_io.get(), 0); if (rc) return rc; }
        HIP_TRY(c, hipMemcpyAsync(c->h_io.get(), c->d_io.get(), words * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < words; ++k) cts[k] = c->h_io.get()[k];
    }
    return BCE_OK;
}

int bce_encrypt_bits(bce_ctx* c, const uint8_t* bits, const uint32_t* slots, uint32_t count, uint64_t enc_index_base,
                     int mode) {
    if (!c || !bits || !slots) return BCE_ERR_ARG;
    if (!c->keys().have_keys) return c->fail(BCE_ERR_NO_KEYS, "no keys");
    const u32 n = c->n;
    const u64 q = c->q;
    const size_t W = n + 1;
    const GaussSampler gauss(3.19);
    std::vector<u64> cts((size_t)count * W);
    if (!c->enc_deterministic) {
        // default: the caller's index is ignored; the context's own counter names the stream and never repeats
        if (!c->enc_seed_ok) return c->fail(BCE_ERR_STATE, "no entropy source for encryption randomness (getrandom and /dev/urandom failed)");
        enc_index_base = c->enc_counter;
        c->enc_counter += count;
    }
    for (u32 i = 0; i < count; ++i) {
        ChaChaStream st(c->enc_seed, kDomENC, enc_index_base + i);
        u64* ct = &cts[(size_t)i * W];
        u128 acc = 0;
        for (u32 k = 0; k < n; ++k) {
            ct[k] = draw_uniform(st, q);
            acc += (u128)ct[k] * lift_signed(c->keys().s[k], q);
        }
        u64 e = lift_signed(gauss.draw(st), q);
        ct[n] = (u64)((acc + e + (u64)(bits[i] % 4) * (q / 4)) % q);
    }
    int rc = bce_lwe_write(c, slots, count, cts.data());
    if (rc) return rc;
    if (mode == BCE_BOOTSTRAPPED) {
        std::vector<bce_gate_desc> d(count);
        for (u32 i = 0; i < count; ++i) d[i] = bce_gate_desc{BCE_OP_REFRESH, slots[i], slots[i], slots[i], 0, 0};
        return bce_eval_gates(c, count, d.data());
    }
    return BCE_OK;
}

int bce_set_encrypt_seed(bce_ctx* c, const uint8_t seed[32]) {
    if (!c) return BCE_ERR_ARG;
    if (seed) {
        std::memcpy(c->enc_seed, seed, 32);
        c->enc_seed_ok = true;
        c->enc_deterministic = true;
    } else {
        c->enc_deterministic = false;
        c->enc_counter = 0;
        c->enc_seed_ok = os_entropy(c->enc_seed);
        if (!c->enc_seed_ok) return c->fail(BCE_ERR_STATE, "no entropy source (getrandom and /dev/urandom failed)");
    }
    return BCE_OK;
}

int bce_decrypt_bits(bce_ctx* c, const uint32_t* slots, uint32_t count, uint8_t* bits) {
    return bce_decrypt_bits_keyed(c, slots, count, nullptr, bits);
}

int bce_decrypt_bits_keyed(bce_ctx* c, const uint32_t* slots, uint32_t count, const uint32_t* keyset_of_slot, uint8_t* bits) {
    if (!c || !slots || !bits) return BCE_ERR_ARG;
    if (const int rc = keyset_of_slot ? need_keys_of_map(c, "bce_decrypt_bits_keyed", keyset_of_slot, count) : need_keys(c)) return rc;
    const u32 n = c->n;
    const u64 q = c->q;
    const size_t W = n + 1;
    std::vector<u64> cts((size_t)count * W);
    int rc = bce_lwe_read(c, slots, count, cts.data());
    if (rc) return rc;
    for (u32 i = 0; i < count; ++i) {
        const u64* ct = &cts[(size_t)i * W];
        const std::vector<int32_t>& s = keyset_of_slot ? c->keysets[keyset_of_slot[i]]->s : c->keys().s;
        // <a, s> over the integers with s in {-1, 0, 1}: |sum| < n q, reduced once (same residue as the reference's
        // mod-q accumulation, lwe-pke.cpp Decrypt)
        u64 inner_q;
        if (q <= (1ull << 24)) {
            int64_t inner = 0;
            for (u32 k = 0; k < n; ++k) inner += (int64_t)ct[k] * s[k];
            inner_q = (u64)(((inner % (int64_t)q) + (int64_t)q) % (int64_t)q);
        } else {
            u128 inner = 0;
            for (u32 k = 0; k < n; ++k) inner += (u128)ct[k] * lift_signed(s[k], q);
            inner_q = (u64)(inner % q);
        }
        u64 r = (ct[n] + q - inner_q) % q;
        r = (r + q / 8) % q;
        bits[i] = (uint8_t)((4 * r) / q);
    }
    return BCE_OK;
}

int bce_eval_gates(bce_ctx* c, uint32_t n_desc, const bce_gate_desc* descs) {
    if (!c) return BCE_ERR_ARG;
    return eval_impl(c, n_desc, descs, 1, 0, nullptr, nullptr, nullptr);
}

int bce_eval_gates_strided(bce_ctx* c, uint32_t n_desc, const bce_gate_desc* descs, uint32_t instances,
                           uint32_t slot_stride) {
    if (!c) return BCE_ERR_ARG;
    return eval_impl(c, n_desc, descs, instances, slot_stride, nullptr, nullptr, nullptr);
}

int bce_eval_gates_keyed(bce_ctx* c, uint32_t n_desc, const bce_gate_desc* descs, uint32_t instances, uint32_t slot_stride,
                         const uint32_t* keyset_of_instance) {
    if (!c) return BCE_ERR_ARG;
    return eval_impl(c, n_desc, descs, instances, slot_stride, nullptr, nullptr, nullptr, keyset_of_instance);
}

// ---- key sets (include/bce_gpu.h, "key sets") --------------------------------------------------------------------------
int bce_keyset_add(bce_ctx* c, uint32_t* id) {
    if (!c || !id) return BCE_ERR_ARG;
    for (u32 i = 1; i < BCE_MAX_KEYSETS; ++i)
        if (!c->keysets[i]) {
            c->keysets[i] = std::make_unique<KeySet>();
            *id = i;
            return BCE_OK;
        }
    return c->fail(BCE_ERR_ARG, "bce_keyset_add: the context holds %d key sets already", BCE_MAX_KEYSETS);
}

int bce_keyset_select(bce_ctx* c, uint32_t id) {
    if (!c) return BCE_ERR_ARG;
    if (id >= BCE_MAX_KEYSETS || !c->keysets[id]) return c->fail(BCE_ERR_ARG, "bce_keyset_select: key set %u does not exist", id);
    c->selected = c->P.keyset_sel = id;
    return BCE_OK;
}

int bce_keyset_drop(bce_ctx* c, uint32_t id) {
    if (!c) return BCE_ERR_ARG;
    if (id >= BCE_MAX_KEYSETS || !c->keysets[id]) return c->fail(BCE_ERR_ARG, "bce_keyset_drop: key set %u does not exist", id);
    if (id == 0) return c->fail(BCE_ERR_ARG, "bce_keyset_drop: key set 0 lives as long as the context");
    if (id == c->selected) return c->fail(BCE_ERR_ARG, "bce_keyset_drop: key set %u is the selected one", id);
    if (plan_names_keyset(c, id)) return c->fail(BCE_ERR_STATE, "bce_keyset_drop: a live plan was created with a map that names key set %u", id);
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = sync_stream(c)) return rc;
    const KeySetDev none{};
    HIP_TRY(c, hipMemcpy(c->d_keysets.get() + id, &none, sizeof none, hipMemcpyHostToDevice));
    c->keysets[id].reset();
    return BCE_OK;
}

uint32_t bce_keyset_count(const bce_ctx* c) {
    u32 count = 0;
    for (u32 i = 0; c && i < BCE_MAX_KEYSETS; ++i) count += c->keysets[i] ? 1 : 0;
    return count;
}
uint32_t bce_keyset_selected(const bce_ctx* c) { return c ? c->selected : 0; }

int bce_synchronize(bce_ctx* c) {
    if (!c) return BCE_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return sync_stream(c);
}

int bce_timing_reset(bce_ctx* c) {
    if (!c) return BCE_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drain_timing(c);
    c->timing = bce_timing{};
    return BCE_OK;
}

int bce_timing_set_events(bce_ctx* c, int on) {
    if (!c) return BCE_ERR_ARG;
    c->events_on = on != 0;
    return BCE_OK;
}

int bce_timing_get(bce_ctx* c, bce_timing* out) {
    if (!c || !out) return BCE_ERR_ARG;
    const int rc = sync_stream(c);
    drain_timing(c);
    *out = c->timing;
    return rc;
}

uint32_t bce_forward_transforms_per_step(const bce_ctx* c) { return c ? forward_transforms_per_step(c->P) : 0; }
uint32_t bce_forward_units(const bce_ctx* c) { return c ? c->P.fwd_units : 0; }
uint32_t bce_forward_mfma(const bce_ctx* c) { return c ? c->P.fwd_mfma : 0; }
uint32_t bce_lazy_arithmetic(const bce_ctx* c) { return c ? c->P.lazy : 0; }
int bce_forward_mfma_tables(uint64_t Q, uint32_t N, uint32_t gBits, uint32_t dG, uint64_t* psi, uint32_t* M6, uint32_t* C, uint32_t* table,
                            uint32_t* w14, uint64_t* bounds) {
    const FwdMfmaTables T = build_fwd_mfma_tables(Q, N, gBits, dG);
    if (T.M6.empty()) return 0;   // not this class of parameters: nothing was built
    if (psi) *psi = T.psi;
    if (M6) std::copy(T.M6.begin(), T.M6.end(), M6);
    if (C) std::copy(T.C.begin(), T.C.end(), C);
    if (table) std::copy(T.table.begin(), T.table.end(), table);
    if (w14) { w14[0] = T.w14; w14[1] = T.w14s; }
    if (bounds) { bounds[0] = T.limb_sum_max; bounds[1] = T.lo_max; bounds[2] = T.hi_max; bounds[3] = T.out_max; }
    return T.ok ? 1 : -1;         // -1: built, but a bound fails for this Q
}

int bce_launch_capacity(const bce_ctx* c, uint32_t* lone, uint32_t* full) {
    if (!c || !lone || !full) return BCE_ERR_ARG;
    launch_capacity(c->P, lone, full);
    return BCE_OK;
}

static int report_derived(const CtxParams& cp, uint64_t* out, const char** message) {
    if (message) *message = cp.status.message;
    if (!out) return BCE_ERR_ARG;
    std::fill(out, out + BCE_D_COUNT, 0);
    if (cp.status.code != BCE_OK) return cp.status.code;
    params_report(cp, out);
    out[BCE_D_dag_lds_bytes] = cp.P.is64 ? 0 : bootstrap_dag_lds_bytes(cp.P, 4);
    return BCE_OK;
}

int bce_params_derive(uint32_t n, uint32_t N, uint64_t q, uint64_t Q, uint64_t qKS, uint32_t baseKS, uint32_t baseG, uint32_t baseR,
                      int method, uint32_t cu_count, uint64_t out[BCE_D_COUNT], const char** message) {
    return report_derived(derive_params(Shape{n, N, q, Q, qKS, baseKS, baseG, baseR, method}, read_ctx_knobs(), cu_count), out, message);
}

int bce_params_derive_set(int paramset, int method, uint32_t cu_count, uint64_t out[BCE_D_COUNT], const char** message) {
    Shape s;
    if (!tabulated_shape(paramset, method, s)) { if (message) *message = "unknown parameter set"; return BCE_ERR_ARG; }
    return report_derived(derive_params(s, read_ctx_knobs(), cu_count), out, message);
}

int bce_bytes_per_bootstrap_parts(const bce_ctx* c, uint64_t out[3]) {
    if (!c || !out) return BCE_ERR_ARG;
    bytes_per_bootstrap_parts(c->P, out);
    return BCE_OK;
}

uint64_t bce_bytes_per_bootstrap(const bce_ctx* c) {
    uint64_t parts[3];
    return bce_bytes_per_bootstrap_parts(c, parts) == BCE_OK ? parts[0] + parts[1] + parts[2] : 0;
}

int bce_debug_eval_stages(bce_ctx* c, uint32_t n_desc, const bce_gate_desc* descs, uint64_t* acc, uint64_t* lweN,
                          uint64_t* ks) {
    if (!c) return BCE_ERR_ARG;
    for (u32 i = 0; i < n_desc; ++i)
        if (!desc_kind(descs[i].op).boot()) return c->fail(BCE_ERR_ARG, "staged outputs need bootstrapped ops only");
    return eval_impl(c, n_desc, descs, 1, 0, acc, lweN, ks);
}

// The tail of EvalBinGate alone (transpose + extract, ModSwitch Q -> qKS, KeySwitch, ModSwitch qKS -> q) on accumulators
// the CALLER supplies: what tools/openfhe_export/compare.py replays OpenFHE's LWEEncryptionScheme::ModSwitch / KeySwitch
// records on, so that a mismatch in a gate vector can be told apart from one in the tail.  Runs the separate tail kernels.
int bce_debug_tail(bce_ctx* c, uint32_t count, const uint64_t* acc, const uint32_t* out_slots, uint64_t* lweN, uint64_t* ks) {
    if (!c || !acc || !out_slots) return BCE_ERR_ARG;
    if (count == 0) return BCE_OK;
    if (const int rc = need_keys(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t words = (size_t)count * 2 * c->N;
    for (size_t i = 0; i < words; ++i)
        if (acc[i] >= c->Q) return c->fail(BCE_ERR_ARG, "accumulator word not reduced mod Q");
    std::vector<bce_gate_desc> d(count);
    for (u32 i = 0; i < count; ++i) {
        if (out_slots[i] >= c->pool_slots) return c->fail(BCE_ERR_POOL, "slot %u outside the pool", out_slots[i]);
        d[i] = bce_gate_desc{BCE_AND, out_slots[i], out_slots[i], out_slots[i], 0, 0};
    }
    DevBuf<char> d_in;
    DevBuf<u32> d_lweN, d_ks;
    DevBuf<u64> d_partial;
    HIP_TRY(c, d_in.alloc(words * c->wbytes));
    HIP_TRY(c, d_lweN.alloc((size_t)count * (c->N + 1)));
    HIP_TRY(c, d_ks.alloc((size_t)count * (c->n + 1)));
    HIP_TRY(c, d_partial.alloc(std::max<size_t>(1, tail_partial_words(c->P, count))));
    int rc = words_to_device(c, d_in.get(), acc, words, c->is64);
    if (rc) return rc;
    StagedUpload* slot = nullptr;
    if ((rc = stage_descs(c, d.data(), count, &slot))) return rc;
    HIP_TRY(c, launch_tail(c->P, descs_of(slot), count, 1, 0, d_in.get(), d_partial.get(), d_lweN.get(), d_ks.get(), c->stream, LaunchEvents{}));
    slot->mark(c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (lweN && (rc = words_from_device(c, lweN, d_lweN.get(), (size_t)count * (c->N + 1), false))) return rc;
    if (ks && (rc = words_from_device(c, ks, d_ks.get(), (size_t)count * (c->n + 1), false))) return rc;
    return BCE_OK;
}

uint32_t bce_debug_tail_split(const bce_ctx* c, uint32_t count) { return c && count ? tail_split(c->P, count) : 0; }

static int pool_pack(bce_ctx* c, const uint32_t* slots, uint32_t count, void* dev, int to_pool) {
    if (!c || !slots || !dev) return BCE_ERR_ARG;
    if (count == 0) return BCE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<bce_gate_desc> d(count);
    for (u32 i = 0; i < count; ++i) {
        if (slots[i] >= c->pool_slots) return c->fail(BCE_ERR_POOL, "slot %u outside the pool", slots[i]);
        d[i] = bce_gate_desc{BCE_OP_COPY, slots[i], slots[i], slots[i], 0, 0};
    }
    StagedUpload* slot = nullptr;
    int rc = stage_descs(c, d.data(), count, &slot);
    if (rc) return rc;
    HIP_TRY(c, launch_pool_pack(c->P, descs_of(slot), count, (u32*)dev, to_pool, c->stream));
    slot->mark(c->stream);
    return BCE_OK;
}

int bce_pool_gather(bce_ctx* c, const uint32_t* slots, uint32_t count, void* dev_dst) {
    return pool_pack(c, slots, count, dev_dst, 0);
}
int bce_pool_scatter(bce_ctx* c, const uint32_t* slots, uint32_t count, const void* dev_src) {
    return pool_pack(c, slots, count, const_cast<void*>(dev_src), 1);
}

int bce_debug_ntt(bce_ctx* c, uint64_t* polys, uint32_t count, int inverse) {
    if (!c || !polys) return BCE_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t words = (size_t)count * c->N;
    for (size_t i = 0; i < words; ++i)
        if (polys[i] >= c->Q) return c->fail(BCE_ERR_ARG, "poly word not reduced mod Q");
    DevBuf<char> d;
    HIP_TRY(c, d.alloc(words * c->wbytes));
    int rc = words_to_device(c, d.get(), polys, words, c->is64);
    if (!rc) rc = dev_ntt(c, d.get(), count, inverse);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return words_from_device(c, polys, d.get(), words, c->is64);
}

}  // extern "C"
