// engine_internal.hpp -- what the three files of the engine share: the context (engine.cpp) and the helpers that its
// schedules (engine_plan.cpp: bce_plan and the device-side checks; engine_dag.cpp: bce_dag) use as well.  Not a public header.
#pragma once
#include <hip/hip_runtime_api.h>

#include <array>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/bce_gpu.h"
#include "devmem.hpp"
#include "kernels.hpp"

struct bce_plan;
struct bce_dag;

namespace bce {

struct EventPair { hipEvent_t a, b; int kind; };

// Contexts that exist, and (bce_ctx::plans, ::dags, under the same mutex) the schedules each one owns.  A bce_plan / bce_dag
// belongs to the context it was created on: the context's destruction releases whatever its callers left behind, and
// bce_plan_destroy / bce_dag_destroy on a context that is already gone (a Circuit destroyed after its engine) is a no-op
// instead of a read of freed memory.
extern std::mutex g_live_mu;
extern std::unordered_set<const bce_ctx*> g_live;

// What the kernels of a captured plan hold by value (bce_plan_run): the context's device pointers and kernel choices
struct CaptureSnapshot {
    std::array<const void*, 4> ptrs{};
    std::array<u32, 4> flags{};   // the last one: the selected key set (0 for a plan with a key-set map: it does not follow the selection)
    bool operator==(const CaptureSnapshot& o) const { return ptrs == o.ptrs && flags == o.flags; }
};

// The key material of one client (include/bce_gpu.h, "key sets").  A context holds up to BCE_MAX_KEYSETS of them; everything
// derived from the parameters alone (tables, fold decision, lazy bounds, pool) stays per context.  The three device buffers
// are allocated once per set and never reallocated: the context's device table (bce_ctx::d_keysets) holds their addresses.
struct KeySet {
    DevBuf<char> d_bsk;          // u32 words (Q < 2^28), u64 words (is64) or doubles (fp64), in the kernels' layout
    DevBuf<char> d_ksk;
    DevBuf<int8_t> d_s8;         // the LWE secret as the device-side checks read it: int8[n padded to 64]
    u64 bsk_polys = 0;
    bool have_keys = false;
    std::vector<int32_t> s, z;   // host secrets
    uint8_t seed[32] = {0};      // key-generation seed (bce_keygen); zero after bce_import_keys
};

}  // namespace bce

struct bce_ctx {
    using u32 = bce::u32;
    using u64 = bce::u64;
    template <class T, bool Pinned = false> using DevBuf = bce::DevBuf<T, Pinned>;
    using StagedUpload = bce::StagedUpload;

    std::unordered_set<bce_plan*> plans;
    std::unordered_set<bce_dag*> dags;
    // parameters
    u32 n = 0, N = 0, logN = 0;
    u64 q = 0, Q = 0, qKS = 0, psi = 0;
    u32 baseKS = 0, dKS = 0, baseG = 0, gBits = 0, dG = 0, baseR = 0, dR = 0;
    int method = 0, device = 0;
    std::string err;

    // every device / pinned buffer below owns its memory (devmem.hpp); bce_ctx_destroy keeps what has an order
    hipStream_t stream = nullptr;
    bce::DevParams P{};   // its pointers mirror the owning members below, set where those are allocated
    // device tables / keys
    DevBuf<uint2> d_twf;
    DevBuf<u32> d_fwd_mfma, d_psi, d_psi_r2, d_xcd_gate;
    DevBuf<ulonglong2> d_tw64;
    DevBuf<double2> d_tw64d;      // (w, w / Q) for the double-precision formulation
    bool is64 = false;
    size_t wbytes = 4;
    // key sets: set 0 exists from creation; a call that takes no key-set map acts on the selected one
    std::array<std::unique_ptr<bce::KeySet>, BCE_MAX_KEYSETS> keysets;
    u32 selected = 0;             // mirrored in P.keyset_sel
    DevBuf<bce::KeySetDev> d_keysets;   // [BCE_MAX_KEYSETS] what the kernels read (P.keysets); one allocation per context
    bce::KeySet& keys() { return *keysets[selected]; }
    const bce::KeySet& keys() const { return *keysets[selected]; }
    // Encryption randomness is independent of the key seed: drawn from OS entropy when the context is created,
    // consumed through a per-context counter that only moves forward, so no (a, e) pair is ever reused.
    // bce_set_encrypt_seed() switches to the deterministic, caller-indexed streams of the parity tests.
    uint8_t enc_seed[32] = {0};
    bool enc_seed_ok = false, enc_deterministic = false;
    uint64_t enc_counter = 0;
    void* rccl_comm = nullptr;   // ncclComm_t of the in-library all-gather (rccl_xchg.cpp), if enabled
    // pool
    DevBuf<u32> d_pool;
    u32 pool_slots = 0;
    // work buffers
    DevBuf<char> d_acc;             // accumulators of the largest launch so far
    DevBuf<u64> d_tail_partial;     // partial key-switch sums (kernels.hip, k_tail_gather)
    bool events_on = true;                 // per-launch HIP events (bce_timing_set_events): off = counters only, no event packets between dependent kernels
    DevBuf<u32> d_io;               // staging of bce_lwe_read for scattered slots (device gather + one pinned copy)
    DevBuf<u32, true> h_io;
    static constexpr int kRing = 4;
    StagedUpload ring[kRing];       // descriptor lists of the launches in flight (stage_descs)
    int ring_pos = 0;
    // verify mode on the device (bce_check_*): the report block followed by the mismatch log, and the staging pair of
    // bce_check_slots (slot list + expected bits); the LWE secret it decrypts with belongs to the key set (KeySet::d_s8)
    DevBuf<char> d_check_mem;
    bce_check_report* d_check() const { return reinterpret_cast<bce_check_report*>(d_check_mem.get()); }
    bce_check_entry* d_check_log() const { return reinterpret_cast<bce_check_entry*>(d_check_mem.get() + sizeof(bce_check_report)); }
    StagedUpload chk_stage;
    // timing
    std::vector<bce::EventPair> pending, free_events;
    bce_timing timing{};
    // dependency-driven runs (bce_dag_*): device copy of P, knobs, and the status words of runs not yet checked
    DevBuf<bce::DevParams> d_P;
    int dag_wg_per_cu = 0, dag_placement = 1;
    uint32_t dag_lazy_us = 20, dag_stall_ms = 4000;
    struct DagStatus { uint32_t abort, done, lazy_waits, pad; uint64_t busy_ticks, wait_ticks, gate_ticks; };
    static constexpr int kDagRuns = 32;
    DevBuf<DagStatus, true> h_dag_status;     // pinned, kDagRuns entries
    struct DagStage { bce::DevParams P; bce::DagParams D; };
    DevBuf<DagStage, true> h_dag_stage;       // pinned, kDagRuns entries: sources of the stream-ordered parameter uploads
    uint64_t dag_expected[kDagRuns] = {0};
    int dag_wps_used[kDagRuns] = {0};
    int dag_pending = 0;
    uint64_t dag_last[7] = {0, 0, 0, 0, 0, 0, 0};

    // keyed: for a plan created with a key-set map.  The keys themselves are found through P.keysets at replay.
    bce::CaptureSnapshot capture_snapshot(bool keyed) const {
        return {{P.pool, P.keysets, P.tw_f, P.psi_tab}, {P.variant, P.fuse_tail, P.fold, keyed ? 0u : selected}};
    }

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return (ctx)->fail(BCE_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

namespace bce {

inline int need_keys(bce_ctx* c) {
    if (c->keys().have_keys) return BCE_OK;
    return c->selected ? c->fail(BCE_ERR_NO_KEYS, "key set %u has no keys: bce_keygen / bce_import_keys has not been called under its selection", c->selected)
                       : c->fail(BCE_ERR_NO_KEYS, "bce_keygen / bce_import_keys has not been called");
}
// a key-set map: every id names an existing set with keys (`who` names the call in the message)
inline int need_keys_of_map(bce_ctx* c, const char* who, const u32* map, u32 instances) {
    for (u32 k = 0; k < instances; ++k) {
        if (map[k] >= BCE_MAX_KEYSETS || !c->keysets[map[k]]) return c->fail(BCE_ERR_ARG, "%s: instance %u names key set %u, which does not exist", who, k, map[k]);
        if (!c->keysets[map[k]]->have_keys) return c->fail(BCE_ERR_NO_KEYS, "%s: key set %u (instance %u) has no keys", who, map[k], k);
    }
    return BCE_OK;
}

// device copy of a host vector in a buffer that is still empty (one element at least)
template <class T>
hipError_t upload_vector(DevBuf<T>& dst, const std::vector<T>& v) {
    const hipError_t e = dst.alloc(v.empty() ? 1 : v.size());
    return e != hipSuccess ? e : hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// engine.cpp (each with its comment there)
int ensure_check(bce_ctx* c);
int ensure_acc(bce_ctx* c, size_t boots);
EventPair get_events(bce_ctx* c, int kind);
int drain_if_long(bce_ctx* c);
int sync_stream(bce_ctx* c);
int expected_are_messages(bce_ctx* c, const char* who, const uint8_t* expect, size_t count);
int launch_bootstraps(bce_ctx* c, const bce_gate_desc* dd, u32 n, u32 instances, u32 slot_stride, void* d_acc, u32* d_lweN, u32* d_ks,
                      bool timed, bool* fused_out, bool pairs, u64* d_partial = nullptr, const u32* d_map = nullptr);

// Schedules.  bce_plan_destroy / bce_dag_destroy, and the deleter of a schedule under construction: nothing to free and
// nothing to touch when the context no longer exists (it took its schedules along) or does not own `s`
inline std::unordered_set<bce_plan*>& schedules_of(bce_ctx* c, bce_plan*) { return c->plans; }
inline std::unordered_set<bce_dag*>& schedules_of(bce_ctx* c, bce_dag*) { return c->dags; }
template <class S>
void destroy_schedule(bce_ctx* c, S* s) {
    if (!s || !c) return;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        if (!g_live.count(c) || !schedules_of(c, s).erase(s)) return;
    }
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    delete s;
}
struct ScheduleDeleter {
    bce_ctx* c;
    template <class S> void operator()(S* s) const { destroy_schedule(c, s); }
};
// for bce_ctx_destroy, which has synchronised and emptied the context's sets (engine_plan.cpp, engine_dag.cpp)
void delete_leftover(bce_plan* p);
bool plan_names_keyset(bce_ctx* c, u32 id);   // engine_plan.cpp: a live plan of c was created with a map that names set id
void delete_leftover(bce_dag* g);

}  // namespace bce
