// engine_plan.cpp -- a whole step schedule at once (bce_plan; include/bce_gpu.h, "a whole step schedule at once") and verify
// mode on the device (bce_check_*, "verify mode on the device"), which shares the plan's check helpers.
#include <algorithm>
#include <cstring>
#include <memory>

#include "desc.hpp"
#include "engine_internal.hpp"

using namespace bce;

struct bce_plan {
    std::vector<u32> off, cnt;                 // step s = descriptors [off[s], off[s] + cnt[s])
    std::vector<uint8_t> pairs;                // step s holds at least one pair descriptor (BCE_PAIR)
    u32 instances = 0, slot_stride = 0, slot_base = 0;
    u32 max_step = 0;                          // descriptors of the largest step
    u64 boots_per_run = 0;
    DevBuf<bce_gate_desc> d_descs;             // all steps, resident; a keyed plan's map sits behind them in the same block
    std::vector<u32> keymap;                   // bce_plan_create_keyed: the key set of every instance (empty: the plan follows the selection)
    const u32* d_map = nullptr;                // its device copy inside d_descs, or null
    // captured form (bce_plan_run): its own accumulator / partial-sum scratch, so that nothing the graph points to is ever
    // re-allocated by other calls on the context.  d_descs, d_acc, d_partial, d_chk_slots and `expect` never move while
    // `exec` exists: each is allocated once, the check lists only after bce_plan_set_checks dropped the capture.
    DevBuf<char> d_acc;
    DevBuf<u64> d_partial;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    u64 fused_launches = 0;
    // the captured kernels hold the context's device pointers and kernel choices by value: what they were at capture
    CaptureSnapshot captured;
    // device-side checks (bce_plan_set_checks): step s checks the slots [chk_off[s], chk_off[s] + chk_cnt[s]) of d_chk_slots
    // against the same range of every instance's row of `expect` ([instances][chk_total], one fixed buffer: the captured
    // graph points into it; bce_plan_set_expected refills it through its pinned half)
    std::vector<u32> chk_off, chk_cnt;
    u32 chk_total = 0;
    int chk_repair = 0;
    bool expected_set = false;
    DevBuf<u32> d_chk_slots;
    StagedUpload expect;
    const uint8_t* d_expect() const { return static_cast<const uint8_t*>(expect.device()); }

    void drop_capture() {
        if (exec) { hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph) { hipGraphDestroy(graph); graph = nullptr; }
    }
    ~bce_plan() { drop_capture(); }   // the graph goes before the buffers it points to
};

void bce::delete_leftover(bce_plan* p) { delete p; }
bool bce::plan_names_keyset(bce_ctx* c, u32 id) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (const bce_plan* p : c->plans)
        if (std::find(p->keymap.begin(), p->keymap.end(), id) != p->keymap.end()) return true;
    return false;
}

namespace {
void plan_free_checks(bce_plan* p) {
    p->d_chk_slots.reset();
    p->expect.reset();
    p->chk_off.clear(); p->chk_cnt.clear();
    p->chk_total = 0; p->expected_set = false;
}
// the checks of plan step s, after its kernels (no allocation, no synchronisation: also runs under stream capture)
int plan_check_step(bce_ctx* c, const bce_plan* p, size_t s) {
    if (!p->chk_total || !p->chk_cnt[s]) return BCE_OK;
    HIP_TRY(c, launch_lwe_check(c->P, p->d_chk_slots.get() + p->chk_off[s], p->d_expect() + p->chk_off[s], p->chk_cnt[s], p->chk_total,
                                p->instances, p->slot_stride, p->chk_repair, (u32)s, c->d_check(), c->d_check_log(), c->stream));
    return BCE_OK;
}
// every checked slot, at every instance (span = the distance of the last instance's copy), lies in the pool
int checked_slots_in_pool(bce_ctx* c, const char* who, const uint32_t* slots, u64 count, u64 span) {
    for (u64 i = 0; i < count; ++i)
        if (slots[i] + span >= c->pool_slots) return c->fail(BCE_ERR_POOL, "%s: check %llu: slot %llu outside the pool (%u slots)", who, (unsigned long long)i, (unsigned long long)(slots[i] + span), c->pool_slots);
    return BCE_OK;
}
// a plan with a map needs the keys of the sets it names (they exist: bce_keyset_drop refuses them), any other the selected set's
int plan_need_keys(bce_ctx* c, const bce_plan* p, const char* who) {
    return p->keymap.empty() ? need_keys(c) : need_keys_of_map(c, who, p->keymap.data(), p->instances);
}
int plan_checks_ready(bce_ctx* c, const bce_plan* p, const char* who) {
    if (p->chk_total && !p->expected_set) return c->fail(BCE_ERR_STATE, "%s: the plan has checks but bce_plan_set_expected has not been called", who);
    return BCE_OK;
}
}  // namespace

extern "C" {

void bce_plan_destroy(bce_ctx* c, bce_plan* p) { destroy_schedule(c, p); }

int bce_plan_create(bce_ctx* c, uint32_t n_steps, const uint32_t* step_sizes, const bce_gate_desc* descs, uint32_t instances,
                    uint32_t slot_stride, uint32_t slot_base, bce_plan** out) {
    return bce_plan_create_keyed(c, n_steps, step_sizes, descs, instances, slot_stride, slot_base, nullptr, out);
}

int bce_plan_create_keyed(bce_ctx* c, uint32_t n_steps, const uint32_t* step_sizes, const bce_gate_desc* descs, uint32_t instances,
                          uint32_t slot_stride, uint32_t slot_base, const uint32_t* keyset_of_instance, bce_plan** out) {
    if (!c || !out) return BCE_ERR_ARG;
    *out = nullptr;
    const u32* const map = keyset_of_instance;
    const char* const who = map ? "bce_plan_create_keyed" : "bce_plan_create";   // the entry point that was called, for the messages
    if (!step_sizes || !descs || n_steps == 0 || instances == 0) return c->fail(BCE_ERR_ARG, "%s: empty schedule", who);
    if (const int rc = map ? need_keys_of_map(c, who, map, instances) : need_keys(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<bce_plan, ScheduleDeleter> p(new bce_plan, ScheduleDeleter{c});
    { std::lock_guard<std::mutex> lk(g_live_mu); c->plans.insert(p.get()); }
    p->instances = instances; p->slot_stride = slot_stride; p->slot_base = slot_base;
    u64 total = 0;
    for (u32 s = 0; s < n_steps; ++s) {
        if (step_sizes[s] == 0) return c->fail(BCE_ERR_ARG, "%s: step %u is empty", who, s);
        p->off.push_back((u32)total); p->cnt.push_back(step_sizes[s]);
        p->max_step = std::max(p->max_step, step_sizes[s]);
        total += step_sizes[s];
        if (total >= (1ull << 31)) return c->fail(BCE_ERR_ARG, "%s: too many descriptors", who);
    }
    std::vector<bce_gate_desc> d(descs, descs + total);
    const u64 span = (u64)slot_base + (u64)(instances - 1) * slot_stride;
    p->pairs.assign(n_steps, 0);
    u32 step = 0;
    for (u64 i = 0; i < total; ++i) {
        bce_gate_desc& g = d[i];
        const DescKind k = desc_kind(g.op);
        if (!k.boot()) return c->fail(BCE_ERR_ARG, "%s: descriptor %llu is not a bootstrapped gate (op %u)", who, (unsigned long long)i, g.op);
        if (k.pair()) {
            while (step + 1 < n_steps && i >= (u64)p->off[step + 1]) ++step;
            p->pairs[step] = 1;
        }
        const u64 hi = top_slot(g, k);
        if (hi + span >= c->pool_slots) return c->fail(BCE_ERR_POOL, "%s: descriptor %llu: slot %llu outside the pool (%u slots)", who, (unsigned long long)i, (unsigned long long)(hi + span), c->pool_slots);
        g.in0 += slot_base; g.in1 += slot_base; g.out += slot_base;
    }
    p->boots_per_run = total * instances;
    if (map) {   // the map rides behind the descriptors, in whole descriptor-sized words of the same resident block
        d.resize(total + ((size_t)instances * sizeof(u32) + sizeof(bce_gate_desc) - 1) / sizeof(bce_gate_desc), bce_gate_desc{});
        std::memcpy(static_cast<void*>(d.data() + total), map, (size_t)instances * sizeof(u32));
    }
    HIP_TRY(c, upload_vector(p->d_descs, d));
    if (map) {   // named only now: bce_keyset_drop looks at the plans that exist
        p->d_map = reinterpret_cast<const u32*>(p->d_descs.get() + total);
        std::lock_guard<std::mutex> lk(g_live_mu);
        p->keymap.assign(map, map + instances);
    }
    *out = p.release();
    return BCE_OK;
}

int bce_plan_run_step(bce_ctx* c, bce_plan* p, uint32_t step) {
    if (!c || !p) return BCE_ERR_ARG;
    if (step >= p->cnt.size()) return c->fail(BCE_ERR_ARG, "bce_plan_run_step: step %u of %zu", step, p->cnt.size());
    if (const int rc = plan_need_keys(c, p, "bce_plan_run_step")) return rc;
    if (const int rc = plan_checks_ready(c, p, "bce_plan_run_step")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = ensure_acc(c, (size_t)p->cnt[step] * p->instances);
    if (rc) return rc;
    const int rc2 = launch_bootstraps(c, p->d_descs.get() + p->off[step], p->cnt[step], p->instances, p->slot_stride, c->d_acc.get(), nullptr, nullptr, true, nullptr, p->pairs[step] != 0, nullptr, p->d_map);
    if (rc2) return rc2;
    if (const int rc3 = plan_check_step(c, p, step)) return rc3;
    return drain_if_long(c);
}

int bce_plan_run(bce_ctx* c, bce_plan* p) {
    if (!c || !p) return BCE_ERR_ARG;
    if (const int rc = plan_need_keys(c, p, "bce_plan_run")) return rc;
    if (const int rc = plan_checks_ready(c, p, "bce_plan_run")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (p->exec && !(c->capture_snapshot(p->d_map != nullptr) == p->captured)) {
        // the pool grew (bce_pool_reserve) or, for a plan without a map, another key set was selected since the capture: the
        // graph's kernel arguments are stale.  (The keys themselves are read through the context's table at every replay.)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p->drop_capture();
    }
    if (!p->exec) {
        // scratch of the captured launches, sized for the largest step
        const size_t nb = (size_t)p->max_step * p->instances;
        if (!p->d_acc.get()) HIP_TRY(c, p->d_acc.alloc(nb * 2 * c->N * c->wbytes));
        if (!p->d_partial.get()) HIP_TRY(c, p->d_partial.alloc(std::max<size_t>(1, tail_partial_words(c->P, (u32)nb))));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // relaxed mode: the launchers set kernel attributes (dynamic LDS size) while the stream is capturing
        HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
        int rc = BCE_OK;
        u64 fused = 0;
        for (size_t s = 0; s < p->cnt.size() && rc == BCE_OK; ++s) {
            bool f = false;
            rc = launch_bootstraps(c, p->d_descs.get() + p->off[s], p->cnt[s], p->instances, p->slot_stride, p->d_acc.get(), nullptr, nullptr, false, &f, p->pairs[s] != 0, p->d_partial.get(), p->d_map);
            fused += f ? 1 : 0;
            if (rc == BCE_OK) rc = plan_check_step(c, p, s);
        }
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &g);   // always end the capture, also after a failed launch
        if (rc != BCE_OK) { if (g) hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || !g) return c->fail(BCE_ERR_HIP, "bce_plan_run: stream capture failed: %s", hipGetErrorString(e));
        p->graph = g;
        p->fused_launches = fused;
        p->captured = c->capture_snapshot(p->d_map != nullptr);
        const hipError_t e2 = hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0);
        if (e2 != hipSuccess) { p->exec = nullptr; return c->fail(BCE_ERR_HIP, "bce_plan_run: hipGraphInstantiate: %s", hipGetErrorString(e2)); }
    }
    EventPair e0 = get_events(c, BCE_BR_GRAPH);
    hipEventRecord(e0.a, c->stream);
    HIP_TRY(c, hipGraphLaunch(p->exec, c->stream));
    hipEventRecord(e0.b, c->stream);
    c->pending.push_back(e0);
    c->timing.br_launches[BCE_BR_GRAPH] += p->cnt.size();
    c->timing.br_bootstraps[BCE_BR_GRAPH] += p->boots_per_run;
    c->timing.blind_rotate_launches += p->cnt.size();
    c->timing.bootstraps += p->boots_per_run;
    c->timing.fused_tail_launches += p->fused_launches;
    return drain_if_long(c);
}

// ---- verify mode on the device (include/bce_gpu.h, "verify mode on the device") -----------------------------------
int bce_check_slots(bce_ctx* c, uint32_t count, const uint32_t* slots, const uint8_t* expect, uint32_t instances,
                    uint32_t slot_stride, int repair, uint32_t tag) {
    if (!c) return BCE_ERR_ARG;
    if (!slots || !expect) return c->fail(BCE_ERR_ARG, "bce_check_slots: null pointer");
    if (const int rc = need_keys(c)) return rc;
    if (count == 0 || instances == 0) return BCE_OK;
    const u64 items = (u64)count * instances;
    if (items > (1ull << 31)) return c->fail(BCE_ERR_ARG, "bce_check_slots: too many checks");
    if (const int rc = checked_slots_in_pool(c, "bce_check_slots", slots, count, (u64)(instances - 1) * slot_stride)) return rc;
    if (const int rc = expected_are_messages(c, "bce_check_slots", expect, items)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = ensure_check(c)) return rc;
    const size_t slot_bytes = (size_t)count * sizeof(u32), bytes = slot_bytes + items;
    StagedUpload& st = c->chk_stage;   // slot list, then expected bits: 64 KiB at least, grown after the work in flight
    HIP_TRY(c, st.reserve(bytes, std::max(bytes, (size_t)1 << 16), c->stream));
    std::memcpy(st.host(), slots, slot_bytes);
    std::memcpy(static_cast<char*>(st.host()) + slot_bytes, expect, items);
    HIP_TRY(c, st.send(bytes, c->stream));
    const char* dev = static_cast<const char*>(st.device());
    HIP_TRY(c, launch_lwe_check(c->P, reinterpret_cast<const u32*>(dev), reinterpret_cast<const uint8_t*>(dev + slot_bytes),
                                count, count, instances, slot_stride, repair, tag, c->d_check(), c->d_check_log(), c->stream));
    return BCE_OK;
}

int bce_plan_set_checks(bce_ctx* c, bce_plan* p, const uint32_t* check_sizes, const uint32_t* slots, int repair) {
    if (!c || !p) return BCE_ERR_ARG;
    if (!p->keymap.empty()) return c->fail(BCE_ERR_UNSUPPORTED, "bce_plan_set_checks on a plan created with a key-set map (bce_plan_create_keyed): device-side checks run under one key set");
    if (const int rc = need_keys(c)) return rc;
    const size_t n_steps = p->cnt.size();
    u64 total = 0;
    for (size_t s = 0; check_sizes && s < n_steps; ++s) total += check_sizes[s];
    if (total && !slots) return c->fail(BCE_ERR_ARG, "bce_plan_set_checks: null slot list");
    if (total * p->instances > (1ull << 31)) return c->fail(BCE_ERR_ARG, "bce_plan_set_checks: too many checks");
    const u64 span = (u64)p->slot_base + (u64)(p->instances - 1) * p->slot_stride;   // the span rule of bce_plan_create
    if (const int rc = checked_slots_in_pool(c, "bce_plan_set_checks", slots, total, span)) return rc;
    std::vector<u32> shifted(total);
    for (u64 i = 0; i < total; ++i) shifted[i] = slots[i] + p->slot_base;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    p->drop_capture();   // its launches would miss (or still hold) the old lists: captured again at the next bce_plan_run
    plan_free_checks(p);
    if (total == 0) return BCE_OK;
    if (const int rc = ensure_check(c)) return rc;
    for (size_t s = 0, at = 0; s < n_steps; ++s) { p->chk_off.push_back((u32)at); p->chk_cnt.push_back(check_sizes[s]); at += check_sizes[s]; }
    const size_t ebytes = (size_t)total * p->instances;
    HIP_TRY(c, upload_vector(p->d_chk_slots, shifted));
    HIP_TRY(c, p->expect.reserve(ebytes, ebytes, nullptr));   // once, here: the next capture points into it
    p->chk_total = (u32)total;
    p->chk_repair = repair;
    return BCE_OK;
}

int bce_plan_set_expected(bce_ctx* c, bce_plan* p, const uint8_t* expect) {
    if (!c || !p) return BCE_ERR_ARG;
    if (!expect) return c->fail(BCE_ERR_ARG, "bce_plan_set_expected: null pointer");
    if (!p->chk_total) return c->fail(BCE_ERR_STATE, "bce_plan_set_expected: the plan has no checks (bce_plan_set_checks)");
    const size_t bytes = (size_t)p->chk_total * p->instances;
    if (const int rc = expected_are_messages(c, "bce_plan_set_expected", expect, bytes)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, p->expect.reserve(bytes, bytes, nullptr));   // its size since bce_plan_set_checks: only waits for the last upload
    std::memcpy(p->expect.host(), expect, bytes);
    HIP_TRY(c, p->expect.send(bytes, c->stream));
    p->expected_set = true;
    return BCE_OK;
}

int bce_check_reset(bce_ctx* c) {
    if (!c) return BCE_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = ensure_check(c)) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_check(), 0, sizeof(bce_check_report), c->stream));
    return BCE_OK;
}

int bce_check_get(bce_ctx* c, bce_check_report* out, bce_check_entry* log, uint32_t log_cap) {
    if (!c) return BCE_ERR_ARG;
    if (!out || (log_cap && !log)) return c->fail(BCE_ERR_ARG, "bce_check_get: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = ensure_check(c)) return rc;
    if (const int rc = sync_stream(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->d_check(), sizeof *out, hipMemcpyDeviceToHost));
    out->log_count = std::min<u32>(out->log_count, kCheckLogCap);   // the device counter goes on counting past the log's end
    const u32 n = std::min(out->log_count, log_cap);
    if (n) HIP_TRY(c, hipMemcpy(log, c->d_check_log(), (size_t)n * sizeof *log, hipMemcpyDeviceToHost));
    return BCE_OK;
}

}  // extern "C"
