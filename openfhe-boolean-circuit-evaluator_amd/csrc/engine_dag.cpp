// engine_dag.cpp -- dependency-driven evaluation (bce_dag; include/bce_gpu.h, "the hot path, dependency-driven"): the task
// list analysed on the host (dag_build.cpp), resident on the device, and run by one persistent launch (dag_sched.hpp).
#include <algorithm>
#include <cstring>
#include <memory>

#include "ctx_params.hpp"
#include "dag_build.hpp"
#include "engine_internal.hpp"

using namespace bce;

struct bce_dag {
    DagBuild h;                                    // the analysis; h.dep = the dependency counts a run starts from
    // immutable device arrays
    DevBuf<bce_gate_desc> d_tasks;
    DevBuf<u32> d_cons_off, d_cons, d_dep_init, d_init;
    DevBuf<uint8_t> d_qid;
    // per-run state, grown on demand to the exact size, after the work in flight
    DevBuf<u32> d_dep;
    DevBuf<u32> d_slots[kDagQueues];
    DevBuf<u32> d_ctl;
    DevBuf<DagParams> d_params;
    // verify mode (bce_dag_set_checks / bce_dag_set_expected): check number + 1 per task, and the expected bits of the next
    // run(s) with their pinned staging buffer, grown on demand
    u32 n_checks = 0;
    int chk_repair = 0;
    DevBuf<u32> d_chk_of_task;
    StagedUpload expect;
    u32 expect_instances = 0;                      // the instance count the expected bits were set for, 0 = not set
};

void bce::delete_leftover(bce_dag* g) { delete g; }

// bce_dag_create and bce_dag_create_pairs: the context's checks, the analysis (build_dag), the object and its uploads
static int dag_create(bce_ctx* c, uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bce_dag** out, bool allow_pairs) {
    if (!c || !out) return BCE_ERR_ARG;
    *out = nullptr;
    if (!tasks || n_tasks == 0) return c->fail(BCE_ERR_ARG, "bce_dag_create: empty task list");
    if (!dag_kernel_available(c->P)) return c->fail(BCE_ERR_UNSUPPORTED, "bce_dag_create: no persistent kernel for this parameter class (N = 1024, 4 gadget digits, Q < 2^28; N = 2048, Q < 2^39, AP with the folded key)");
    if ((u64)n_tasks >= (1ull << 31)) return c->fail(BCE_ERR_ARG, "bce_dag_create: too many tasks");
    HIP_TRY(c, hipSetDevice(c->device));
    DagBuild h;
    if (const DagBuildStatus st = build_dag(n_tasks, tasks, prio, allow_pairs, kDagQueues, h); st.code != BCE_OK) return c->fail(st.code, "%s", st.message.c_str());

    std::unique_ptr<bce_dag, ScheduleDeleter> g(new bce_dag, ScheduleDeleter{c});
    { std::lock_guard<std::mutex> lk(g_live_mu); c->dags.insert(g.get()); }
    g->h = std::move(h);
    HIP_TRY(c, g->d_tasks.alloc(n_tasks));
    HIP_TRY(c, hipMemcpy(g->d_tasks.get(), tasks, (size_t)n_tasks * sizeof(bce_gate_desc), hipMemcpyHostToDevice));
    HIP_TRY(c, upload_vector(g->d_cons_off, g->h.cons_off));
    HIP_TRY(c, upload_vector(g->d_cons, g->h.cons));
    HIP_TRY(c, upload_vector(g->d_dep_init, g->h.dep));
    HIP_TRY(c, upload_vector(g->d_init, g->h.init_items));
    HIP_TRY(c, upload_vector(g->d_qid, g->h.qid));
    HIP_TRY(c, g->d_ctl.alloc(kDagCtlWords));
    HIP_TRY(c, g->d_params.alloc(1));
    *out = g.release();
    return BCE_OK;
}

extern "C" {

int bce_dag_supported(const bce_ctx* c) { return c && dag_kernel_available(c->P) ? 1 : 0; }

int bce_dag_set_limits(bce_ctx* c, int workgroups_per_cu, int placement, uint32_t lazy_us, uint32_t stall_ms) {
    if (!c || workgroups_per_cu < 0 || workgroups_per_cu > 2) return c ? c->fail(BCE_ERR_ARG, "workgroups_per_cu must be 0, 1 or 2") : BCE_ERR_ARG;
    if (stall_ms == 0 || stall_ms > 40000) return c->fail(BCE_ERR_ARG, "stall_ms must be in 1..40000");
    c->dag_wg_per_cu = workgroups_per_cu; c->dag_placement = placement ? 1 : 0; c->dag_lazy_us = lazy_us; c->dag_stall_ms = stall_ms;
    return BCE_OK;
}

int bce_dag_last_run(bce_ctx* c, uint64_t out[7]) {
    if (!c || !out) return BCE_ERR_ARG;
    for (int i = 0; i < 7; ++i) out[i] = c->dag_last[i];
    return BCE_OK;
}

int bce_dag_launch_choice(const uint64_t derived[BCE_D_COUNT], int workgroups_per_cu, int placement, uint32_t lazy_us, uint32_t stall_ms,
                          uint32_t depth, uint64_t items, uint64_t out[BCE_L_COUNT]) {
    if (!derived || !out) return BCE_ERR_ARG;
    DevParams P{};
    P.cu_count = (u32)derived[BCE_D_cu_count];
    P.is64 = (u32)derived[BCE_D_is64];
    const DagLaunchChoice L = dag_launch_choice(P, (u32)derived[BCE_D_wg_per_cu_full], (size_t)derived[BCE_D_dag_lds_bytes],
                                                DagLimits{workgroups_per_cu, placement, lazy_us, stall_ms}, read_dag_knobs(), depth, items);
    out[BCE_L_wps] = (u64)L.wps; out[BCE_L_grid] = L.grid; out[BCE_L_policy] = L.policy; out[BCE_L_gate_ticks] = L.gate_ticks;
    out[BCE_L_gate_backlog] = L.gate_backlog; out[BCE_L_lazy_ticks] = L.lazy_ticks; out[BCE_L_stall_ticks] = L.stall_ticks;
    out[BCE_L_rearm_only] = L.rearm_only ? 1 : 0;
    return BCE_OK;
}

void bce_dag_destroy(bce_ctx* c, bce_dag* g) { destroy_schedule(c, g); }

int bce_dag_set_checks(bce_ctx* c, bce_dag* g, uint32_t n_checks, const uint32_t* tasks, int repair) {
    if (!c || !g) return BCE_ERR_ARG;
    if (n_checks && !tasks) return c->fail(BCE_ERR_ARG, "bce_dag_set_checks: null task list");
    if (const int rc = need_keys(c)) return rc;
    const u32 n_tasks = g->h.n_tasks;
    std::vector<u32> of_task(n_tasks, 0);
    for (u32 i = 0; i < n_checks; ++i) {
        if (tasks[i] >= n_tasks) return c->fail(BCE_ERR_ARG, "bce_dag_set_checks: check %u names task %u of %u", i, tasks[i], n_tasks);
        if (of_task[tasks[i]]) return c->fail(BCE_ERR_ARG, "bce_dag_set_checks: task %u is listed twice (checks %u and %u)", tasks[i], of_task[tasks[i]] - 1, i);
        of_task[tasks[i]] = i + 1;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // a run in flight may still read the old list
    g->n_checks = 0; g->expect_instances = 0;      // new lists need their own expected bits
    if (n_checks == 0) return BCE_OK;              // detached: bce_dag_run passes no list to the kernel
    if (const int rc = ensure_check(c)) return rc;
    if (!g->d_chk_of_task.get()) HIP_TRY(c, g->d_chk_of_task.alloc(n_tasks));
    HIP_TRY(c, hipMemcpy(g->d_chk_of_task.get(), of_task.data(), (size_t)n_tasks * sizeof(u32), hipMemcpyHostToDevice));
    g->n_checks = n_checks;
    g->chk_repair = repair ? 1 : 0;
    return BCE_OK;
}

int bce_dag_set_expected(bce_ctx* c, bce_dag* g, uint32_t instances, const uint8_t* expect) {
    if (!c || !g) return BCE_ERR_ARG;
    if (!expect) return c->fail(BCE_ERR_ARG, "bce_dag_set_expected: null pointer");
    if (instances == 0) return c->fail(BCE_ERR_ARG, "bce_dag_set_expected: no instances");
    if (!g->n_checks) return c->fail(BCE_ERR_STATE, "bce_dag_set_expected: the DAG has no checks (bce_dag_set_checks)");
    const size_t bytes = (size_t)g->n_checks * instances;
    if (const int rc = expected_are_messages(c, "bce_dag_set_expected", expect, bytes)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (bytes > g->expect.capacity()) g->expect_instances = 0;   // the old bits go with the old buffer
    HIP_TRY(c, g->expect.reserve(bytes, bytes, c->stream));       // exact size; a run in flight may still read the old buffer
    std::memcpy(g->expect.host(), expect, bytes);
    HIP_TRY(c, g->expect.send(bytes, c->stream));
    g->expect_instances = instances;
    return BCE_OK;
}

int bce_dag_create(bce_ctx* c, uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bce_dag** out) {
    return dag_create(c, n_tasks, tasks, prio, out, false);
}
int bce_dag_create_pairs(bce_ctx* c, uint32_t n_tasks, const bce_gate_desc* tasks, const uint8_t* prio, bce_dag** out) {
    return dag_create(c, n_tasks, tasks, prio, out, true);
}

int bce_dag_debug_block_task(bce_dag* g, uint32_t t) {
    if (!g || t >= g->h.n_tasks) return BCE_ERR_ARG;
    g->h.dep[t] += 1;
    return hipMemcpy(g->d_dep_init.get(), g->h.dep.data(), (size_t)g->h.n_tasks * sizeof(u32), hipMemcpyHostToDevice) == hipSuccess ? BCE_OK : BCE_ERR_HIP;
}

int bce_dag_run(bce_ctx* c, bce_dag* g, uint32_t instances, uint32_t slot_stride, uint32_t slot_base) {
    if (!c || !g) return BCE_ERR_ARG;
    if (instances == 0) return BCE_OK;
    if (const int rc = need_keys(c)) return rc;
    const DagBuild& h = g->h;
    if (g->n_checks && g->expect_instances == 0) return c->fail(BCE_ERR_STATE, "bce_dag_run: the DAG has checks but bce_dag_set_expected has not been called");
    if (g->n_checks && g->expect_instances != instances) return c->fail(BCE_ERR_STATE, "bce_dag_run: %u instances, but the expected bits were set for %u", instances, g->expect_instances);
    if (instances > 1 && slot_stride <= h.max_slot) return c->fail(BCE_ERR_ARG, "bce_dag_run: slot_stride %u does not cover the DAG's slots (0..%u)", slot_stride, h.max_slot);
    if ((u64)slot_base + h.max_slot + (u64)(instances - 1) * slot_stride >= c->pool_slots) return c->fail(BCE_ERR_POOL, "bce_dag_run: slot %llu outside the pool (%u slots)", (unsigned long long)((u64)slot_base + h.max_slot + (u64)(instances - 1) * slot_stride), c->pool_slots);
    const u64 items = (u64)h.n_tasks * instances;
    if (items >= 0xFFFFFFF0ull) return c->fail(BCE_ERR_ARG, "bce_dag_run: %llu bootstraps exceed one run's 32-bit item space", (unsigned long long)items);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->dag_pending >= bce_ctx::kDagRuns) { const int rc = sync_stream(c); if (rc) return rc; }
    if (!c->d_P.get()) HIP_TRY(c, c->d_P.alloc(1));
    if (!c->h_dag_status.get()) HIP_TRY(c, c->h_dag_status.alloc(bce_ctx::kDagRuns));
    if (!c->h_dag_stage.get()) HIP_TRY(c, c->h_dag_stage.alloc(bce_ctx::kDagRuns));
    // per-run state (a dag object serves one run at a time: runs are ordered on the engine's stream)
    HIP_TRY(c, g->d_dep.grow(items, items, c->stream));
    DagParams D{};
    for (u32 q = 0; q < kDagQueues; ++q) {
        const size_t need = (size_t)h.qcount[q] * instances;
        HIP_TRY(c, g->d_slots[q].grow(need, need, c->stream));
        D.slots[q] = g->d_slots[q].get();
        D.qcap[q] = (u32)need;
        D.init_off[q] = h.init_off[q];
    }
    D.init_off[kDagQueues] = h.init_off[kDagQueues];
    D.tasks = g->d_tasks.get(); D.cons_off = g->d_cons_off.get(); D.cons = g->d_cons.get(); D.qid = g->d_qid.get(); D.dep_init = g->d_dep_init.get();
    D.dep = g->d_dep.get(); D.init_items = g->d_init.get(); D.ctl = g->d_ctl.get();
    D.n_tasks = h.n_tasks; D.instances = instances; D.slot_stride = slot_stride; D.slot_base = slot_base;
    if (g->n_checks) {   // verify mode: the worker checks (and repairs) before it releases a task's consumers
        if (const int rc = ensure_check(c)) return rc;
        D.chk_of_task = g->d_chk_of_task.get(); D.expect = static_cast<const uint8_t*>(g->expect.device()); D.n_checks = g->n_checks; D.repair = (u32)g->chk_repair;
        D.report = c->d_check(); D.log = c->d_check_log();
    }
    // one or two workgroups per CU, the grid, the policy bits and the gate constants (ctx_params.cpp)
    const DagLaunchChoice L = dag_launch_choice(c->P, kernel_class(c->P).wg_per_cu_full, c->P.is64 ? 0 : bootstrap_dag_lds_bytes(c->P, 4),
                                                DagLimits{c->dag_wg_per_cu, c->dag_placement, c->dag_lazy_us, c->dag_stall_ms}, read_dag_knobs(), h.depth, items);
    D.lazy_ticks = L.lazy_ticks; D.stall_ticks = L.stall_ticks; D.policy = L.policy; D.gate_ticks = L.gate_ticks; D.gate_backlog = L.gate_backlog;
    // parameter blocks reach the device in stream order (an earlier run may still be reading the previous ones) from
    // pinned staging entries that stay untouched until the next synchronisation
    const int slot = c->dag_pending++;
    bce_ctx::DagStage& stage = c->h_dag_stage.get()[slot];
    stage.P = c->P;
    stage.D = D;
    HIP_TRY(c, hipMemcpyAsync(c->d_P.get(), &stage.P, sizeof(DevParams), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(g->d_params.get(), &stage.D, sizeof(DagParams), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_dag_rearm(D, c->stream));
    EventPair e0 = get_events(c, BCE_BR_DAG);
    hipEventRecord(e0.a, c->stream);
    if (!L.rearm_only) HIP_TRY(c, launch_bootstrap_dag(c->P, c->d_P.get(), g->d_params.get(), L.wps, L.grid, c->stream));
    hipEventRecord(e0.b, c->stream);
    c->pending.push_back(e0);
    c->dag_expected[slot] = items;
    c->dag_wps_used[slot] = L.wps;
    HIP_TRY(c, hipMemcpyAsync(&c->h_dag_status.get()[slot], g->d_ctl.get() + kDagAbort, sizeof(bce_ctx::DagStatus), hipMemcpyDeviceToHost, c->stream));
    c->timing.br_launches[BCE_BR_DAG] += 1;
    c->timing.br_bootstraps[BCE_BR_DAG] += items;
    c->timing.blind_rotate_launches += 1;
    c->timing.fused_tail_launches += 1;
    c->timing.bootstraps += items;
    return BCE_OK;
}

}  // extern "C"
