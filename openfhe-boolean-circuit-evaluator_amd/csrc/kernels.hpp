// kernels.hpp -- launch interface of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_ext.h>

#include <tuple>

#include <cstdint>

#include "../../include/bce_gpu.h"

namespace bce {

using u32 = uint32_t;
using u64 = uint64_t;

// The keys of one key set as the kernels read them: one entry of the context's device table (all null for a free id).
struct KeySetDev {
    const void* bsk;    // EVALUATION domain, GINX [n][2][R][2][N]; AP [n][baseR][dR][R][2][N]; u32 words, u64 words (is64) or doubles (fp64)
    const void* ksk;    // [N][baseKS][dKS][ksk_stride]
    const int8_t* s8;   // the LWE secret as the device-side checks read it: int8[n], zero-padded to a multiple of 64
};

// What key_set() reads, for kernels that take no DevParams (k_lwe_check): the table and the selected set.  Checks never
// run with a key-set map (bce_plan_set_checks refuses a keyed plan), so the map is null by type.
struct KeySetRef {
    const KeySetDev* keysets;
    u32 keyset_sel;
    static constexpr const u32* keyset_map = nullptr;
};

// Everything a kernel needs, passed by value (lives in SGPRs / kernarg).
struct DevParams {
    u32 n, N, logN;
    u32 q;            // LWE modulus, power of two
    u32 Q;            // ring modulus, prime < 2^28, Q = 1 mod 2N
    u32 qKS;          // key-switch modulus
    u32 baseKS, dKS;
    u32 ksk_stride;   // elements per KSK row (>= n+1, padded)
    u32 ksk_u16;      // 1: rows are uint16_t, 0: uint32_t
    u32 ks_chunk;     // rows whose elements can be summed in 32 bits: floor(2^32 / qKS), a multiple of 8, >= 8
    u32 gBits, dG;    // gadget: base 2^gBits, dG digits; R = 2*dG RGSW rows
    u32 baseR, dR;    // AP only
    u32 method_ap;    // 1: AP/DM accumulator, 0: GINX/CGGI
    u32 factor;       // 2N / q
    u32 Q8p1;         // Q/8 + 1
    u32 red_shift;    // Barrett for x < 2^(2*bitlen(Q)+3): x1 = x >> red_shift
    u32 red_mu;       // floor(2^(32+red_shift) / Q)
    u32 Ninv, Ninv_s; // N^-1 mod Q and its Shoup companion
    u32 Winv_last, Winv_last_s;  // -psi^(N/2) * N^-1: twiddle of the last inverse stage with the scaling folded in
    u32 mu32;         // floor(2^32 / Q): one-step reduction of any 32-bit value to [0, 2Q)
    u32 lazy;         // 1 when the forward NTT can run without any correction (bounds in engine.cpp)
    u32 c32;          // 2^32 mod Q (folds 64-bit MAC sums of un-normalised NTT outputs)
    u32 occupancy_target;  // workgroups per CU the blind-rotation kernel is compiled for (2 or 3)
    u32 variant;           // blind-rotation kernel choice: 0 automatic; 1 one-wave-per-transform kernel; 2 / 3 split-
                           // transform kernel forced to its 256- / 128-register build (development knob BCE_VARIANT)
    u32 cu_count;          // compute units of the device (automatic choice: a launch of <= cu_count workgroups)
    u32* xcd_gate;         // [16 XCC ids][32 words] arrival counters of the launch's workgroups per XCD, or null: multi-round launches of
                           // the split-transform kernel start their workgroups in per-XCD cohorts (round 4; BCE_XCD_GATE=0 disables)
    u32 xcd_gate_ticks;    // longest wait at that gate (100 MHz ticks)
    u32 fuse_tail;         // 1: saturated launches of the split-transform kernel run the tail in their epilogue (BCE_FUSE_TAIL=0 disables)
    u32 fold_ninv;         // 1 (folded fp64 kernels, kernels64.hip): rows l >= 1 of the key are also multiplied by N^-1 and the
                           // evaluation-form accumulator is kept scaled by N^-1, so that the un-normalised inverse transform yields
                           // the coefficients themselves (no N^-1 product per coefficient and step)
    u32 fold;              // 1: the key is stored with the lowest gadget digit folded in (rows l >= 1 hold ek_l - B^l ek_0) and
                           // the kernels multiply the digit-0 rows by the evaluation-form accumulator itself (BCE_FOLD=0 disables)
    u32 fwd_units;         // 1: the two-workgroups-per-CU build of the folded GINX split-transform kernel runs its six forward transforms
                           // as 24 quarter units, three per wave (kernels.hip, ntt_forward_quarter3<false>; BCE_FWD_UNITS=0 keeps
                           // the whole-row + half-row bodies)
    u32 factor_even;       // 1: factor = 2N / q is even, so every rotation exponent a' is even and I^a' = +-1: the quarter-unit build
                           // is compiled with the GINX MAC tail for that case (no parity selects, no products by I^+-a')
    u32 I4[4], I4s[4];     // powers of I = psi^(N/2) (primitive 4th root of unity) and Shoup companions
    const uint2* tw_f;  // [N] (psi^brv(i), shoup), index m+i as in the CT forward NTT; the inverse
                        // transform derives psi^-k = -psi^(N-k) from the same table
    const u32* psi_tab; // [N] psi^e in natural exponent order (monomial lookups of the GINX MAC)
    // Montgomery form of the GINX MAC tail in the split-transform kernels (R = 2^32, kernels.hip ginx_mac_tail_redc):
    const u32* psi_tab_r2;  // [N] psi^e * R^2 mod Q
    u32 qinv_neg;           // -Q^-1 mod 2^32
    u32 r2_off;             // Q - (R^2 mod Q): psi^e R^2 + r2_off = (psi^e - 1) R^2 mod Q, lazily in [0, 2Q)
    // ---- 64-bit ring modulus path (kernels64.hip), used when is64 != 0 (Q >= 2^28) ----
    u32 is64;
    u64 Q64, Q8p1_64;
    u64 mu64;           // floor(2^64 / Q)
    u64 c64;            // 2^64 mod Q
    u64 Ninv64, Ninv64_s;
    const ulonglong2* tw64;  // [N] (psi^brv(i), floor(. * 2^64 / Q))
    // double-precision formulation of the 64-bit path (kernels64.hip, namespace wd), used when fp64 != 0 (Q < 2^39):
    // the bootstrapping-key words of a key set are then IEEE doubles
    u32 fp64;
    double Qd, invQd;          // Q, 1/Q
    double Ninvd, Ninvd_q;     // N^-1 mod Q and N^-1 / Q
    const double2* tw64d;      // [N] (psi^brv(i), psi^brv(i) / Q)
    u32* pool;          // [slots][pool_stride]
    u32 pool_stride;
    // ---- matrix-pipe forward stages of the quarter units (at the end: the other kernels' argument layout is unchanged) ----
    u32 fwd_mfma;          // 1 (needs fwd_units): the stages on bits 9..4 of those transforms run on the matrix pipe as i8 products of
                           // the signed gadget digits with the limbs of one constant 64 x 64 matrix (kernels.hip,
                           // ntt_forward_quarter3<true>; tables and conditions: fwd_mfma.hpp; BCE_FWD_MFMA=0 keeps the quarter-unit body)
    u32 w14, w14s;         // 2^14 mod Q and its Shoup companion (recombination of the limb products)
    const u32* fwd_mfma_tab;   // [4 quarters][4 tiles][64 lanes][4 words]: A operands, or null
    // ---- key sets: where a workgroup finds its keys (gate_front.hpp, key_set) ----
    const KeySetDev* keysets;  // [BCE_MAX_KEYSETS], one fixed table per context (captured graphs point at it)
    u32 keyset_sel;            // the selected set: what a launch without a map runs under
    const u32* keyset_map;     // [instances] set of every instance, or null; set per launch in the launch's copy of this block
};

// ---- the kernel-class rule: which blind-rotation family a context runs, and everything that follows from it -----------
// The one place that knows it.  The 32-bit part (shape rule of the split-transform family, read off kLatBuilds) lives in
// kernels.hip, the 64-bit part (shape rule of the integer / fp64 families, read off kWdBuilds) in kernels64.hip.
constexpr size_t kLdsBytesPerCu = 160 * 1024;
// An AP key of the split-transform family must be smaller than this (one buffer resource, 32-bit row offsets: kernel_class)
constexpr unsigned long long kSplitApKeyBytes = 1ull << 31;
enum class KernelFamily {
    WavePerTransform,   // k_blind_rotate (kernels.hip): one wave per transform, every 32-bit shape the split family does not take
    SplitTransform,     // k_blind_rotate_lat / k_bootstrap_dag (kernels.hip): N = 1024, four gadget digits, lazy bounds hold,
                        // an AP key below kSplitApKeyBytes
    Int64,              // w64::k_blind_rotate64 (kernels64.hip), with its narrow build (four digits, N >= 1024, Q < 2^31)
    Fp64,               // wd::k_blind_rotate64d / k_bootstrap_dag64 (kernels64.hip): Q < 2^39 in doubles
};
struct KernelClass {
    KernelFamily family;
    const char* error;        // null, or why no kernel exists for this shape (what bce_ctx_create* reports; BCE_ERR_UNSUPPORTED)
    const char* lds_error;    // null, or why the family's LDS layout does not fit a CU for this shape (same status)
    bool fold_build;          // a build that reads the folded key exists for this shape and method (does not look at P.fold)
    bool dag;                 // a persistent dependency-driven build (launch_bootstrap_dag) exists for P as it stands
    u32 fp64;                 // P.fp64 as granted: the request, and the shape has a doubles kernel
    u32 occupancy_target;     // P.occupancy_target as granted: 3 unless 2 was asked for or three workgroups' LDS exceed a CU's
    u32 wg_per_cu_lone, wg_per_cu_full;   // workgroups a CU holds in a launch of <= cu_count workgroups / in a saturated one
    size_t lds_bytes;         // dynamic LDS of one workgroup (of the saturated launch's build where the builds differ)
};
// Reads the shape (is64, Q64, logN, dG, n, method_ap, lazy, variant) and two REQUESTS the engine presets: P.fp64 (doubles
// wanted) and P.occupancy_target (2 or 3 wanted); the engine stores the granted values back.  `error` needs the shape
// fields alone; fold_build does not read P.fold; `dag` and lds_bytes describe P as it stands (fold, fwd_mfma, fuse_tail).
KernelClass kernel_class(const DevParams& P);

// ---- dependency-driven evaluation of a whole bootstrap DAG by ONE persistent launch (k_bootstrap_dag) ----------------
// Replaces the manager <-> executor loop of the reference (src/circuit.cpp:575-683 ready-gate rule, :698-710 parallel
// region) on the device: every (task, instance) pair has a counter of unfinished producers; a workgroup that finishes a
// bootstrap decrements its consumers' counters and pushes those that reach zero to a ready queue; idle workgroups pull
// from the queues.  No kernel boundary and no device-wide barrier between dependent bootstraps.
constexpr u32 kDagQueues = 4;        // priority classes (0 = most urgent)
constexpr u32 kDagCtlStride = 32;    // control block: words [0, 4) = heads, [4, 8) = tails of the four classes (one 32-byte block)
constexpr u32 kDagCuKeys = 4096;     // (XCC id, SE, SH, CU) keys of the placement table
// control block (u32 words): heads and tails in the first line; then the words below; then the per-CU tables
constexpr u32 kDagAbort = kDagQueues * kDagCtlStride;      // != 0: a poller gave up (code)
constexpr u32 kDagDone = kDagAbort + 1;                    // bootstraps completed
constexpr u32 kDagLazyWaits = kDagAbort + 2;               // diagnostics: claims a half-busy CU delayed for an idle one
constexpr u32 kDagBusyTicks = kDagAbort + 4;               // u64: 100 MHz ticks workgroups spent between claiming an item and releasing its consumers
constexpr u32 kDagWaitTicks = kDagAbort + 6;               // u64: ticks workgroups spent looking for an item they then got
constexpr u32 kDagIdleCus = 8;                             // compute units none of whose workgroups runs a bootstrap (same line as heads / tails)
constexpr u32 kDagCuArrive = kDagAbort + 32;               // [kDagCuKeys] workgroups that announced themselves per CU
constexpr u32 kDagCuBusy = kDagCuArrive + kDagCuKeys;      // [kDagCuKeys] workgroups running a bootstrap per CU
constexpr u32 kDagGate = kDagCuBusy + kDagCuKeys;          // [16 XCC ids] x 32 words: word pair 0 = the XCD's start gate (u64)
constexpr u32 kDagCohortRing = 64;                         // generations of an XCD's gate whose (size, arrived) pairs are kept
constexpr u32 kDagCohort = kDagGate + 16 * 32;             // [16 XCC ids][kDagCohortRing] x {size, arrived}
constexpr u32 kDagGateWaits = kDagAbort + 8;               // u64: ticks workgroups waited at their XCD's start gate
constexpr u32 kDagCtlWords = kDagCohort + 16 * kDagCohortRing * 2;
// DagRearm: what re-arming reads (k_dag_rearm takes it by value); DagParams adds what only the persistent kernel reads.
struct DagRearm {
    const bce_gate_desc* tasks;   // [n_tasks] topological order, SSA slots
    const u32* cons_off;          // [n_tasks + 1]
    const u32* cons;              // consumers of every task
    const uint8_t* qid;           // [n_tasks] priority class
    const u32* dep_init;          // [n_tasks] producers inside the DAG (0..2)
    u32* dep;                     // [instances][n_tasks] unfinished producers
    u32* slots[kDagQueues];       // queue entries: item + 1 (0 = not yet pushed); item = instance * n_tasks + task
    u32 qcap[kDagQueues];         // entries the queue will ever receive (tasks of that class x instances)
    const u32* init_items;        // initially ready tasks of every class, concatenated; init_off[q] .. init_off[q + 1]
    u32 init_off[kDagQueues + 1];
    u32* ctl;                     // control block, kDagCtlWords words
    u32 n_tasks, instances, slot_stride, slot_base;   // instance k: slot numbers + slot_base + k * slot_stride
    u32 lazy_ticks;               // 100 MHz ticks a workgroup on a half-busy CU leaves a lone ready item to an idle CU
    u32 stall_ticks;              // 100 MHz ticks without any push after which a poller sets the abort word
    u32 policy;                   // bit 0: placement-aware claims (idle CUs first); bit 1: dry run (development);
                                  // bit 2: workgroups of one XCD that claimed from a deep queue start their bootstraps together;
                                  // bit 3: tickets for every claim (round 3's rule, kept for the A/B against the hybrid claim)
    u32 gate_ticks;               // longest wait at the XCD start gate (100 MHz ticks)
    u32 gate_backlog;             // queue depth at claim time from which a bootstrap goes through the gate
};
struct DagParams : DagRearm {
    // verify mode (bce_dag_set_checks): the worker checks a task's refreshed ciphertext between its bootstrap and the
    // release of its consumers (dag_sched.hpp: dag_check).  chk_of_task == nullptr: the run has no checks.
    const u32* chk_of_task;       // [n_tasks] check number + 1, 0 = the task is not checked
    const uint8_t* expect;        // [instances][n_checks] expected messages (0..3)
    u32 n_checks;
    u32 repair;                   // != 0: a mismatching row is overwritten with the trivial ciphertext of the expected message
    bce_check_report* report;     // the context's report block and mismatch log (bce_check_reset / bce_check_get)
    bce_check_entry* log;
};
// rearm = reset counters / queues for one evaluation; then the persistent launch.  wps = 2: one workgroup per CU
// (256-register build), 4: two per CU.  grid = resident workgroups (never more).
hipError_t launch_dag_rearm(const DagRearm& D, hipStream_t s);
// d_P / d_params: the engine's DevParams and the run's DagParams in DEVICE memory (the kernel reads their fields where
// it needs them instead of holding kernel arguments in registers across its loop)
hipError_t launch_bootstrap_dag(const DevParams& P, const DevParams* d_P, const DagParams* d_params, int wps, u32 grid,
                                hipStream_t s);
inline bool dag_kernel_available(const DevParams& P) { return kernel_class(P).dag; }
// dynamic LDS of one workgroup of the 32-bit persistent kernel (split-transform family; the mailbox included): what
// bce_dag_run sizes its grid by, so that it never launches more workgroups than are resident
size_t bootstrap_dag_lds_bytes(const DevParams& P, int wps);

// Timestamps of a launch without event packets of their own in the queue: start / stop are attached to the kernel's
// dispatch (hipExtLaunchKernel) -- what hipEventRecord before and after a kernel costs on the device timeline (5-10 us of
// idle time each side) is what a dependent step of one bootstrap latency cannot afford.  Null members: nothing attached.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
// kern(args...) through hipExtLaunchKernel with the two events attached to the DISPATCH (its start / stop timestamps; either
// may be null: the launch is then simply untimed on that side); args are converted to the kernel's own parameter types first
template <typename... KA, typename... A>
inline hipError_t launch_with_events(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, LaunchEvents ev, A... args) {
    static_assert(sizeof...(KA) == sizeof...(A), "argument count");
    std::tuple<KA...> held{static_cast<KA>(args)...};
    void* ptrs[sizeof...(KA)];
    std::apply([&](auto&... a) { size_t i = 0; ((ptrs[i++] = (void*)&a), ...); }, held);
    return hipExtLaunchKernel(reinterpret_cast<const void*>(kern), grid, block, ptrs, lds, s, ev.start, ev.stop, 0);
}
// kern(args...) as a plain launch, or through launch_with_events when a timestamp is attached
template <typename... KA, typename... A>
inline hipError_t launch_kernel(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, LaunchEvents ev, A... args) {
    if (ev.start || ev.stop) return launch_with_events(kern, grid, block, lds, s, ev, args...);
    hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<KA>(args)...);
    return hipGetLastError();
}
// The launch idiom of the kernels whose dynamic LDS may exceed the default limit: opt in to `lds` bytes, then launch_kernel
template <typename... KA, typename... A>
inline hipError_t launch_kernel_lds(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, LaunchEvents ev, A... args) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return e != hipSuccess ? e : launch_kernel(kern, grid, block, lds, s, ev, args...);
}

// acc_out: [n_boot][2][N] words of the context's width (u32, or u64 when P.is64), COEFFICIENT domain, values in [0, Q)
// *kernel_id (optional) receives the enum bce_br_kernel value of the kernel that was launched, for every family
// *tail_fused (optional) is set when the launched kernel also ran the tail of EvalBinGate (extract, ModSwitch,
// KeySwitch, ModSwitch -> pool[out]) in its epilogue; the caller then skips launch_tail().  dbg_lweN / dbg_ks as
// for launch_tail (used only when the tail is fused).
hipError_t launch_blind_rotate(const DevParams& P, const bce_gate_desc* d_descs, u32 n_desc, u32 instances,
                               u32 slot_stride, void* acc_out, hipStream_t s, int* kernel_id = nullptr,
                               u32* dbg_lweN = nullptr, u32* dbg_ks = nullptr, bool* tail_fused = nullptr, LaunchEvents ev = {});

// extract + ModSwitch(Q->qKS) + KeySwitch + ModSwitch(qKS->q) -> pool[out]
// dbg_lweN: u32 [n_boot][N+1] or null; dbg_ks: u32 [n_boot][n+1] or null
// partial: device scratch of tail_partial_words(P, n_desc * instances) u64 words (partial key-switch sums)
// pairs: the descriptors hold at least one BCE_PAIR: both kernels run a second time for the second outputs (slot out + 1;
// the debug buffers then have 2 n_boot rows, the second outputs in the second half).  A blind-rotation kernel that fuses
// the tail runs the second pass itself.
size_t tail_partial_words(const DevParams& P, u32 boots);
u32 tail_split(const DevParams& P, u32 boots);   // workgroups launch_tail spreads one bootstrap's rows over (16 .. 1)
hipError_t launch_tail(const DevParams& P, const bce_gate_desc* d_descs, u32 n_desc, u32 instances, u32 slot_stride,
                       const void* acc_in /* u32 or u64 words by P.is64 */, u64* partial, u32* dbg_lweN, u32* dbg_ks,
                       hipStream_t s, LaunchEvents ev = {}, bool pairs = false);   // ev.start on the first kernel, ev.stop on the last

// key words u64 <-> IEEE double in place (layout of the double-precision formulation, kernels64.hip)
hipError_t launch_words_u64_f64(u64* words, size_t count, int to_double, hipStream_t s);

// EvalNOT / COPY over pool slots
hipError_t launch_lwe_unary(const DevParams& P, const bce_gate_desc* d_descs, u32 n_desc, u32 instances,
                            u32 slot_stride, hipStream_t s);

// dense buffer [count][n+1] u32 <-> pool rows named by d_descs[i].in0
hipError_t launch_pool_pack(const DevParams& P, const bce_gate_desc* d_descs, u32 count, u32* buf, int to_pool,
                            hipStream_t s);

// Verify mode on the device (k_lwe_check; reference: the decrypt-compare-repair of every gate output, src/gate.cpp:153-160).
// Item i = (check i % count, instance i / count) reads pool row d_slots[i % count] + (i / count) * slot_stride and the
// expected bit d_expect[(i / count) * expect_stride + i % count]; phase = b - <a, s> mod q with s = int8[n] in {-1, 0, 1} of the instance's key set,
// got = Round(4 phase / q), err = centred(phase - expect q/4).  Counters go to *d_report with agent-scope atomics, every
// mismatch (got != expect) to d_log[kCheckLogCap] while it has room.  repair != 0: a mismatching row is overwritten with the
// TRIVIAL ciphertext (0, ..., 0, expect q/4) -- not the reference's Encrypt(sk, bit): no device PRNG, no host round trip,
// repaired runs are bit-reproducible, and verify mode holds key and plaintext anyway.  The rows of one launch are distinct.
// No allocation, no synchronisation, counters are never reset here: the launch can be captured into a hipGraph.
constexpr u32 kCheckLogCap = 4096;
constexpr u32 kCheckWaves = 4;       // items a workgroup works on at a time (one wave each)
hipError_t launch_lwe_check(const DevParams& P, const u32* d_slots, const uint8_t* d_expect, u32 count,
                            u32 expect_stride, u32 instances, u32 slot_stride, int repair, u32 tag, bce_check_report* d_report,
                            bce_check_entry* d_log, hipStream_t s);

// in-place negacyclic NTT of `count` polys, [count][N] words of the context's width in global memory
hipError_t launch_ntt_batch(const DevParams& P, void* polys, u32 count, int inverse, hipStream_t s);

// In place on `rgsw` RGSW ciphertexts [R = 2 dG rows][2][N] (evaluation form, integer words: u32, or u64 when P.is64):
// dir = +1: row(2l + c) -= B^l row(c) for l = 1..dG-1 (the layout the FOLD kernels read); dir = -1 undoes it.
hipError_t launch_fold_gadget(const DevParams& P, void* bsk, u64 rgsw, int dir, hipStream_t s);

// b[p*b_step][k] += a[p][k] * z[k] mod Q for count polys (key generation); words of the context's width
hipError_t launch_pointwise_mac(const DevParams& P, void* b, const void* a, const void* z, u32 count, u32 b_step,
                                hipStream_t s);

// host-side decrypt helper kernels are not needed: decryption happens on the host (needs sk)

// ---- internal to the kernel files: what kernels.hip dispatches to for P.is64 (kernels64.hip) ------------------------
constexpr const char* kDigitCountError = "gadget digit count must be 3 or 4 (N = 2048: 3, or 4 with a ring modulus of 28..30 bits)";
KernelClass kernel_class64(const DevParams& P);   // everything but occupancy_target
hipError_t launch_bootstrap_dag64(const DevParams& P, const DevParams* d_P, const DagParams* d_params, u32 grid, hipStream_t s);
// *tail_fused (optional) is set when the launched kernel also ran the tail (then dbg_lweN / dbg_ks are its debug outputs)
hipError_t launch_blind_rotate64(const DevParams& P, const bce_gate_desc* d_descs, u32 n_desc, u32 instances, u32 slot_stride,
                                 u64* acc_out, hipStream_t s, u32* dbg_lweN, u32* dbg_ks, bool* tail_fused, LaunchEvents ev);
hipError_t launch_ntt_batch64(const DevParams& P, u64* polys, u32 count, int inverse, hipStream_t s);
hipError_t launch_pointwise_mac64(const DevParams& P, u64* b, const u64* a, const u64* z, u32 count, u32 b_step, hipStream_t s);

}  // namespace bce
