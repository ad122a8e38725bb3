// ctx_params.hpp -- what a context decides about itself, as pure host functions of the shape, the knobs (knobs.hpp) and the
// device's CU count: the tabulated parameter sets, the argument checks, every scalar field of DevParams with the host tables
// (derive_params), the launch choice of a dependency-driven run (dag_launch_choice) and the descriptions the getters of
// include/bce_gpu.h answer with.  No HIP call, no environment, no bce_ctx: a machine without a device can ask "what would
// run" (bce_params_derive, bce_dag_launch_choice).  kernel_class (kernels.hpp) is the one thing taken from the kernel files.
#pragma once
#include <vector>

#include "fwd_mfma.hpp"
#include "kernels.hpp"
#include "knobs.hpp"

namespace bce {

struct Shape {
    u32 n = 0, N = 0;
    u64 q = 0, Q = 0, qKS = 0;   // qKS == 0: the key-switch modulus is Q
    u32 baseKS = 0, baseG = 0, baseR = 0;
    int method = 0;
};
// shape of a tabulated set (enum bce_paramset; Q = PreviousPrime(FirstPrime(bits, 2N), 2N)); false: no such set
bool tabulated_shape(int paramset, int method, Shape& out);

struct CtxStatus {
    int code = BCE_OK;
    const char* message = "";   // a literal
};
// the argument checks of bce_ctx_create*, made before the device is asked for
CtxStatus validate_shape(const Shape& s);

// What derive_params builds on the host for upload_ctx to put on the device
struct HostTables {
    std::vector<uint2> twf;         // [N] (psi^brv(i), Shoup companion) in the device layout of kernels.hip (tw_pos)
    std::vector<u32> psi, psi_r2;   // [N] psi^e in natural exponent order, and psi^e R^2 (R = 2^32)
    std::vector<ulonglong2> tw64;   // 64-bit path: [N] (psi^brv(i), floor(. 2^64 / Q)) ...
    std::vector<double2> tw64d;     // ... and (psi^brv(i), psi^brv(i) / Q) for the double-precision formulation
    FwdMfmaTables fwd;              // A operands of the matrix-pipe forward stages (used when P.fwd_mfma)
    bool xcd_gate = false;          // the per-XCD arrival counters are wanted
};
struct CtxParams {
    CtxStatus status;   // not BCE_OK: validate_shape's verdict, or what only the derivation can tell (no kernel for the
                        // shape, a key-switch modulus the tail cannot take, an LDS layout that does not fit); P and T are then partial
    DevParams P{};      // every scalar field; the pointers stay null
    HostTables T;
    u64 psi = 0;        // the minimal primitive 2N-th root of unity mod Q
};
CtxParams derive_params(const Shape& s, const CtxKnobs& knobs, u32 cu_count);

// ---- descriptions of a derived context (the getters of include/bce_gpu.h and bce_params_derive share them) --------------
u32 forward_transforms_per_step(const DevParams& P);
void launch_capacity(const DevParams& P, u32* lone, u32* full);
void bytes_per_bootstrap_parts(const DevParams& P, u64 out[3]);
// out[BCE_D_COUNT] of bce_params_derive, all but BCE_D_dag_lds_bytes (a figure of the kernel files)
void params_report(const CtxParams& cp, u64* out);

// ---- launch choice of bce_dag_run ---------------------------------------------------------------------------------------
struct DagLimits {   // bce_dag_set_limits
    int wg_per_cu = 0, placement = 1;
    u32 lazy_us = 20, stall_ms = 4000;
};
struct DagLaunchChoice {
    int wps = 4;             // 2: one workgroup per CU, 4: two
    u32 grid = 0;
    u32 policy = 0, gate_ticks = 0, gate_backlog = 0, lazy_ticks = 0, stall_ticks = 0;   // DagRearm's fields
    bool rearm_only = false; // development: the persistent kernel is not launched
};
// P: cu_count and is64 are read.  wg_per_cu_full: kernel_class(P)'s.  dag_lds_bytes_wps4: bootstrap_dag_lds_bytes(P, 4) of a
// 32-bit context (not read when P.is64).  depth, items: the DAG's longest chain and tasks x instances.
DagLaunchChoice dag_launch_choice(const DevParams& P, u32 wg_per_cu_full, size_t dag_lds_bytes_wps4, const DagLimits& lim,
                                  const DagKnobs& knobs, u32 depth, u64 items);

}  // namespace bce
