// knobs.hpp -- every environment variable of the engine: two plain structs and the two functions that read them.  No other
// file of the engine calls getenv; what a knob means is decided where the struct is consumed (ctx_params.cpp).  All sixteen are
// development / parity knobs (DESIGN.md section 5 has the table).  Host-only, no HIP.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace bce {

// development / parity knobs that default to on: NAME=0 switches the feature off
inline bool env_off(const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '0';
}

// a knob whose value is a number, with "unset" kept apart from "0"
struct EnvNumber {
    bool set = false;
    uint32_t value = 0;
};
inline EnvNumber env_number(const char* name) {
    const char* e = std::getenv(name);
    return e ? EnvNumber{true, (uint32_t)std::atoi(e)} : EnvNumber{};
}
// first character of a knob's value (0 for an empty one), -1 when unset
inline int env_char(const char* name) {
    const char* e = std::getenv(name);
    return e ? (unsigned char)e[0] : -1;
}

// Read once per context creation (derive_params)
struct CtxKnobs {
    uint32_t variant = 0;        // BCE_VARIANT: DevParams::variant (0 automatic)
    bool fuse_tail = true;       // BCE_FUSE_TAIL=0: separate tail kernels
    bool occupancy2 = false;     // BCE_OCCUPANCY=2: two workgroups per CU of the one-wave-per-transform kernel wanted
    bool fp64 = true;            // BCE_FP64=0: the integer kernel for Q < 2^39
    bool xcd_gate = true;        // BCE_XCD_GATE=0: no per-XCD arrival counters
    EnvNumber xcd_gate_us;       // BCE_XCD_GATE_US: longest wait at that gate
    bool fold = true;            // BCE_FOLD=0: the plain key
    bool fwd_units = true;       // BCE_FWD_UNITS=0: whole-row + half-row forward bodies
    bool fwd_mfma = true;        // BCE_FWD_MFMA=0: the quarter-unit body without the matrix pipe
};
inline CtxKnobs read_ctx_knobs() {
    CtxKnobs k;
    k.variant = env_number("BCE_VARIANT").value;
    k.fuse_tail = !env_off("BCE_FUSE_TAIL");
    k.occupancy2 = env_char("BCE_OCCUPANCY") == '2';
    k.fp64 = !env_off("BCE_FP64");
    k.xcd_gate = !env_off("BCE_XCD_GATE");
    k.xcd_gate_us = env_number("BCE_XCD_GATE_US");
    k.fold = !env_off("BCE_FOLD");
    k.fwd_units = !env_off("BCE_FWD_UNITS");
    k.fwd_mfma = !env_off("BCE_FWD_MFMA");
    return k;
}

// Read at every bce_dag_run (dag_launch_choice): tests switch them between runs of one context
struct DagKnobs {
    EnvNumber gate_us;           // BCE_DAG_GATE_US: longest wait at the XCD start gate
    EnvNumber gate_backlog;      // BCE_DAG_GATE_BACKLOG: queue depth from which a bootstrap goes through the gate
    // first characters, -1 = unset (env_char)
    int wps = -1;                // BCE_DAG_WPS: '2' = one workgroup per CU, '4' = two; anything else: the rule decides
    int place = -1;              // BCE_DAG_PLACE: unset keeps the context's placement, '0' off, anything else on
    int debug = -1;              // BCE_DAG_DEBUG: 'r' = re-arm only, 'd' = dry run (no bootstraps)
    int gate = -1;               // BCE_DAG_GATE: unset = gate with two workgroups per CU, '0' off, anything else on
    bool tickets = false;        // BCE_DAG_TICKETS=1: tickets for every claim
};
inline DagKnobs read_dag_knobs() {
    DagKnobs k;
    k.gate_us = env_number("BCE_DAG_GATE_US");
    k.gate_backlog = env_number("BCE_DAG_GATE_BACKLOG");
    k.wps = env_char("BCE_DAG_WPS");
    k.place = env_char("BCE_DAG_PLACE");
    k.debug = env_char("BCE_DAG_DEBUG");
    k.gate = env_char("BCE_DAG_GATE");
    k.tickets = env_char("BCE_DAG_TICKETS") == '1';
    return k;
}

}  // namespace bce
