// desc.hpp -- the one rule about the descriptor word `op` (include/bce_gpu.h, bce_gate_desc) on the host: which ops are
// bootstrapped, how many inputs and outputs a descriptor has, and the highest slot it touches.  Header-only, no engine call:
// the engine's argument checks, the DAG analysis (dag_build.cpp) and the schedule module (schedule.cpp) all ask here.
#pragma once
#include <cstdint>

#include "../../include/bce_gpu.h"

namespace bce {

// The descriptor word `op`: bits 0..7 the gate, bits 8..15 the second gate + 1 of a pair (BCE_PAIR, two different gates of
// OR, AND, NOR, NAND on one blind rotation); BCE_XOR is gate byte 6 with bit 16, and the only word with a bit above 15.
// 0: plain descriptor, 1: legal pair, -1: anything else in the high bits.
inline int pair_kind(uint32_t op) {
    if (op <= 0xFFu || op == BCE_XOR) return 0;
    const uint32_t lo = op & 0xFFu, hi = op >> 8;
    return (lo <= BCE_NAND && hi >= 1 && hi - 1 <= BCE_NAND && hi - 1 != lo) ? 1 : -1;
}

enum class DescClass : uint8_t {
    None,      // no op of the engine: an unknown code, or illegal bits 8..
    Gate,      // bootstrapped, two inputs: a plain gate up to BCE_XNOR_FAST, BCE_XOR, or a legal pair
    Refresh,   // BCE_OP_REFRESH: bootstrapped, one input
    Unary,     // BCE_OP_NOT, BCE_OP_COPY: one input, no bootstrap
};
struct DescKind {
    DescClass cls;
    uint8_t inputs, outputs;   // in1 is read only when inputs == 2; a pair writes out and out + 1
    bool boot() const { return cls == DescClass::Gate || cls == DescClass::Refresh; }
    bool pair() const { return outputs == 2; }
};
inline DescKind desc_kind(uint32_t op) {
    if (pair_kind(op) > 0) return {DescClass::Gate, 2, 2};
    if (op <= BCE_XNOR_FAST || op == BCE_XOR) return {DescClass::Gate, 2, 1};
    if (op == BCE_OP_REFRESH) return {DescClass::Refresh, 1, 1};
    if (op == BCE_OP_NOT || op == BCE_OP_COPY) return {DescClass::Unary, 1, 1};
    return {DescClass::None, 0, 1};
}
// the highest slot the descriptor touches (64 bits: out + 1 of a pair may pass 2^32)
inline uint64_t top_slot(const bce_gate_desc& d, DescKind k) {
    uint64_t hi = (uint64_t)d.out + (k.pair() ? 1u : 0u);
    if (d.in0 > hi) hi = d.in0;
    if (k.inputs == 2 && d.in1 > hi) hi = d.in1;
    return hi;
}

}  // namespace bce
