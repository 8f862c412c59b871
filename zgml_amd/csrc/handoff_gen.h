// handoff_gen.h — the generation rule of the in-launch q / k / v hand-off (qmatvec.hip: QmvPublish, attention_decode.h:
// DecodeHandoff). Plain C++: device code and host tests (tests/cpp/handoff_gen_probe.cpp) include it alike.
//
// A hand-off granule is 8 bytes, {value bits : 32, generation : 32}, written by ONE naturally aligned 8-byte store. Producers
// (one word per column group) and consumers (one word per attention workgroup) each keep a private generation that starts at 0
// and is advanced once per execution by its owner; nothing is zeroed between executions, so the state survives graph replay.
// The granule area is zeroed once, and generation 0 is never written: a zeroed granule, or one of an earlier execution, never
// matches the generation an execution waits for.
#pragma once
#include <stdint.h>
#include <type_traits>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZGML_HANDOFF_HD __host__ __device__
#else
#define ZGML_HANDOFF_HD
#endif

namespace zgml {

ZGML_HANDOFF_HD constexpr uint32_t handoff_next_gen(uint32_t g) { return g + 1u ? g + 1u : 1u; } // 1, 2, ..., 0xFFFFFFFF, 1, ...

ZGML_HANDOFF_HD constexpr unsigned long long handoff_granule(uint32_t value_bits, uint32_t gen) {
    return (unsigned long long)value_bits | ((unsigned long long)gen << 32);
}
ZGML_HANDOFF_HD constexpr uint32_t handoff_granule_gen(unsigned long long granule) { return (uint32_t)(granule >> 32); }
ZGML_HANDOFF_HD constexpr uint32_t handoff_granule_value(unsigned long long granule) { return (uint32_t)granule; }

static_assert(handoff_next_gen(0u) == 1u && handoff_next_gen(0xFFFFFFFEu) == 0xFFFFFFFFu && handoff_next_gen(0xFFFFFFFFu) == 1u,
              "generations run 1 .. 0xFFFFFFFF and skip 0");

// The COUNTER form of an in-launch q / k / v hand-off, kept by the 256-thread fused launch of K-on-lanes weights (qmatvec.hip:
// qkv_attn_kon_kernel; with 256 attention workgroups sweeping beside 768 streaming ones the granule form lost 0.6 % at position 1900 of
// Llama-2-7B: profiles/r21_handoff_granules.txt) and by the opt-in K-split path (ksplit.hip, its own producer): one monotonic counter per
// head slice of each projection, bumped once by every column group that has stored its outputs write-through and drained. The
// attention waits (bounded) for its head's three counters to pass `seen + need`, remembers the new values in its private `seen`
// words (kv heads have several consumers, so the shared counters are never reset) and reads q / k / v with agent-scope loads.
struct CounterHandoff {
    const uint32_t* cnt; // [n_heads | n_kv | n_kv] monotonic counters, 32 words apart
    uint32_t* seen;      // [workgroups of the attention part][3]
    const uint32_t* idx; // [records][3]: the q / k / v counters of each record's head (records need not be in head order)
    uint32_t n_heads;
    uint32_t need;       // column groups per head slice = d_head / 16
    uint32_t* timeout;   // set when a wait gives up
    uint32_t poll_sleep; // s_sleep(1) units (64 clocks) between two polls
};

} // namespace zgml
