// handoff_gen_probe — walks the generation rule of the in-launch q / k / v hand-off (zgml_amd/csrc/handoff_gen.h) on the CPU for
// tests/test_hip_handoff_granules.py. A producer word and a consumer word both start at 0 and are advanced once per execution by
// their owners. The probe advances both one step at a time: 2^20 executions from 0, then — every value of 1 .. 0xFFFFFFFF is on the
// walk from 0, so both words are set to 0xFFFFFFFF - 2^20 — 2^21 executions across the wrap. Exit status 0 and "ok=1" mean: the
// two stayed equal, no generation was 0, and no execution waited for the tag that the execution before it had left in the granule
// (or for the zero of a fresh granule).
#include <stdint.h>
#include <stdio.h>

#include "../../zgml_amd/csrc/handoff_gen.h"

using zgml::handoff_granule;
using zgml::handoff_granule_gen;
using zgml::handoff_granule_value;
using zgml::handoff_next_gen;

static_assert(handoff_next_gen(0u) == 1u, "a fresh word's first generation is 1");
static_assert(handoff_next_gen(0xFFFFFFFFu) == 1u, "the wrap skips 0");
static_assert(handoff_granule_gen(handoff_granule(0x3F800000u, 7u)) == 7u && handoff_granule_value(handoff_granule(0x3F800000u, 7u)) == 0x3F800000u,
              "a granule holds the value's bits and the generation side by side");
static_assert(handoff_granule_gen(0ull) == 0u, "a zeroed granule carries generation 0, which is never waited for");

struct Walk {
    uint32_t producer = 0, consumer = 0;
    unsigned long long granule = 0; // zeroed once, then only ever written by the producer
    unsigned long long steps = 0, zeros = 0, unequal = 0, stale_match = 0;
    void run(unsigned long long n) {
        for (unsigned long long i = 0; i < n; i++, steps++) {
            const uint32_t want = handoff_next_gen(consumer);    // what this execution's consumer waits for
            stale_match += handoff_granule_gen(granule) == want; // ... must not be what the granule still holds
            const uint32_t gen = handoff_next_gen(producer);
            granule = handoff_granule((uint32_t)steps, gen);
            zeros += gen == 0u || want == 0u;
            unequal += gen != want || handoff_granule_gen(granule) != want;
            producer = gen, consumer = want; // both owners write their word back
        }
    }
};

int main() {
    Walk w;
    w.run(1ull << 20);
    const bool first_ok = w.producer == (1u << 20) && w.consumer == w.producer;
    const uint32_t near = 0xFFFFFFFFu - (1u << 20);
    w.producer = w.consumer = near, w.granule = handoff_granule(0u, near);
    w.run(1ull << 21); // 2^20 steps reach 0xFFFFFFFF, the next one gives 1, 2^20 - 1 more give 2^20
    const bool ok = first_ok && !w.zeros && !w.unequal && !w.stale_match && w.producer == (1u << 20) && w.consumer == w.producer;
    printf("steps=%llu zeros=%llu unequal=%llu stale_match=%llu last=%u next_of_max=%u next_of_zero=%u ok=%d\n", w.steps, w.zeros, w.unequal, w.stale_match,
           w.producer, handoff_next_gen(0xFFFFFFFFu), handoff_next_gen(0u), ok ? 1 : 0);
    return ok ? 0 : 1;
}
