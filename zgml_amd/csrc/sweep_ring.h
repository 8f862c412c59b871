// sweep_ring.h — the bookkeeping of the granule hand-off's wait (attention_decode.h: DecodeHandoff) as a ring of D sweeps in
// flight. Plain C++: device code and host tests (tests/cpp/sweep_ring_probe.cpp) include it alike, as handoff_gen.h.
//
// A sweep is ONE reading of all the granules a head waits for (handoff_gen.h), ALL its loads issued back to back, each value
// taken together with its own tag. The wait ends with the first sweep in which every tag carries the execution's generation; the
// values handed on are THAT sweep's and no other's: a sweep that mixes generations is dropped whole and read again. Sweeps are
// checked in the order they were issued (the loads of one wave return in order), so the accepting check is the last check.
//
// D > 1 keeps D sweeps issued: the idea is that a granule which becomes visible just behind one sweep's sample is seen by the next
// sweep a D-th of a round trip later instead of a whole one, the oldest slot waited for with a counted vmcnt while D - 1 sweeps'
// loads stay outstanding (sweep_ring_in_flight). As hipcc builds this loop today that is NOT what runs: the loop's header waits
// for every outstanding load, so the sweeps of a round are a burst drained together, and depths 2 and 4 measured slower than 1
// (profiles/r30_sweep_ring.txt sections 6, 7). The kernel keeps D = 1 at d_head 64; the depth stays a parameter so that it can be
// measured again.
//
// The ring is parameterised by what performs a sweep:
//     issue()    -> Sweep   starts a sweep (the kernel: its agent-scope loads; a host probe: a scripted memory)
//     matches(s) -> bool    every tag of the (returned) sweep carries this execution's generation
//     accept(s)             hands the values of a matching sweep on (called at most once, with a sweep that matched)
//     pause(p)              kSweepStagger: between two of the first D issues; kSweepBackoff: behind a failed check
// D == 1: issue, check, pause, issue, check, ...
#pragma once
#include <stdint.h>

#include "handoff_gen.h"

namespace zgml {

// Checked sweeps before a wait gives up (never hang the device: the caller sets the host-visible time-out word). The sequential
// loop's limit, so the wait gives up no later than it did (a checked sweep costs one round trip or less where it cost three) and
// still some five orders of magnitude beyond a legitimate wait (a sweep's trip measures 0.36 us idle and more under load:
// 400000 of them are 144 ms and more, against a wait of 2-3 us: profiles/r30_sweep_ring.txt). Looked at once per round of D sweeps.
constexpr uint32_t kSweepLimit = 400000u;

enum SweepPause { kSweepStagger = 0, kSweepBackoff = 1 };

struct SweepResult {
    bool accepted;    // false: the limit was reached, nothing was handed on
    uint32_t checked; // sweeps whose tags were compared
};

// loads that may still be outstanding when the oldest of D sweeps of `loads_per_sweep` loads is consumed (the counted wait)
ZGML_HANDOFF_HD constexpr int sweep_ring_in_flight(int depth, int loads_per_sweep) { return (depth - 1) * loads_per_sweep; }

// (the slots are D NAMED objects, not an array: the device compiler keeps each in registers of its own whatever it does to the
// D copies of the check, where an indexed slot ends up in scratch memory behind a run-time index)
template <int D, typename Sweep, typename Issue, typename Matches, typename Accept, typename Pause>
ZGML_HANDOFF_HD inline SweepResult sweep_ring(Issue&& issue, Matches&& matches, Accept&& accept, Pause&& pause, uint32_t limit = kSweepLimit) {
    static_assert(D >= 1 && D <= 4, "one to four sweeps in flight");
    Sweep s0 = issue(), s1 = s0, s2 = s0, s3 = s0; // (s1..s3: placeholders until issued; unused ones fold away)
    if constexpr (D > 1) pause(kSweepStagger), s1 = issue();
    if constexpr (D > 2) pause(kSweepStagger), s2 = issue();
    if constexpr (D > 3) pause(kSweepStagger), s3 = issue();
    // One turn of the ring on its oldest slot: accepted, or re-issued behind the D - 1 younger ones.
    // The limit is looked at once per round of D turns: one latch, and every slot is carried round the loop
    // in its own registers (a limit check per turn made the device compiler copy slots in flight at the loop's end, behind a
    // wait for ALL of them).
    uint32_t rounds = 0; // whole rounds of D checked sweeps
    auto turn = [&](Sweep& s) -> bool {
        if (matches(s)) {
            accept(s);
            return true;
        }
        pause(kSweepBackoff);
        s = issue();
        return false;
    };
    for (;;) {
        if (turn(s0)) return SweepResult{true, rounds * D + 1};
        if constexpr (D > 1)
            if (turn(s1)) return SweepResult{true, rounds * D + 2};
        if constexpr (D > 2)
            if (turn(s2)) return SweepResult{true, rounds * D + 3};
        if constexpr (D > 3)
            if (turn(s3)) return SweepResult{true, rounds * D + 4};
        if (++rounds * D >= limit) return SweepResult{false, rounds * D}; // (the sweeps re-issued last are dropped unread)
    }
}

} // namespace zgml
