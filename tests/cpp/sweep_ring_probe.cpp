// sweep_ring_probe — drives the ring of the granule hand-off's wait (zgml_amd/csrc/sweep_ring.h) on the CPU with a scripted memory:
// 12 granules (the producer lines of one head: 4 of q, 4 of k, 4 of v at d_head 64) turn from the old generation to the new one
// at chosen ISSUE indices; a sweep issued as the t-th reads granule i new iff t >= flip[i]. Checked for D = 1..4:
//   - a result is accepted only from a sweep in which all tags matched, and carries that sweep's values (the FIRST such sweep issued);
//   - a sweep that mixes generations is never accepted, and no value of it reaches the output;
//   - the loop ends at the limit and reports it;
//   - the accepting check is the LAST check: no sweep is looked at behind it (the kernel stages every checked sweep in LDS and
//     relies on the one staged last being the accepted one);
//   - D = 1 visits memory exactly as the sequential loop does (but for one sweep issued and dropped unread when it gives up).
// Built stand-alone (tests/test_sweep_ring_host.py: g++ -fsanitize=address,undefined) and run directly.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../zgml_amd/csrc/sweep_ring.h"

using namespace zgml;

namespace {
constexpr int NG = 12;
constexpr uint32_t OLD_GEN = 6, NEW_GEN = 7, NEVER = 0xFFFFFFFFu;
struct Sweep {
    unsigned long long g[NG];
    uint32_t t; // its issue index (the probe's own: the ring does not look at it)
};
uint32_t old_value(int i) { return 0x1000u + i; }
uint32_t new_value(int i) { return 0x2000u + i; }

struct Run {
    SweepResult res{};
    std::string log;       // I<t> issue, C<t> check, S stagger, B back-off
    int accepts = 0, mixed_accepted = 0, old_values_out = 0, staggers = 0, checks_after_accept = 0;
    uint32_t accepted_t = NEVER, last_checked_t = NEVER, issues = 0;
    uint32_t out[NG] = {};
};

template <int D>
Run run_ring(const uint32_t (&flip)[NG], uint32_t limit) {
    Run r;
    auto issue = [&]() {
        Sweep s;
        s.t = r.issues++;
        for (int i = 0; i < NG; i++) s.g[i] = s.t >= flip[i] ? handoff_granule(new_value(i), NEW_GEN) : handoff_granule(old_value(i), OLD_GEN);
        r.log += "I" + std::to_string(s.t) + " ";
        return s;
    };
    auto matches = [&](const Sweep& s) {
        r.log += "C" + std::to_string(s.t) + " ";
        r.checks_after_accept += r.accepts > 0;
        r.last_checked_t = s.t;
        bool ok = true;
        for (int i = 0; i < NG; i++) ok = ok && handoff_granule_gen(s.g[i]) == NEW_GEN;
        return ok;
    };
    auto accept = [&](const Sweep& s) {
        r.accepts++, r.accepted_t = s.t;
        for (int i = 0; i < NG; i++) {
            if (handoff_granule_gen(s.g[i]) != NEW_GEN) r.mixed_accepted++;
            r.out[i] = handoff_granule_value(s.g[i]);
            if (r.out[i] != new_value(i)) r.old_values_out++;
        }
    };
    auto pause = [&](SweepPause p) {
        r.log += p == kSweepStagger ? "S " : "B ";
        r.staggers += p == kSweepStagger;
    };
    r.res = sweep_ring<D, Sweep>(issue, matches, accept, pause, limit);
    return r;
}

// the loop the ring replaces (attention_decode.h before the ring): issue, check, back off, issue, ...
std::string sequential_log(const uint32_t (&flip)[NG], uint32_t limit) {
    std::string log;
    uint32_t last = 0;
    for (int i = 0; i < NG; i++) last = flip[i] > last ? flip[i] : last;
    for (uint32_t t = 0;; t++) {
        log += "I" + std::to_string(t) + " C" + std::to_string(t) + " ";
        if (t >= last) return log;
        log += "B ";
        // (the one difference, on the give-up path alone: the ring looks at the limit once per round, behind the round's last
        // re-issue, so one more sweep is issued and dropped unread where the old loop stopped in front of its sleep)
        if (t + 1 >= limit) return log + "I" + std::to_string(t + 1) + " ";
    }
}

int failures = 0;
void expect(bool ok, const char* what, const char* script, int d) {
    if (!ok) failures++, printf("FAIL D=%d %s: %s\n", d, script, what);
}

template <int D>
void check_script(const char* name, const uint32_t (&flip)[NG]) {
    uint32_t last = 0;
    for (int i = 0; i < NG; i++) last = flip[i] > last ? flip[i] : last;
    const Run r = run_ring<D>(flip, 1000);
    expect(r.res.accepted && r.accepts == 1, "accepted exactly once", name, D);
    expect(r.mixed_accepted == 0, "no mixed sweep accepted", name, D);
    expect(r.old_values_out == 0, "the output carries the accepted sweep's values only", name, D);
    expect(r.checks_after_accept == 0 && r.last_checked_t == r.accepted_t, "the accepted sweep is the one checked last: nothing is checked behind it", name, D);
    expect(r.accepted_t == last, "the FIRST sweep issued with every granule new is the one accepted", name, D);
    expect(r.res.checked == last + 1, "every older sweep was checked and dropped, in issue order", name, D);
    expect(r.staggers == D - 1, "D - 1 staggered first issues", name, D);
    expect(r.issues <= last + (uint32_t)D, "never more than D sweeps in flight", name, D);
    if (D == 1) expect(r.log == sequential_log(flip, 1000), "D = 1 visits memory as the sequential loop", name, D);
}

template <int D>
void check_limit() {
    uint32_t flip[NG];
    for (int i = 0; i < NG; i++) flip[i] = i == 5 ? NEVER : 0; // one producer never publishes
    for (uint32_t limit : {1u, 7u, 10u, 400u}) {
        const Run r = run_ring<D>(flip, limit);
        expect(!r.res.accepted && r.accepts == 0, "the limit ends the loop and nothing is handed on", "one line never", D);
        expect(r.res.checked >= limit && r.res.checked < limit + D, "gives up at the limit (looked at once per round)", "one line never", D);
        if (D == 1) expect(r.log == sequential_log(flip, limit), "D = 1 gives up as the sequential loop", "one line never", D);
    }
}

template <int D>
void check_all() {
    uint32_t f[NG];
    for (int i = 0; i < NG; i++) f[i] = 0;
    check_script<D>("all there at the first sweep", f);
    for (int i = 0; i < NG; i++) f[i] = 5;
    check_script<D>("all at once at sweep 5", f);
    for (int i = 0; i < NG; i++) f[i] = i + 1;
    check_script<D>("one by one, first line first", f);
    for (int i = 0; i < NG; i++) f[i] = NG - i;
    check_script<D>("one by one, last line first", f);
    for (int i = 0; i < NG; i++) f[i] = i == NG - 1 ? 57 : 2;
    check_script<D>("the last line a straggler", f);
    for (int i = 0; i < NG; i++) f[i] = i == 0 ? 58 : 3;
    check_script<D>("the first line a straggler", f);
    for (int i = 0; i < NG; i++) f[i] = (i * 7) % NG + (i % 3 == 0 ? 9 : 0);
    check_script<D>("scattered", f);
    check_limit<D>();
}
} // namespace

static_assert(sweep_ring_in_flight(1, 3) == 0 && sweep_ring_in_flight(2, 3) == 3 && sweep_ring_in_flight(4, 6) == 18, "loads behind the oldest sweep");

int main() {
    check_all<1>(), check_all<2>(), check_all<3>(), check_all<4>();
    printf("ok=%d failures=%d\n", failures == 0, failures);
    return failures != 0;
}
