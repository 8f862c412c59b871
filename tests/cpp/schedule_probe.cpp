// schedule_probe.cpp — a C shim over zgml::build_schedule (zgml_amd/csrc/schedule.hip, compiled as plain C++ next to it) for
// tests/test_schedule.py: the dependency schedule is pure host code, so its properties are checked without a GPU.
#include <cstdint>
#include <vector>

#include "../../zgml_amd/csrc/schedule.h"

extern "C" {

// The schedule of ops[0..n_ops): level[i] per op, and every declared access span as one row of 7 words
// (op, is_write, buf, lo, hi, period, width) in `spans` (at most spans_cap rows; *n_spans receives how many there are).
// `seq_kv_bound`: NULL or one entry per op. `refreshed`: NULL, or an op list of the same length checked with
// dynamic_fields_in_bounds against the schedule — returns 1 / 0 for it, -1 when none is given.
int zs_schedule(const zgml_device_op* ops, uint64_t n_ops, const uint64_t* sizes, uint64_t n_sizes, const uint64_t* barriers,
                uint64_t n_barriers, const uint32_t* seq_kv_bound, const zgml_device_op* refreshed, uint32_t* level, uint64_t* spans,
                uint64_t spans_cap, uint64_t* n_spans) {
    const std::vector<zgml_device_op> v(ops, ops + n_ops);
    const std::vector<uint64_t> sz(sizes, sizes + n_sizes), bar(barriers, barriers + n_barriers);
    std::vector<uint32_t> bound;
    if (seq_kv_bound) bound.assign(seq_kv_bound, seq_kv_bound + n_ops);
    const zgml::Schedule s = zgml::build_schedule(v, sz, bar, seq_kv_bound ? &bound : nullptr);
    for (uint64_t i = 0; i < n_ops; i++) level[i] = s.level[i];
    uint64_t k = 0;
    auto put = [&](uint64_t op, bool w, const zgml::Span& sp) {
        if (k < spans_cap) {
            uint64_t* r = spans + 7 * k;
            r[0] = op, r[1] = w ? 1 : 0, r[2] = sp.buf, r[3] = sp.lo, r[4] = sp.hi, r[5] = sp.period, r[6] = sp.width;
        }
        k++;
    };
    for (uint64_t i = 0; i < n_ops; i++) {
        for (const zgml::Span& sp : s.access[i].reads) put(i, false, sp);
        for (const zgml::Span& sp : s.access[i].writes) put(i, true, sp);
    }
    *n_spans = k;
    if (!refreshed) return -1;
    return zgml::dynamic_fields_in_bounds(s, std::vector<zgml_device_op>(refreshed, refreshed + n_ops)) ? 1 : 0;
}

// spans_overlap for every pair of the n spans given as rows of 5 words (buf, lo, hi, period, width): out[i * n + j]
void zs_overlap_matrix(const uint64_t* rows, uint64_t n, uint8_t* out) {
    std::vector<zgml::Span> sp(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t* r = rows + 5 * i;
        sp[i].buf = (uint16_t)r[0], sp[i].lo = r[1], sp[i].hi = r[2], sp[i].period = r[3], sp[i].width = r[4];
    }
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t j = 0; j < n; j++) out[i * n + j] = zgml::spans_overlap(sp[i], sp[j]) ? 1 : 0;
}

} // extern "C"
