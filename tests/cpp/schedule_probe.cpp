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

// dynamic_field_in_bounds op by op against the schedule of ops[0..n_ops): out[i] for refreshed[i] standing at index i
void zs_dynamic_field_in_bounds(const zgml_device_op* ops, uint64_t n_ops, const uint64_t* sizes, uint64_t n_sizes, const uint32_t* seq_kv_bound,
                                const zgml_device_op* refreshed, uint8_t* out) {
    std::vector<uint32_t> bound;
    if (seq_kv_bound) bound.assign(seq_kv_bound, seq_kv_bound + n_ops);
    const zgml::Schedule s = zgml::build_schedule(std::vector<zgml_device_op>(ops, ops + n_ops), std::vector<uint64_t>(sizes, sizes + n_sizes), {},
                                                  seq_kv_bound ? &bound : nullptr);
    for (uint64_t i = 0; i < n_ops; i++) out[i] = zgml::dynamic_field_in_bounds(s, i, refreshed[i]) ? 1 : 0;
}

// dyn_field(*op) as words: out[0] role (0 none, 1 offset, 2 seq_kv), out[1] moves(), out[2] base, out[3] stride, out[4] whether there is
// a word, out[5..8] at(0, 1), at(0, 4), at(5, 1), at(5, 4); the const overload must agree (out[9]). Then `poke` is written THROUGH the
// word (when there is one): the caller reads it back from the struct field it is supposed to alias.
void zs_dyn_field(zgml_device_op* op, uint32_t poke, uint32_t* out) {
    const zgml::DynField f = zgml::dyn_field(*op);
    const zgml::DynField g = zgml::dyn_field(*const_cast<const zgml_device_op*>(op));
    out[0] = f.role == zgml::DynField::Offset ? 1 : f.role == zgml::DynField::SeqKv ? 2 : 0;
    out[1] = f.moves() ? 1 : 0, out[2] = f.base, out[3] = f.stride, out[4] = f.word ? 1 : 0;
    out[5] = f.at(0, 1), out[6] = f.at(0, 4), out[7] = f.at(5, 1), out[8] = f.at(5, 4);
    out[9] = g.word == f.word && g.role == f.role && g.base == f.base && g.stride == f.stride ? 1 : 0;
    if (f.word) *f.word = poke;
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
