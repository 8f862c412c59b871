// kv_park.h — the blob of a parked sequence (zgml_hip_kv_park / zgml_hip_kv_resume, include/zgml_hip.h), stated once as host-only
// logic: the runtime (kv_park.hip) and a CPU probe (tests/cpp/kv_park_probe.cpp) both compile it. Little-endian, no pointers.
//
//   header     32 bytes   magic "ZKVP", version, n_lanes (u64), n (columns), flags, total_bytes (u64)
//   directory  16 bytes per lane: d_head, form (0: f32 run, 1: int8 run), data_offset (u64, bytes from the blob's start)
//   payload    per lane, in lane order: the data run — n * d_head floats (f32) or n * d_head bytes (int8) — and for int8 a scale
//              run of n * d_head / 32 floats. EVERY run starts on a 16-byte boundary of the blob (the gaps in front of one are zero);
//              the scale run of lane i starts at the first such boundary behind its data run, the data run of lane i + 1 at the
//              first behind lane i's last run. total_bytes is the boundary behind the last run.
//
// The host writes header, directory and the gaps, the device only the runs. A lane's form is int8 when the lane is int8, or when the
// park asked for ZGML_KV_PARK_INT8 and the lane is f32 (refused unless d_head % 32 == 0: the column rule of kvq.h works on blocks
// of 32). An empty blob (n == 0 or n_lanes == 0) is the bare header with n_lanes = n = 0. A blob that passes kvp_check_blob has
// exactly the offsets kvp_layout gives for its directory's (d_head, form): nothing in it can point outside total_bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include "zgml_hip.h"

namespace zgml {

constexpr uint32_t kKvpMagic = 0x50564B5Au; // the bytes 'Z' 'K' 'V' 'P'
constexpr uint32_t kKvpVersion = 1;
constexpr uint64_t kKvpNoLane = ~(uint64_t)0; // a refusal that is not about one lane
constexpr uint64_t kKvpMaxRun = 1ull << 40;   // values of one lane's run (keeps every offset far from 64 bits)

enum KvpForm : uint32_t { KVP_F32 = 0, KVP_I8 = 1 };
struct KvpHeader {
    uint32_t magic, version;
    uint64_t n_lanes;
    uint32_t n, flags;
    uint64_t total_bytes;
};
struct KvpLaneRec {
    uint32_t d_head, form;
    uint64_t data_offset;
};
static_assert(sizeof(KvpHeader) == 32 && sizeof(KvpLaneRec) == 16, "the blob's records have no padding");

inline uint64_t kvp_align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
inline uint64_t kvp_payload_offset(uint64_t n_lanes) { return sizeof(KvpHeader) + n_lanes * sizeof(KvpLaneRec); }
inline uint64_t kvp_scales_offset(const KvpLaneRec& r, uint32_t n) { return kvp_align16(r.data_offset + (uint64_t)n * r.d_head); } // (int8 runs)
// the 16-byte boundary behind the lane's last run
inline uint64_t kvp_lane_end(const KvpLaneRec& r, uint32_t n) {
    const uint64_t vals = (uint64_t)n * r.d_head;
    return r.form == KVP_I8 ? kvp_align16(kvp_scales_offset(r, n) + vals / 32 * sizeof(float)) : kvp_align16(r.data_offset + vals * sizeof(float));
}
inline uint32_t kvp_form(const zgml_kv_lane& l, uint32_t flags) { return l.block_size || (flags & ZGML_KV_PARK_INT8) ? KVP_I8 : KVP_F32; }

// what a lane record alone can say against parking n of its columns with `flags` (the texts of kv_lane_base where it makes the
// same check; the buffer and the extent are the runtime's to check); nullptr: nothing
inline const char* kvp_lane_shape(const zgml_kv_lane& l, uint32_t n, uint32_t flags) {
    if (l.block_size != 0 && l.block_size != 32) return "block_size must be 0 (f32 columns) or 32 (the quantised cache layout)";
    if (!l.d_head || !l.n_cols) return "d_head and n_cols must not be 0";
    if (n > l.n_cols) return "columns beyond the lane's n_cols";
    if (l.block_size && l.d_head % 32) return "an int8 lane needs d_head % 32 == 0";
    if (l.block_size && l.offset) return "an int8 lane is a whole cache buffer: offset must be 0";
    if (!l.block_size && (flags & ZGML_KV_PARK_INT8) && l.d_head % 32) return "ZGML_KV_PARK_INT8 on an f32 lane needs d_head % 32 == 0";
    if ((uint64_t)n * l.d_head > kKvpMaxRun) return "more values per lane than one launch carries";
    return nullptr;
}

// The layout of a park of n columns of `lanes`: -> total bytes, dir[0 .. n_lanes) filled when dir != nullptr. 0: refused, *why says
// why and *lane which lane (kKvpNoLane: none in particular). n == 0 or n_lanes == 0: the empty blob, whatever the lanes say.
inline uint64_t kvp_layout(const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t n, uint32_t flags, KvpLaneRec* dir, uint64_t* lane, const char** why) {
    *lane = kKvpNoLane, *why = nullptr;
    if (flags & ~(uint32_t)ZGML_KV_PARK_INT8) return *why = "unknown flags", 0;
    if (!n || !n_lanes) return sizeof(KvpHeader);
    if (!lanes) return *why = "no lane records", 0;
    if (n_lanes > 0x7FFFFFFFull) return *why = "more lanes than one launch carries", 0;
    uint64_t off = kvp_payload_offset(n_lanes);
    for (uint64_t i = 0; i < n_lanes; i++) {
        if ((*why = kvp_lane_shape(lanes[i], n, flags))) return *lane = i, 0;
        const KvpLaneRec r{lanes[i].d_head, kvp_form(lanes[i], flags), off};
        if (dir) dir[i] = r;
        off = kvp_lane_end(r, n);
    }
    return off;
}
// zgml_hip_kv_park_bytes
inline uint64_t kvp_park_bytes(const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t n, uint32_t flags) {
    uint64_t lane;
    const char* why;
    return kvp_layout(lanes, n_lanes, n, flags, nullptr, &lane, &why);
}
// ... and what a park checks before it looks at the program: the layout, the blob and its room. -> total bytes, 0: refused
inline uint64_t kvp_park_check(const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t n, uint32_t flags, const void* blob, uint64_t cap, KvpLaneRec* dir,
                               uint64_t* lane, const char** why) {
    *lane = kKvpNoLane;
    if (!blob) return *why = "no blob", 0;
    const uint64_t total = kvp_layout(lanes, n_lanes, n, flags, dir, lane, why);
    if (total && cap < total) return *why = "cap below the blob's size (zgml_hip_kv_park_bytes)", 0;
    return total;
}

// header and directory into the blob (dir: the layout's records; an empty blob has none)
inline void kvp_write_header(void* blob, uint64_t n_lanes, uint32_t n, uint32_t flags, uint64_t total, const KvpLaneRec* dir) {
    const bool empty = !n || !n_lanes;
    const KvpHeader h{kKvpMagic, kKvpVersion, empty ? 0 : n_lanes, empty ? 0 : n, flags, total};
    memcpy(blob, &h, sizeof h);
    if (!empty) memcpy((char*)blob + sizeof h, dir, n_lanes * sizeof(KvpLaneRec));
}

// the gaps between a run's end and the next 16-byte boundary: zero, so equal parks give equal blobs and nothing of the staging
// block's earlier contents leaves the device
inline void kvp_zero_gaps(void* blob, const KvpLaneRec* dir, uint64_t n_lanes, uint32_t n) {
    auto zero = [&](uint64_t end) { memset((char*)blob + end, 0, kvp_align16(end) - end); };
    for (uint64_t i = 0; i < n_lanes; i++) {
        const uint64_t vals = (uint64_t)n * dir[i].d_head;
        if (dir[i].form == KVP_I8)
            zero(dir[i].data_offset + vals), zero(kvp_scales_offset(dir[i], n) + vals / 32 * sizeof(float));
        else
            zero(dir[i].data_offset + vals * sizeof(float));
    }
}

// What a resume checks before it looks at the program: the blob against itself and against the destination's lane records.
// true: *h is the header and (h->n != 0) dir[0 .. n_lanes) the directory, whose offsets are the layout's. The blob may sit at any
// address (every record is copied out).
inline bool kvp_check_blob(const void* blob, uint64_t bytes, const zgml_kv_lane* lanes, uint64_t n_lanes, KvpHeader* h, KvpLaneRec* dir, uint64_t* lane,
                           const char** why) {
    *lane = kKvpNoLane, *why = nullptr;
    if (!blob) return *why = "no blob", false;
    if (bytes < sizeof(KvpHeader)) return *why = "bytes below a header's size", false;
    memcpy(h, blob, sizeof *h);
    if (h->magic != kKvpMagic) return *why = "bad magic (not a parked blob)", false;
    if (h->version != kKvpVersion) return *why = "unknown version", false;
    if (h->total_bytes != bytes) return *why = "bytes differ from the header's total", false;
    if (h->flags & ~(uint32_t)ZGML_KV_PARK_INT8) return *why = "unknown flags", false;
    if (!h->n || !h->n_lanes) {
        if (h->n || h->n_lanes || bytes != sizeof(KvpHeader)) return *why = "an empty blob is a bare header", false;
        return true;
    }
    if (h->n_lanes != n_lanes) return *why = "n_lanes differs from the destination's", false;
    if (!lanes) return *why = "no lane records", false;
    if (n_lanes > 0x7FFFFFFFull) return *why = "more lanes than one launch carries", false;
    if (bytes < kvp_payload_offset(n_lanes)) return *why = "bytes below the directory's size", false;
    uint64_t off = kvp_payload_offset(n_lanes);
    for (uint64_t i = 0; i < n_lanes; i++) {
        KvpLaneRec r;
        memcpy(&r, (const char*)blob + sizeof(KvpHeader) + i * sizeof r, sizeof r);
        *lane = i;
        if (r.form != KVP_F32 && r.form != KVP_I8) return *why = "unknown form of a run", false;
        if (!r.d_head || (r.form == KVP_I8 && r.d_head % 32) || (uint64_t)h->n * r.d_head > kKvpMaxRun) return *why = "a run's d_head is not one a park writes", false;
        if (r.d_head != lanes[i].d_head) return *why = "d_head differs from the destination's", false;
        if (r.form == KVP_I8 && !lanes[i].block_size) return *why = "int8 -> f32 is not a resume (a quantised column has no f32 original)", false;
        if (r.data_offset != off) return *why = "a run's offset is not the layout's", false;
        dir[i] = r;
        off = kvp_lane_end(r, h->n);
    }
    *lane = kKvpNoLane;
    if (off != bytes) return *why = "the header's total is not the layout's", false;
    return true;
}

} // namespace zgml
