// kv_park.hip — zgml_hip_kv_park / zgml_hip_kv_resume (include/zgml_hip.h): a range of KV columns of every lane of a sequence into
// a host blob and back, so a sequence's state outlives its program and its slot (prompt cache, preemption, persistence). kv_park.h
// states the blob; the payload passes through ONE device staging block the context owns, because the lanes of a sequence are
// thousands of short runs scattered over the plan's buffers (Llama-2-7B: 2048) and a copy per run is the cost shape kv_move was
// written to remove: one launch packs them into (unpacks them from) staging at the directory's offsets, and one copy carries the
// payload over the bus.
//
// The kernel is kv_copy.h's chunk body over (lane, chunk), as kv_move_kernel: the records' blob side points into staging, whose
// runs start on 16-byte boundaries, so the 16-byte path is taken whenever the lane side allows it. A workgroup reads and writes
// only its own chunk: no cross-workgroup ordering, no hand-off. Park: lane -> staging (copy, or quantise under ZGML_KV_PARK_INT8);
// resume: staging -> lane (copy, or quantise an f32 run into an int8 lane: the bytes kv_move writes for f32 -> int8).
#include "runtime_internal.h"

#include "kv_copy.h"
#include "kv_park.h"

// The staging block: device memory for one blob's payload. `done` is recorded behind the block's last use (a park's copy out, a
// resume's unpack launch); a later call waits for it before it overwrites or frees the block.
struct KvParkStage {
    char* dev = nullptr;
    uint64_t cap = 0;
    hipEvent_t done = nullptr;
};

namespace zgml_rt {

void free_kv_park_stage(zgml_hip_ctx* ctx) {
    if (!ctx->kv_park_stage) return;
    (void)hipFree(ctx->kv_park_stage->dev);
    if (ctx->kv_park_stage->done) (void)hipEventDestroy(ctx->kv_park_stage->done);
    delete ctx->kv_park_stage;
    ctx->kv_park_stage = nullptr;
}

namespace {

__global__ void __launch_bounds__(kKvmBlock) kv_park_kernel(const KvMoveLane* __restrict__ lanes, uint32_t chunk) { kvm_lane_chunk<false>(lanes, chunk); }

// the staging block with room for `bytes`, its last use completed; nullptr: reported on the context
KvParkStage* kv_park_stage(zgml_hip_ctx* ctx, uint64_t bytes) {
    if (!ctx->kv_park_stage) {
        ctx->kv_park_stage = new KvParkStage();
        if (!CTX_CHECK(ctx, hipEventCreateWithFlags(&ctx->kv_park_stage->done, hipEventDisableTiming))) return nullptr;
    }
    KvParkStage* st = ctx->kv_park_stage;
    if (!st->done || !CTX_CHECK(ctx, hipEventSynchronize(st->done))) return nullptr; // (an event never recorded counts as complete)
    if (st->cap < bytes) {
        (void)hipFree(st->dev);
        st->dev = nullptr, st->cap = 0;
        const uint64_t cap = std::max<uint64_t>((bytes + 0xFFFFF) & ~(uint64_t)0xFFFFF, 1u << 20); // whole MiB
        if (!CTX_CHECK(ctx, hipMalloc((void**)&st->dev, cap))) return nullptr;
        st->cap = cap;
    }
    return st;
}

// the records of one call, the byte ranges it touches on the lane side and its longest run
struct KvParkCall {
    std::vector<KvMoveLane> recs;
    std::vector<KvRange> ranges; // the lane side
    uint64_t max_elems = 0;
};

// record i of a call over lane `l` of `program` (checked by kv_lane_base: false, *why); the blob side is filled in by the caller
// once staging is known (src / dst hold the blob OFFSETS until then)
bool kv_park_record(zgml_hip_program* program, const zgml_kv_lane& l, const zgml::KvpLaneRec& run, uint32_t col, uint32_t n, bool to_blob, KvParkCall* call,
                    const char** why) {
    char* data;
    float* scales;
    if (!kv_lane_base(program, l, (uint64_t)col + n, why, &data, &scales)) return false;
    const uint64_t dh = l.d_head, elems = (uint64_t)n * dh, bpc = dh / 32, unit = l.block_size ? 1 : 4;
    char* lane_data = data + (uint64_t)col * dh * unit;
    float* lane_scales = scales ? scales + (uint64_t)col * bpc : nullptr;
    char* blob_data = (char*)(uintptr_t)run.data_offset;
    float* blob_scales = run.form == zgml::KVP_I8 ? (float*)(uintptr_t)zgml::kvp_scales_offset(run, n) : nullptr;
    KvMoveLane r;
    r.elems = elems, r._pad = 0;
    if (to_blob) {
        r.mode = l.block_size ? KVM_I8 : (run.form == zgml::KVP_I8 ? KVM_QUANT : KVM_F32);
        r.src = lane_data, r.src_scales = lane_scales, r.dst = blob_data, r.dst_scales = blob_scales;
    } else {
        r.mode = run.form == zgml::KVP_I8 ? KVM_I8 : (l.block_size ? KVM_QUANT : KVM_F32);
        r.src = blob_data, r.src_scales = blob_scales, r.dst = lane_data, r.dst_scales = lane_scales;
    }
    call->recs.push_back(r);
    call->ranges.push_back({(uintptr_t)lane_data, (uintptr_t)lane_data + elems * unit, !to_blob});
    if (lane_scales) call->ranges.push_back({(uintptr_t)lane_scales, (uintptr_t)(lane_scales + (uint64_t)n * bpc), !to_blob});
    call->max_elems = std::max(call->max_elems, elems);
    return true;
}

// blob offsets -> addresses inside staging (which holds the payload alone: offset payload_off of the blob is staging's byte 0)
void kv_park_rebase(KvParkCall* call, char* stage, uint64_t payload_off, bool to_blob) {
    auto at = [&](const void* off) { return off ? stage + ((uintptr_t)off - payload_off) : nullptr; };
    for (KvMoveLane& r : call->recs) {
        if (to_blob)
            r.dst = at(r.dst), r.dst_scales = (float*)at(r.dst_scales);
        else
            r.src = at(r.src), r.src_scales = (const float*)at(r.src_scales);
    }
}

// the records through the pool, then the launch
bool kv_park_launch(zgml_hip_ctx* ctx, const KvParkCall& call, uint32_t chunk) {
    const uint64_t bytes = call.recs.size() * sizeof(KvMoveLane);
    KvPoolBlock* blk = kv_pool_block(ctx, bytes);
    if (!blk) return false;
    memcpy(blk->host, call.recs.data(), bytes);
    if (!kv_pool_upload(ctx, blk, bytes)) return false;
    const dim3 grid((uint32_t)call.recs.size(), (uint32_t)((call.max_elems + chunk - 1) / chunk));
    kv_park_kernel<<<grid, kKvmBlock, 0, ctx->stream>>>((const KvMoveLane*)blk->dev, chunk);
    return CTX_CHECK(ctx, hipGetLastError());
}

} // namespace
} // namespace zgml_rt

extern "C" {

uint64_t zgml_hip_kv_park_bytes(const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t n, uint32_t flags) { return zgml::kvp_park_bytes(lanes, n_lanes, n, flags); }

int zgml_hip_kv_park(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t col, uint32_t n, uint32_t flags, void* blob,
                     uint64_t cap) {
    if (!ctx || !program) return -1;
    auto refuse = [&](uint64_t lane, const char* why) {
        ctx->fail(lane == zgml::kKvpNoLane ? std::string("kv_park: ") + why : "kv_park: lane " + std::to_string(lane) + ": " + why);
        return -1;
    };
    const bool empty = !n || !n_lanes;
    std::vector<zgml::KvpLaneRec> dir(empty || n_lanes > 0x7FFFFFFFull ? 0 : n_lanes); // (the layout refuses more lanes before it fills any record)
    uint64_t lane;
    const char* why = nullptr;
    const uint64_t total = zgml::kvp_park_check(lanes, n_lanes, n, flags, blob, cap, dir.data(), &lane, &why);
    if (!total) return refuse(lane, why);
    if (empty) return zgml::kvp_write_header(blob, 0, 0, flags, total, nullptr), 0;
    KvParkCall call;
    call.recs.reserve(n_lanes), call.ranges.reserve(n_lanes * 2);
    for (uint64_t i = 0; i < n_lanes; i++)
        if (!kv_park_record(program, lanes[i], dir[i], col, n, true, &call, &why)) return refuse(i, why);
    // (a park writes no lane: the range check of kv_move has nothing to refuse on the lane side)
    const uint32_t chunk = kvm_chunk_for(call.max_elems);
    if (!chunk) return refuse(zgml::kKvpNoLane, "more values per lane than one launch carries");

    (void)hipSetDevice(ctx->device);
    const uint64_t payload_off = zgml::kvp_payload_offset(n_lanes), payload = total - payload_off;
    KvParkStage* st = kv_park_stage(ctx, payload);
    if (!st) return -1;
    kv_park_rebase(&call, st->dev, payload_off, true);
    if (!kv_park_launch(ctx, call, chunk)) return -1;
    zgml::kvp_write_header(blob, n_lanes, n, flags, total, dir.data());
    const bool ok = CTX_CHECK(ctx, hipMemcpyAsync((char*)blob + payload_off, st->dev, payload, hipMemcpyDeviceToHost, ctx->stream)) &&
                    CTX_CHECK(ctx, hipEventRecord(st->done, ctx->stream)) && CTX_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ok) zgml::kvp_zero_gaps(blob, dir.data(), n_lanes, n);
    return ok ? 0 : -1;
}

int zgml_hip_kv_resume(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, uint64_t n_lanes, uint32_t col, const void* blob, uint64_t bytes) {
    if (!ctx || !program) return -1;
    auto refuse = [&](uint64_t lane, const char* why) {
        ctx->fail(lane == zgml::kKvpNoLane ? std::string("kv_resume: ") + why : "kv_resume: lane " + std::to_string(lane) + ": " + why);
        return -1;
    };
    zgml::KvpHeader h;
    // (the check fills the directory only behind its own test that the blob holds one of n_lanes records)
    std::vector<zgml::KvpLaneRec> dir(blob && n_lanes <= 0x7FFFFFFFull && bytes >= zgml::kvp_payload_offset(n_lanes) ? n_lanes : 0);
    uint64_t lane;
    const char* why = nullptr;
    if (!zgml::kvp_check_blob(blob, bytes, lanes, n_lanes, &h, dir.data(), &lane, &why)) return refuse(lane, why);
    if (!h.n || !h.n_lanes) return 0;
    KvParkCall call;
    call.recs.reserve(n_lanes), call.ranges.reserve(n_lanes * 2);
    for (uint64_t i = 0; i < n_lanes; i++)
        if (!kv_park_record(program, lanes[i], dir[i], col, h.n, false, &call, &why)) return refuse(i, why);
    if (kv_ranges_clash(call.ranges)) return refuse(zgml::kKvpNoLane, "overlapping destination ranges (a lane listed twice, or two lanes whose written columns meet)");
    const uint32_t chunk = kvm_chunk_for(call.max_elems);
    if (!chunk) return refuse(zgml::kKvpNoLane, "more values per lane than one launch carries");

    (void)hipSetDevice(ctx->device);
    const uint64_t payload_off = zgml::kvp_payload_offset(n_lanes), payload = bytes - payload_off;
    KvParkStage* st = kv_park_stage(ctx, payload);
    if (!st) return -1;
    kv_park_rebase(&call, st->dev, payload_off, false);
    for (uint64_t i = 0; i < n_lanes; i++) unhoist_if_guarded(program, lanes[i].buf);
    // the blob is consumed once the copy into staging has completed: wait for that alone; the unpack launch stays stream-ordered
    if (!CTX_CHECK(ctx, hipMemcpyAsync(st->dev, (const char*)blob + payload_off, payload, hipMemcpyHostToDevice, ctx->stream)) ||
        !CTX_CHECK(ctx, hipEventRecord(st->done, ctx->stream)) || !CTX_CHECK(ctx, hipEventSynchronize(st->done)))
        return -1;
    if (!kv_park_launch(ctx, call, chunk)) return -1;
    return CTX_CHECK(ctx, hipEventRecord(st->done, ctx->stream)) ? 0 : -1;
}

} // extern "C"
