// kv_move.hip — zgml_hip_kv_move (include/zgml_hip.h): a range of KV columns of every cache of a sequence from one compiled program
// to another in ONE launch — the admission of a prefill plan's caches into a slot of a batched plan, and the fork of a slot. Per
// lane pair the columns are copied (f32 -> f32; int8 -> int8: bytes and scales) or quantised (f32 -> int8) exactly as kvq_store
// does (kvq.h states the rule).
//
// The copy and the quantising body of a workgroup's chunk, the record of a lane pair and the chunk size are kv_copy.h's (shared
// with kv_park.hip); this file adds the lane checks, the range check and the pool of record blocks that the lane calls share.
#include "runtime_internal.h"

#include "kv_copy.h"

struct KvMovePool {
    std::vector<zgml_rt::KvPoolBlock> blocks; // (uploaded: recorded behind the block's last upload: the host side is free again once it has passed)
};

namespace zgml_rt {

void free_kv_move_pool(zgml_hip_ctx* ctx) {
    if (!ctx->kv_move_pool) return;
    for (auto& b : ctx->kv_move_pool->blocks) {
        (void)hipHostFree(b.host);
        (void)hipFree(b.dev);
        if (b.uploaded) (void)hipEventDestroy(b.uploaded);
    }
    delete ctx->kv_move_pool;
    ctx->kv_move_pool = nullptr;
}

namespace {

template <bool NT>
__global__ void __launch_bounds__(kKvmBlock) kv_move_kernel(const KvMoveLane* __restrict__ lanes, uint32_t chunk) {
    kvm_lane_chunk<NT>(lanes, chunk);
}

} // namespace

// a free block of the pool with room for `bytes` (its last upload has completed), or a new one
KvPoolBlock* kv_pool_block(zgml_hip_ctx* ctx, uint64_t bytes) {
    if (!ctx->kv_move_pool) ctx->kv_move_pool = new KvMovePool();
    auto& blocks = ctx->kv_move_pool->blocks;
    for (auto& b : blocks)
        if (b.cap >= bytes && hipEventQuery(b.uploaded) == hipSuccess) return &b;
    (void)hipGetLastError(); // (hipErrorNotReady of a busy block is not an error of the call)
    KvPoolBlock b;
    b.cap = std::max<uint64_t>(bytes, 256 * sizeof(KvMoveLane));
    if (!CTX_CHECK(ctx, hipHostMalloc((void**)&b.host, b.cap, hipHostMallocDefault)) || !CTX_CHECK(ctx, hipMalloc((void**)&b.dev, b.cap)) ||
        !CTX_CHECK(ctx, hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming))) {
        (void)hipHostFree(b.host);
        (void)hipFree(b.dev);
        if (b.uploaded) (void)hipEventDestroy(b.uploaded);
        return nullptr;
    }
    blocks.push_back(b);
    return &blocks.back();
}

bool kv_pool_upload(zgml_hip_ctx* ctx, KvPoolBlock* blk, uint64_t bytes) {
    return CTX_CHECK(ctx, hipMemcpyAsync(blk->dev, blk->host, bytes, hipMemcpyHostToDevice, ctx->stream)) && CTX_CHECK(ctx, hipEventRecord(blk->uploaded, ctx->stream));
}

// no written range may meet another written range or a read range (a lane pair that overlaps itself, or two pairs that meet)
bool kv_ranges_clash(std::vector<KvRange>& ranges) {
    std::sort(ranges.begin(), ranges.end(), [](const KvRange& a, const KvRange& b) { return a.lo < b.lo; });
    uintptr_t hi_written = 0, hi_read = 0;
    for (const KvRange& r : ranges) {
        if (r.lo < hi_written || (r.written && r.lo < hi_read)) return true;
        (r.written ? hi_written : hi_read) = std::max(r.written ? hi_written : hi_read, r.hi);
    }
    return false;
}

bool kv_lane_base(zgml_hip_program* p, const zgml_kv_lane& l, uint64_t col_end, const char** why, char** data, float** scales) {
    *data = nullptr, *scales = nullptr;
    if (l.buf >= p->bufs.size() || !p->bufs[l.buf]) return *why = "no such live buffer (dead or elided)", false;
    if (l.block_size != 0 && l.block_size != 32) return *why = "block_size must be 0 (f32 columns) or 32 (the quantised cache layout)", false;
    if (!l.d_head || !l.n_cols) return *why = "d_head and n_cols must not be 0", false;
    if (col_end > l.n_cols) return *why = "columns beyond the lane's n_cols", false;
    const uint64_t vals = (uint64_t)l.n_cols * l.d_head;
    if (l.block_size == 0) {
        if (l.offset > p->sizes[l.buf] || vals > p->sizes[l.buf] - l.offset) return *why = "the lane's extent exceeds its buffer", false;
        *data = (char*)(p->bufs[l.buf] + l.offset);
        return true;
    }
    if (l.d_head % 32) return *why = "an int8 lane needs d_head % 32 == 0", false;
    if (l.offset) return *why = "an int8 lane is a whole cache buffer: offset must be 0", false;
    if (vals % 4 || vals / 4 + vals / 32 > p->sizes[l.buf]) return *why = "the lane's extent exceeds its buffer", false;
    *data = (char*)p->bufs[l.buf];
    *scales = p->bufs[l.buf] + vals / 4;
    return true;
}

} // namespace zgml_rt

extern "C" {

int zgml_hip_kv_move(zgml_hip_ctx* ctx, zgml_hip_program* dst, const zgml_kv_lane* dst_lanes, zgml_hip_program* src, const zgml_kv_lane* src_lanes,
                     uint64_t n_lanes, uint32_t src_col, uint32_t dst_col, uint32_t n) {
    if (!ctx || !dst || !src) return -1;
    if (!n_lanes || !n) return 0;
    auto refuse = [&](uint64_t i, const char* why) {
        ctx->fail("kv_move: lane " + std::to_string(i) + ": " + why);
        return -1;
    };
    if (!dst_lanes || !src_lanes) return refuse(0, "no lane records");
    if (n_lanes > 0x7FFFFFFFull) return refuse(0, "more lanes than one launch carries");
    std::vector<KvMoveLane> recs(n_lanes);
    std::vector<KvRange> ranges;
    ranges.reserve(n_lanes * 4);
    uint64_t max_elems = 0;
    for (uint64_t i = 0; i < n_lanes; i++) {
        const zgml_kv_lane &d = dst_lanes[i], &s = src_lanes[i];
        const char* why = nullptr;
        char *dp, *sp;
        float *dsc, *ssc;
        if (!kv_lane_base(dst, d, (uint64_t)dst_col + n, &why, &dp, &dsc) || !kv_lane_base(src, s, (uint64_t)src_col + n, &why, &sp, &ssc)) return refuse(i, why);
        if (d.d_head != s.d_head) return refuse(i, "d_head of the source and the destination differ");
        if (s.block_size && !d.block_size) return refuse(i, "int8 -> f32 is not a move (a quantised column has no f32 original)");
        KvMoveLane& r = recs[i];
        const uint64_t dh = d.d_head, elems = (uint64_t)n * dh, bpc = dh / 32;
        r.elems = elems, r._pad = 0;
        r.mode = s.block_size ? KVM_I8 : (d.block_size ? KVM_QUANT : KVM_F32);
        const uint64_t s_unit = s.block_size ? 1 : 4, d_unit = d.block_size ? 1 : 4;
        r.src = sp + (uint64_t)src_col * dh * s_unit, r.dst = dp + (uint64_t)dst_col * dh * d_unit;
        r.src_scales = ssc ? ssc + (uint64_t)src_col * bpc : nullptr, r.dst_scales = dsc ? dsc + (uint64_t)dst_col * bpc : nullptr;
        ranges.push_back({(uintptr_t)r.src, (uintptr_t)r.src + elems * s_unit, false});
        ranges.push_back({(uintptr_t)r.dst, (uintptr_t)r.dst + elems * d_unit, true});
        if (r.src_scales) ranges.push_back({(uintptr_t)r.src_scales, (uintptr_t)(r.src_scales + (uint64_t)n * bpc), false});
        if (r.dst_scales) ranges.push_back({(uintptr_t)r.dst_scales, (uintptr_t)(r.dst_scales + (uint64_t)n * bpc), true});
        max_elems = std::max(max_elems, elems);
    }
    if (kv_ranges_clash(ranges)) {
        ctx->fail("kv_move: overlapping source and destination ranges of one buffer (a lane pair may not overlap itself, and no pair may write what another reads or writes)");
        return -1;
    }
    const uint32_t chunk = kvm_chunk_for(max_elems);
    if (!chunk) return refuse(0, "more values per lane than one launch carries");

    (void)hipSetDevice(ctx->device);
    KvPoolBlock* blk = kv_pool_block(ctx, n_lanes * sizeof(KvMoveLane));
    if (!blk) return -1;
    for (uint64_t i = 0; i < n_lanes; i++) unhoist_if_guarded(dst, dst_lanes[i].buf);
    memcpy(blk->host, recs.data(), n_lanes * sizeof(KvMoveLane));
    if (!kv_pool_upload(ctx, blk, n_lanes * sizeof(KvMoveLane))) return -1;
    const dim3 grid((uint32_t)n_lanes, (uint32_t)((max_elems + chunk - 1) / chunk));
    if (ctx->opt_kv_move_nt)
        kv_move_kernel<true><<<grid, kKvmBlock, 0, ctx->stream>>>((const KvMoveLane*)blk->dev, chunk);
    else
        kv_move_kernel<false><<<grid, kKvmBlock, 0, ctx->stream>>>((const KvMoveLane*)blk->dev, chunk);
    return CTX_CHECK(ctx, hipGetLastError()) ? 0 : -1;
}

} // extern "C"
