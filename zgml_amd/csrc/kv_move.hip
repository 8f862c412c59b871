// kv_move.hip — zgml_hip_kv_move (include/zgml_hip.h): a range of KV columns of every cache of a sequence from one compiled program
// to another in ONE launch — the admission of a prefill plan's caches into a slot of a batched plan, and the fork of a slot. Per
// lane pair the columns are copied (f32 -> f32; int8 -> int8: bytes and scales) or quantised (f32 -> int8) exactly as kvq_store
// does (kvq.h states the rule).
//
// Shape: in every form the moved columns of a lane are ONE contiguous run of n * d_head values on either side (columns lie back to
// back in both layouts), and the scales of an int8 lane a second run of n * d_head / 32 floats. The grid is (lane, chunk): a
// workgroup takes `chunk` values of its lane's run — 16-byte loads and stores where both addresses allow, dwords otherwise. In the
// quantising form a lane of a wave takes 4 dims, so 8 adjacent lanes hold a block of 32 and a wave 8 blocks; the block maximum
// is a shuffle-xor reduction within those 8 lanes (a maximum has no rounding: any order gives kvq_store_kernel's wave_max). No
// workgroup reads what another writes: there is no cross-workgroup ordering, hand-off or loop over work items, and the host
// refuses a call whose destination ranges meet another destination or any source range.
#include "runtime_internal.h"

#include "kvq.h"

enum KvMoveMode : uint32_t { KVM_F32 = 0, KVM_I8 = 1, KVM_QUANT = 2 };
struct KvMoveLane {
    const void* src;         // first moved value of the source (f32: floats; int8: bytes)
    void* dst;               // ... of the destination
    const float* src_scales; // int8 source: scale of the first moved block
    float* dst_scales;       // int8 destination
    uint64_t elems;          // n * d_head values
    uint32_t mode, _pad;
};

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

constexpr int kKvmBlock = 256;
constexpr uint32_t kKvmChunk = 8192; // values per workgroup: 32 KB of f32 — 8 16-byte loads per lane; a multiple of 4 * kKvmBlock

typedef uint32_t kvm_u4 __attribute__((ext_vector_type(4)));
typedef float kvm_f4 __attribute__((ext_vector_type(4)));

// `bytes` (a multiple of 4) from s to d, the workgroup's threads side by side
template <bool NT>
__device__ __forceinline__ void kvm_copy(char* d, const char* s, uint32_t bytes) {
    const uint32_t tid = threadIdx.x;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        const uint32_t n16 = bytes / 16;
        const kvm_u4* s4 = (const kvm_u4*)s;
        kvm_u4* d4 = (kvm_u4*)d;
        constexpr int U = 8; // (a 32 KB chunk is one round: every load of the chunk in flight before the first store)
        uint32_t i = tid;
        for (; i + (U - 1) * kKvmBlock < n16; i += U * kKvmBlock) {
            kvm_u4 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = NT ? __builtin_nontemporal_load(s4 + i + u * kKvmBlock) : s4[i + u * kKvmBlock];
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (NT)
                    __builtin_nontemporal_store(v[u], d4 + i + u * kKvmBlock);
                else
                    d4[i + u * kKvmBlock] = v[u];
            }
        }
        for (; i < n16; i += kKvmBlock) d4[i] = s4[i];
        const uint32_t done = n16 * 16;
        for (uint32_t b = done + 4 * tid; b < bytes; b += 4 * kKvmBlock) *(uint32_t*)(d + b) = *(const uint32_t*)(s + b);
        return;
    }
    for (uint32_t b = 4 * tid; b < bytes; b += 4 * kKvmBlock) *(uint32_t*)(d + b) = *(const uint32_t*)(s + b);
}

template <bool NT>
__global__ void __launch_bounds__(kKvmBlock) kv_move_kernel(const KvMoveLane* __restrict__ lanes, uint32_t chunk) {
    const KvMoveLane& L = lanes[blockIdx.x];
    const uint64_t lo = (uint64_t)blockIdx.y * chunk;
    if (lo >= L.elems) return;
    const uint32_t cnt = (uint32_t)(L.elems - lo < chunk ? L.elems - lo : chunk);
    if (L.mode == KVM_F32) {
        kvm_copy<NT>((char*)L.dst + lo * 4, (const char*)L.src + lo * 4, cnt * 4);
        return;
    }
    if (L.mode == KVM_I8) { // (d_head % 32 == 0: lo and cnt are whole blocks)
        kvm_copy<NT>((char*)L.dst + lo, (const char*)L.src + lo, cnt);
        kvm_copy<NT>((char*)(L.dst_scales + lo / 32), (const char*)(L.src_scales + lo / 32), cnt / 32 * 4);
        return;
    }
    // f32 -> int8: 4 dims per lane, a block of 32 dims on 8 adjacent lanes; cnt is a multiple of 32, so a group of 8 lanes is live or
    // idle as a whole and the loop's trip count is the same for every lane of the workgroup
    const float* src = (const float*)L.src + lo;
    uint32_t* dst = (uint32_t*)((int8_t*)L.dst + lo);
    float* sc = L.dst_scales + lo / 32;
    const bool vec = ((uintptr_t)src & 15) == 0;
    constexpr int QU = 8; // 16-byte loads in flight per lane: a 32 KB chunk is one round (a lone load per round left the kernel latency-bound)
    for (uint32_t base = 0; base < cnt; base += QU * 4 * kKvmBlock) {
        kvm_f4 v[QU];
#pragma unroll
        for (int u = 0; u < QU; u++) {
            const uint32_t e = base + (u * kKvmBlock + threadIdx.x) * 4;
            v[u] = kvm_f4{0.f, 0.f, 0.f, 0.f};
            if (e < cnt) {
                if (vec)
                    v[u] = NT ? __builtin_nontemporal_load((const kvm_f4*)(src + e)) : *(const kvm_f4*)(src + e);
                else
                    v[u] = kvm_f4{src[e], src[e + 1], src[e + 2], src[e + 3]};
            }
        }
#pragma unroll
        for (int u = 0; u < QU; u++) {
            const uint32_t e = base + (u * kKvmBlock + threadIdx.x) * 4;
            float mx = fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
#pragma unroll
            for (int off = 4; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            const KvqScale s = kvq_block_scale(mx);
            const uint32_t w = (uint32_t)(uint8_t)kvq_quantise(v[u].x, s.inv) | (uint32_t)(uint8_t)kvq_quantise(v[u].y, s.inv) << 8 |
                               (uint32_t)(uint8_t)kvq_quantise(v[u].z, s.inv) << 16 | (uint32_t)(uint8_t)kvq_quantise(v[u].w, s.inv) << 24;
            if (e < cnt) {
                dst[e / 4] = w;
                if ((threadIdx.x & 7) == 0) sc[e / 32] = s.scale;
            }
        }
    }
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
    struct Range {
        uintptr_t lo, hi;
        bool written;
    };
    std::vector<KvMoveLane> recs(n_lanes);
    std::vector<Range> ranges;
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
    // no written range may meet another written range or a read range (a lane pair that overlaps itself, or two pairs that meet)
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    uintptr_t hi_written = 0, hi_read = 0;
    for (const Range& r : ranges) {
        if (r.lo < hi_written || (r.written && r.lo < hi_read)) {
            ctx->fail("kv_move: overlapping source and destination ranges of one buffer (a lane pair may not overlap itself, and no pair may write what another reads or writes)");
            return -1;
        }
        (r.written ? hi_written : hi_read) = std::max(r.written ? hi_written : hi_read, r.hi);
    }
    uint32_t chunk = kKvmChunk;
    while ((max_elems + chunk - 1) / chunk > 65535) chunk *= 2;
    if (chunk < kKvmChunk || chunk > (1u << 29)) return refuse(0, "more values per lane than one launch carries"); // (a chunk's byte count stays a 32-bit number)

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
