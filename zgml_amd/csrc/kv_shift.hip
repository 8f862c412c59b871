// kv_shift.hip — zgml_hip_kv_shift (include/zgml_hip.h): the context shift of every KV lane of a sequence in ONE launch. Columns
// [keep + discard, n_filled) of a lane move down to [keep, n_filled - discard) in place; a K lane's moved keys are turned back by
// `discard` positions of RoPE on the way (kv_shift.h states the rule and the column map; the kernel calls its kvs_rotate /
// kvs_dequantise and kvq.h's scale and quantiser, so a device column is the header's column to the bit).
//
// Shape: the in-place hazard decides it. Source and destination runs of a lane overlap whenever more columns move than are
// dropped, and workgroups have no order among themselves, so ONE workgroup owns a lane and walks its moved columns in ascending
// ROUNDS. Within a round every thread loads its share into registers, waits until those loads have COMPLETED (s_waitcnt vmcnt(0):
// issued is not enough, a store of another wave could overtake an outstanding load), meets the others at one __syncthreads(), and
// only then stores. Why one barrier per round is enough for a left shift: round r reads [s + rR, s + (r + 1)R) and writes
// [d + rR, d + (r + 1)R) with d < s, so everything rounds <= r write lies below s + (r + 1)R, where round r + 1 starts reading:
// a round never writes what a LATER round reads, and what it writes over in its own or an earlier round's source has been read
// by every thread in front of this or an earlier barrier. There is no cross-workgroup hand-off, no spinning and no atomics; the
// host refuses lanes whose extents meet, so no workgroup touches another's bytes.
//
// Per column. f32 K: a thread takes 4 consecutive `lo` dims and their 4 `hi` partners (hd dims further) as two 16-byte loads where
// the lane's base and d_head allow, one pair as two dwords otherwise (a lane at an odd f32 offset, d_head % 8 != 0). int8 K: a
// thread takes 4 `lo` bytes and their 4 `hi` partners as two dwords plus the two blocks' scales; a 32-block lies on 8 adjacent
// lanes (its `lo` and `hi` halves on 4 at d_head 32), and the block maximum of the ROTATED values is a shuffle-xor reduction over
// them, as in kv_move_kernel's quantising form (a maximum has no rounding: any order gives kvq_quantise_column's). V lanes and
// int8 V lanes are byte runs moved left in the same rounds, 16 bytes per thread where both addresses allow.
#include "runtime_internal.h"

#include "kv_shift.h"

enum KvShiftKind : uint32_t { KVS_F32_COPY = 0, KVS_F32_ROTATE = 1, KVS_I8_COPY = 2, KVS_I8_ROTATE = 3 };
struct KvShiftLane {
    char* data;    // column 0 of the lane (f32: floats; int8: bytes)
    float* scales; // int8: column 0's scales
    uint32_t kind, _pad;
};

namespace zgml_rt {
namespace {

constexpr uint32_t kKvsBlock = 256;

typedef uint32_t kvs_u4 __attribute__((ext_vector_type(4)));
typedef float kvs_f4 __attribute__((ext_vector_type(4)));

// the one barrier of a round: every load the thread has issued has returned its data, then the workgroup meets
__device__ __forceinline__ void kvs_round_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// `bytes` (a multiple of 4) from s down to d < s, in ascending rounds of U accesses per thread. T: kvs_u4 (both 16-byte aligned: a
// round is kKvsCopyRound bytes) or uint32_t (the fallback of unaligned runs: a quarter of that, at the same register cost)
template <typename T>
__device__ __forceinline__ void kvs_move_left_as(char* d, const char* s, uint64_t bytes) {
    constexpr uint32_t U = zgml::kKvsCopyRound / (16 * kKvsBlock);
    const uint64_t n = bytes / sizeof(T);
    const T* sp = (const T*)s;
    T* dp = (T*)d;
    for (uint64_t base = 0; base < n; base += (uint64_t)U * kKvsBlock) {
        T v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint64_t i = base + u * kKvsBlock + threadIdx.x;
            v[u] = T{};
            if (i < n) v[u] = sp[i];
        }
        kvs_round_barrier();
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint64_t i = base + u * kKvsBlock + threadIdx.x;
            if (i < n) dp[i] = v[u];
        }
    }
}
__device__ __forceinline__ void kvs_move_left(char* d, const char* s, uint64_t bytes) {
    if (!bytes) return;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        kvs_move_left_as<kvs_u4>(d, s, bytes & ~(uint64_t)15);
        // (the dwords behind the last 16 bytes: their source lies above everything written so far)
        const uint64_t done = bytes & ~(uint64_t)15;
        if (done < bytes) kvs_move_left_as<uint32_t>(d + done, s + done, bytes - done);
        return;
    }
    kvs_move_left_as<uint32_t>(d, s, bytes);
}

// f32 K lane. W = 4: an item is 4 `lo` dims and their 4 partners (16-byte accesses); W = 1: one pair (dwords)
template <uint32_t W>
__device__ __forceinline__ void kvs_rotate_f32(float* lane, const float* cs, uint32_t dh, uint32_t keep, uint32_t discard, uint32_t n_move) {
    typedef float T __attribute__((ext_vector_type(W)));
    constexpr uint32_t U = zgml::kKvsRotateRound / (8 * kKvsBlock); // items per thread and round (W = 1: a round is a quarter of kKvsRotateRound)
    const uint32_t hd = dh / 2, ipc = hd / W;                           // items per column (<= U * kKvsBlock: the host keeps d_head <= 2048)
    const uint32_t cpr = U * kKvsBlock / ipc;                           // columns per round
    float* dst = lane + (uint64_t)keep * dh;
    const float* src = dst + (uint64_t)discard * dh;
    // kKvsBlock % ipc == 0 (every power-of-two d_head): a thread's dims are the same in every item, and so are its c and s
    const bool fixed = kKvsBlock % ipc == 0;
    T c = T{}, s = T{};
    if (fixed) c = *(const T*)(cs + (threadIdx.x % ipc) * W), s = *(const T*)(cs + hd + (threadIdx.x % ipc) * W);
    for (uint32_t c0 = 0; c0 < n_move; c0 += cpr) {
        const uint32_t n_items = (n_move - c0 < cpr ? n_move - c0 : cpr) * ipc;
        T lo[U], hi[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t t = u * kKvsBlock + threadIdx.x, col = t / ipc, i = (t - col * ipc) * W;
            lo[u] = T{}, hi[u] = T{};
            if (t < n_items) {
                const float* p = src + (uint64_t)(c0 + col) * dh + i;
                lo[u] = *(const T*)p, hi[u] = *(const T*)(p + hd);
            }
        }
        kvs_round_barrier();
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t t = u * kKvsBlock + threadIdx.x, col = t / ipc, i = (t - col * ipc) * W;
            if (t < n_items) {
                if (!fixed) c = *(const T*)(cs + i), s = *(const T*)(cs + hd + i);
                T rl, rh;
#pragma unroll
                for (uint32_t k = 0; k < W; k++) {
                    const zgml::KvsPair r = zgml::kvs_rotate(lo[u][k], hi[u][k], c[k], s[k]);
                    rl[k] = r.lo, rh[k] = r.hi;
                }
                float* p = dst + (uint64_t)(c0 + col) * dh + i;
                *(T*)p = rl, *(T*)(p + hd) = rh;
            }
        }
    }
}

__device__ __forceinline__ float kvs_max4(kvs_f4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
__device__ __forceinline__ uint32_t kvs_quantise4(kvs_f4 v, float inv) {
    return (uint32_t)(uint8_t)zgml::kvq_quantise(v.x, inv) | (uint32_t)(uint8_t)zgml::kvq_quantise(v.y, inv) << 8 |
           (uint32_t)(uint8_t)zgml::kvq_quantise(v.z, inv) << 16 | (uint32_t)(uint8_t)zgml::kvq_quantise(v.w, inv) << 24;
}

// int8 K lane (d_head 32 or a multiple of 64): an item is 4 `lo` bytes and their 4 partners; ipc = hd / 4 items per column lie on
// adjacent lanes of one wave in groups of 8 (4 at d_head 32) that start at a multiple of their size — ipc and kKvsBlock are both
// multiples of it —, so a group is live or idle as a whole and every lane of a wave runs every shuffle
__device__ __forceinline__ void kvs_rotate_i8(char* q, float* scales, const float* cs, uint32_t dh, uint32_t keep, uint32_t discard, uint32_t n_move) {
    constexpr uint32_t U = zgml::kKvsRotateRound / (8 * kKvsBlock);
    const uint32_t hd = dh / 2, ipc = hd / 4, bpc = dh / 32;
    const uint32_t cpr = U * kKvsBlock / ipc;
    const bool one_block = dh == 32; // `lo` and `hi` share the column's only block
    char* dq = q + (uint64_t)keep * dh;
    const char* sq = dq + (uint64_t)discard * dh;
    float* dsc = scales + (uint64_t)keep * bpc;
    const float* ssc = dsc + (uint64_t)discard * bpc;
    const bool fixed = kKvsBlock % ipc == 0;
    kvs_f4 c = kvs_f4{0.f, 0.f, 0.f, 0.f}, s = c;
    if (fixed) c = *(const kvs_f4*)(cs + (threadIdx.x % ipc) * 4), s = *(const kvs_f4*)(cs + hd + (threadIdx.x % ipc) * 4);
    for (uint32_t c0 = 0; c0 < n_move; c0 += cpr) {
        const uint32_t n_items = (n_move - c0 < cpr ? n_move - c0 : cpr) * ipc;
        uint32_t wlo[U], whi[U];
        float slo[U], shi[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t t = u * kKvsBlock + threadIdx.x, col = t / ipc, i = (t - col * ipc) * 4;
            wlo[u] = whi[u] = 0, slo[u] = shi[u] = 0.f;
            if (t < n_items) {
                const char* p = sq + (uint64_t)(c0 + col) * dh + i;
                const float* ps = ssc + (uint64_t)(c0 + col) * bpc;
                wlo[u] = *(const uint32_t*)p, whi[u] = *(const uint32_t*)(p + hd);
                slo[u] = ps[i / 32], shi[u] = ps[(hd + i) / 32];
            }
        }
        kvs_round_barrier();
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t t = u * kKvsBlock + threadIdx.x, col = t / ipc, i = (t - col * ipc) * 4;
            const bool live = t < n_items;
            if (!fixed && live) c = *(const kvs_f4*)(cs + i), s = *(const kvs_f4*)(cs + hd + i);
            kvs_f4 rl, rh;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const float lo = zgml::kvs_dequantise((int8_t)(wlo[u] >> (8 * k)), slo[u]), hi = zgml::kvs_dequantise((int8_t)(whi[u] >> (8 * k)), shi[u]);
                const zgml::KvsPair r = zgml::kvs_rotate(lo, hi, c[k], s[k]);
                rl[k] = r.lo, rh[k] = r.hi;
            }
            float mlo = kvs_max4(rl), mhi = kvs_max4(rh);
            if (one_block) {
                mlo = fmaxf(mlo, mhi);
#pragma unroll
                for (int off = 2; off > 0; off >>= 1) mlo = fmaxf(mlo, __shfl_xor(mlo, off, 64));
                mhi = mlo;
            } else {
#pragma unroll
                for (int off = 4; off > 0; off >>= 1) mlo = fmaxf(mlo, __shfl_xor(mlo, off, 64)), mhi = fmaxf(mhi, __shfl_xor(mhi, off, 64));
            }
            const zgml::KvqScale klo = zgml::kvq_block_scale(mlo), khi = zgml::kvq_block_scale(mhi);
            if (live) {
                char* p = dq + (uint64_t)(c0 + col) * dh + i;
                float* ps = dsc + (uint64_t)(c0 + col) * bpc;
                *(uint32_t*)p = kvs_quantise4(rl, klo.inv), *(uint32_t*)(p + hd) = kvs_quantise4(rh, khi.inv);
                if (one_block) {
                    if (i == 0) ps[0] = klo.scale;
                } else if (i % 32 == 0) {
                    ps[i / 32] = klo.scale, ps[(hd + i) / 32] = khi.scale;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kKvsBlock) kv_shift_kernel(const KvShiftLane* __restrict__ lanes, const float* __restrict__ cs, uint32_t dh, uint32_t keep,
                                                             uint32_t discard, uint32_t n_move) {
    const KvShiftLane L = lanes[blockIdx.x]; // (uniform over the workgroup: every thread takes the same path and the same rounds)
    const uint64_t to = (uint64_t)keep * dh, by = (uint64_t)discard * dh, run = (uint64_t)n_move * dh;
    switch (L.kind) {
        case KVS_F32_COPY: kvs_move_left(L.data + to * 4, L.data + (to + by) * 4, run * 4); break;
        case KVS_F32_ROTATE:
            if (((uintptr_t)L.data & 15) == 0 && dh % 8 == 0)
                kvs_rotate_f32<4>((float*)L.data, cs, dh, keep, discard, n_move);
            else
                kvs_rotate_f32<1>((float*)L.data, cs, dh, keep, discard, n_move);
            break;
        case KVS_I8_COPY:
            kvs_move_left(L.data + to, L.data + to + by, run);
            kvs_move_left((char*)(L.scales + to / 32), (const char*)(L.scales + (to + by) / 32), run / 32 * 4);
            break;
        default: kvs_rotate_i8(L.data, L.scales, cs, dh, keep, discard, n_move); break;
    }
}

} // namespace
} // namespace zgml_rt

extern "C" {

void zgml_hip_kv_shift_rounds(uint32_t* rotate_values, uint32_t* copy_bytes) {
    if (rotate_values) *rotate_values = zgml::kKvsRotateRound;
    if (copy_bytes) *copy_bytes = zgml::kKvsCopyRound;
}

int zgml_hip_kv_shift(zgml_hip_ctx* ctx, zgml_hip_program* program, const zgml_kv_lane* lanes, const uint8_t* rotate, uint64_t n_lanes, uint32_t keep,
                      uint32_t discard, uint32_t n_filled, const float* cos_row, const float* sin_row) {
    if (!ctx || !program) return -1;
    if (!n_lanes || !discard) return 0;
    auto refuse = [&](const std::string& why) {
        ctx->fail("kv_shift: " + why);
        return -1;
    };
    if ((uint64_t)keep + discard > n_filled) return refuse("keep + discard exceeds n_filled");
    if ((uint64_t)keep + discard == n_filled) return 0; // (every column in use is kept or dropped: nothing moves)
    if (!lanes || !rotate) return refuse("no lane records");
    if (!cos_row || !sin_row) return refuse("no cos / sin row");
    if (n_lanes > 0x7FFFFFFFull) return refuse("more lanes than one launch carries");
    struct Extent {
        uintptr_t lo, hi;
    };
    std::vector<KvShiftLane> recs(n_lanes);
    std::vector<Extent> extents(n_lanes);
    const uint32_t dh = lanes[0].d_head;
    for (uint64_t i = 0; i < n_lanes; i++) {
        const zgml_kv_lane& l = lanes[i];
        auto refuse_lane = [&](const char* why) { return refuse("lane " + std::to_string(i) + ": " + why); };
        const char* why = nullptr;
        char* data;
        float* scales;
        if (!zgml_rt::kv_lane_base(program, l, n_filled, &why, &data, &scales)) return refuse_lane(why);
        if (l.d_head % 2) return refuse_lane("d_head is odd (RoPE turns pairs)");
        if (l.d_head != dh) return refuse_lane("d_head differs from lane 0's (one call, one d_head)");
        if (dh > 2048) return refuse_lane("d_head beyond 2048 (a round of the kernel carries whole columns)");
        if (l.block_size && rotate[i] && dh != 32 && dh % 64) return refuse_lane("an int8 K lane needs d_head 32 or d_head % 64 == 0 (whole blocks on either side of a pair)");
        recs[i] = KvShiftLane{data, scales, (l.block_size ? 2u : 0u) | (rotate[i] ? 1u : 0u), 0};
        const uint64_t vals = (uint64_t)l.n_cols * dh;
        extents[i] = {(uintptr_t)data, (uintptr_t)data + (l.block_size ? vals + vals / 32 * 4 : vals * 4)};
    }
    std::sort(extents.begin(), extents.end(), [](const Extent& a, const Extent& b) { return a.lo < b.lo; });
    for (uint64_t i = 1; i < n_lanes; i++)
        if (extents[i].lo < extents[i - 1].hi) return refuse("two lanes' extents meet (a lane listed twice, or lanes that overlap)");

    (void)hipSetDevice(ctx->device);
    // one block: the two rows (c, then s: d_head floats), then the records
    const uint64_t rows_bytes = ((uint64_t)dh * sizeof(float) + 15) & ~(uint64_t)15, bytes = rows_bytes + n_lanes * sizeof(KvShiftLane);
    zgml_rt::KvPoolBlock* blk = zgml_rt::kv_pool_block(ctx, bytes);
    if (!blk) return -1;
    for (uint64_t i = 0; i < n_lanes; i++) zgml_rt::unhoist_if_guarded(program, lanes[i].buf);
    memset(blk->host, 0, rows_bytes);
    memcpy(blk->host, cos_row, dh / 2 * sizeof(float));
    memcpy(blk->host + dh / 2 * sizeof(float), sin_row, dh / 2 * sizeof(float));
    memcpy(blk->host + rows_bytes, recs.data(), n_lanes * sizeof(KvShiftLane));
    if (!zgml_rt::kv_pool_upload(ctx, blk, bytes)) return -1;
    zgml_rt::kv_shift_kernel<<<(uint32_t)n_lanes, zgml_rt::kKvsBlock, 0, ctx->stream>>>((const KvShiftLane*)(blk->dev + rows_bytes), (const float*)blk->dev, dh, keep,
                                                                                       discard, n_filled - keep - discard);
    return CTX_CHECK(ctx, hipGetLastError()) ? 0 : -1;
}

} // extern "C"
