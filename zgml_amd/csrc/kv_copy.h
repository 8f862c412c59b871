// kv_copy.h — what one workgroup does with its chunk of a KV lane's run, stated once for the kernels that carry runs of KV columns
// between two places: kv_move_kernel (kv_move.hip: program to program) and kv_park_kernel (kv_park.hip: program to and from the
// staging block of a host blob). A record names the two sides of a lane's run; per record the run is copied (f32 -> f32;
// int8 -> int8: bytes and scales) or quantised (f32 -> int8) exactly as kvq_store does (kvq.h states the rule).
//
// Shape: the moved columns of a lane are ONE contiguous run of n * d_head values on either side, and the scales of an int8 lane a
// second run of n * d_head / 32 floats. The grid is (lane, chunk): a workgroup takes `chunk` values of its lane's run — 16-byte
// loads and stores where both addresses allow, dwords otherwise. In the quantising form a lane of a wave takes 4 dims, so 8
// adjacent lanes hold a block of 32 and a wave 8 blocks; the block maximum is a shuffle-xor reduction within those 8 lanes (a
// maximum has no rounding: any order gives kvq_store_kernel's wave_max). No workgroup reads what another writes: there is no
// cross-workgroup ordering, hand-off or loop over work items; the host refuses a call whose written ranges meet another written
// range or a range the call reads.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "kvq.h"

namespace zgml_rt {

enum KvMoveMode : uint32_t { KVM_F32 = 0, KVM_I8 = 1, KVM_QUANT = 2 };
struct KvMoveLane {
    const void* src;         // first moved value of the source (f32: floats; int8: bytes)
    void* dst;               // ... of the destination
    const float* src_scales; // int8 source: scale of the first moved block
    float* dst_scales;       // int8 destination
    uint64_t elems;          // n * d_head values
    uint32_t mode, _pad;
};

constexpr int kKvmBlock = 256;
constexpr uint32_t kKvmChunk = 8192; // values per workgroup: 32 KB of f32 — 8 16-byte loads per lane; a multiple of 4 * kKvmBlock

// values per workgroup for runs of up to max_elems values: kKvmChunk, doubled until the chunks of the longest run fit grid.y;
// 0: more values per lane than one launch carries (a chunk's byte count stays a 32-bit number)
inline uint32_t kvm_chunk_for(uint64_t max_elems) {
    uint32_t chunk = kKvmChunk;
    while ((max_elems + chunk - 1) / chunk > 65535 && chunk <= (1u << 29)) chunk *= 2;
    return chunk > (1u << 29) ? 0 : chunk;
}

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

// f32 -> int8: `cnt` floats at src -> cnt bytes at dst and cnt / 32 scales at sc. 4 dims per lane, a block of 32 dims on 8 adjacent
// lanes; cnt is a multiple of 32, so a group of 8 lanes is live or idle as a whole and the loop's trip count is the same for every
// lane of the workgroup
template <bool NT>
__device__ __forceinline__ void kvm_quantise(uint32_t* dst, float* sc, const float* src, uint32_t cnt) {
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
            const zgml::KvqScale s = zgml::kvq_block_scale(mx);
            const uint32_t w = (uint32_t)(uint8_t)zgml::kvq_quantise(v[u].x, s.inv) | (uint32_t)(uint8_t)zgml::kvq_quantise(v[u].y, s.inv) << 8 |
                               (uint32_t)(uint8_t)zgml::kvq_quantise(v[u].z, s.inv) << 16 | (uint32_t)(uint8_t)zgml::kvq_quantise(v[u].w, s.inv) << 24;
            if (e < cnt) {
                dst[e / 4] = w;
                if ((threadIdx.x & 7) == 0) sc[e / 32] = s.scale;
            }
        }
    }
}

// the workgroup's chunk of its lane's run: values [blockIdx.y * chunk, ... + chunk) of record blockIdx.x
template <bool NT>
__device__ __forceinline__ void kvm_lane_chunk(const KvMoveLane* __restrict__ lanes, uint32_t chunk) {
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
    kvm_quantise<NT>((uint32_t*)((int8_t*)L.dst + lo), L.dst_scales + lo / 32, (const float*)L.src + lo, cnt);
}

} // namespace zgml_rt
