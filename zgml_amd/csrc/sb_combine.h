// sb_combine.h — the K-split fan-in of the super-block mat-vecs (sb_kernels.hip): every part of one super-block column stores
// its partial outputs, counts itself on an integer word in the scratch head, and the LAST part to arrive adds the partials in
// PART order (not arrival order; no float atomics), so two launches give the same bytes. The word is re-armed for the next launch.
#pragma once
#include "qmv_common.h"

namespace zgml {
namespace {

using gf32 = __attribute__((address_space(1))) float;
using gu32 = __attribute__((address_space(1))) unsigned int;

constexpr uint32_t kSbCombineBatch = 8; // partial sums the combining workgroup loads before it adds them

// Called by every thread of the workgroup. `live` threads hold the partial `y` of column `n`; `cnt` is the column block's word,
// `flag` a word of LDS. Returns false on every part but the last to arrive; there `y` becomes the sum over the parts.
__device__ __forceinline__ bool sb_combine(float& y, bool live, float* partial, uint32_t* cnt, uint32_t part, uint32_t parts, uint32_t N, uint32_t n, uint32_t* flag) {
    if (live) __hip_atomic_store((gf32*)(partial + (uint64_t)part * N + n), y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every storing wave drains before the count
    __syncthreads();
    if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add((gu32*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != parts - 1) return false; // not the last part of this column block
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // compiler only: the loads below stay below the count
    y = 0.f;
    if (live)
        for (uint32_t p0 = 0; p0 < parts; p0 += kSbCombineBatch) { // part order, not arrival order; a batch of loads in flight at once
            float pv[kSbCombineBatch];                             // (one dependent load per part cost 1.4 us each)
#pragma unroll
            for (uint32_t q = 0; q < kSbCombineBatch; q++) // (past the end: the last part again, dropped below)
                pv[q] = __hip_atomic_load((gf32*)(partial + (uint64_t)min(p0 + q, parts - 1) * N + n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (uint32_t q = 0; q < kSbCombineBatch; q++) y += p0 + q < parts ? pv[q] : 0.f;
        }
    if (threadIdx.x == 0) __hip_atomic_store((gu32*)cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-arm
    return true;
}

} // namespace
} // namespace zgml
