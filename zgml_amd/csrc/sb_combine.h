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

// The protocol's three steps, stated once for the M = 1 form and the row form below.
// [arrive] after the caller's partial stores: every storing wave drains, the workgroup counts itself once on `cnt`; true on the
// last part to arrive
__device__ __forceinline__ bool sb_combine_arrive(uint32_t* cnt, uint32_t parts, uint32_t* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every storing wave drains before the count
    __syncthreads();
    if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add((gu32*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != parts - 1) return false; // not the last part of this column block
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // compiler only: the loads of the sums stay below the count
    return true;
}
// [sum] one output's partials, `stride` floats apart from `col` on, added in part order (not arrival order): THE additions of
// every super-block mat-vec output, one row or many
template <class Stride> // (uint32_t N at M = 1, uint64_t M * N for rows: the M = 1 kernels keep their 32-bit multiply)
__device__ __forceinline__ float sb_sum_parts(const float* col, Stride stride, uint32_t parts) {
    float y = 0.f;
    for (uint32_t p0 = 0; p0 < parts; p0 += kSbCombineBatch) { // a batch of loads in flight at once
        float pv[kSbCombineBatch];                             // (one dependent load per part cost 1.4 us each)
#pragma unroll
        for (uint32_t q = 0; q < kSbCombineBatch; q++) // (past the end: the last part again, dropped below)
            pv[q] = __hip_atomic_load((gf32*)(col + (uint64_t)min(p0 + q, parts - 1) * stride), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (uint32_t q = 0; q < kSbCombineBatch; q++) y += p0 + q < parts ? pv[q] : 0.f;
    }
    return y;
}
// [re-arm] the word is zero again for the next launch
__device__ __forceinline__ void sb_combine_rearm(uint32_t* cnt) {
    if (threadIdx.x == 0) __hip_atomic_store((gu32*)cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by every thread of the workgroup. `live` threads hold the partial `y` of column `n`; `cnt` is the column block's word,
// `flag` a word of LDS. Returns false on every part but the last to arrive; there `y` becomes the sum over the parts.
__device__ __forceinline__ bool sb_combine(float& y, bool live, float* partial, uint32_t* cnt, uint32_t part, uint32_t parts, uint32_t N, uint32_t n, uint32_t* flag) {
    if (live) __hip_atomic_store((gf32*)(partial + (uint64_t)part * N + n), y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!sb_combine_arrive(cnt, parts, flag)) return false;
    y = 0.f;
    if (live) y = sb_sum_parts(partial + n, N, parts);
    sb_combine_rearm(cnt);
    return true;
}

// The same fan-in for the R rows of a row group (the multi-row mat-vecs): still ONE count per workgroup on the group's own word,
// the partials [parts][M][N] (`partial`: row 0 of the group in part 0; `part_stride` = M * N), and the last part to arrive sums
// every row of the group with sb_sum_parts, so a row's bytes are those of its M = 1 launch. A thread holds column n of the rows rr
// with (rr & 1) == `odd` (512 threads: two per column); rows rr >= `rows` of the group are not live.
template <int R>
__device__ __forceinline__ bool sb_combine_rows(float (&y)[R], uint32_t odd, uint32_t rows, float* partial, uint64_t part_stride, uint32_t* cnt, uint32_t part,
                                                uint32_t parts, uint32_t N, uint32_t n, uint32_t* flag) {
#pragma unroll
    for (int rr = 0; rr < R; rr++)
        if ((rr & 1) == (int)odd && rr < (int)rows)
            __hip_atomic_store((gf32*)(partial + (uint64_t)part * part_stride + (uint64_t)rr * N + n), y[rr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!sb_combine_arrive(cnt, parts, flag)) return false;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
        if ((rr & 1) == (int)odd && rr < (int)rows) y[rr] = sb_sum_parts(partial + (uint64_t)rr * N + n, part_stride, parts);
    sb_combine_rearm(cnt);
    return true;
}

} // namespace
} // namespace zgml
