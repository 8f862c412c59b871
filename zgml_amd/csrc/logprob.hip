// logprob.hip — log softmax(row)[token] over whole rows of logits (zgml_hip_logprobs, the `logprobs` field of zgml_sampling;
// runtime_resident.hip): two launches whatever the number of rows. The rule — the blocks, the order of every sum, sample_exp and
// sample_log — is sample.h's ("THE LOG-PROBABILITY"); here is only how workgroups evaluate it, and a device value equals the
// header's over the same logits bits, to the bit. No workgroup waits for another, there are no atomics and no last-arriver
// stage (section 4.14).
//   [partial]  grid (blocks, rows), 256 threads: a workgroup reads its block of 4096 logits once — thread l its k-th 16 bytes at
//              element 1024 k + 4 l, k = 0..3 —, folds the block's maximum (wave shuffles, then four words of LDS), adds the
//              exponentials into its four accumulators, ascending k, and folds the 256 thread sums over the pairs (l, l + h):
//              h = 128, 64 in LDS, h = 32 .. 1 as shuffles of wave 0. It stores (m_b, s_b).
//   [finish]   grid (1, rows), one wave: the row's M (order-free), the blocks' terms s_b * sample_exp(m_b - M) with a lane each,
//              then lane 0 alone: the sum over ascending b, the token's logit, one f32 store. Which token, and where the value
//              goes, is LogprobTarget's (kernels.h). The kernel is four calls of tail_device.h's finish bodies, which the top
//              form of this launch (top_logprob.hip) calls too.
#include "kernels.h"
#include "tail_device.h"

namespace zgml {
namespace {

constexpr uint32_t kLpWaves = kLogprobThreads / 64;

__global__ void __launch_bounds__(kLogprobThreads) logprob_partial_kernel(const float* __restrict__ v, uint32_t n, float* __restrict__ part) {
    __shared__ float fold[kLogprobThreads];
    __shared__ float wmax[kLpWaves];
    const uint32_t l = threadIdx.x, b = blockIdx.x;
    const uint32_t start = b * kLogprobBlock; // (< n: the grid has logprob_blocks(n) columns)
    const uint32_t len = n - start < kLogprobBlock ? n - start : kLogprobBlock;
    const float* blk = v + (uint64_t)blockIdx.y * n + start;
    // a row at an odd offset of its buffer (zgml_hip_logprobs) is not 16-byte aligned: element loads then. Uniform over the workgroup
    const bool aligned = ((uintptr_t)blk & 15) == 0;
    float x[4][4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t i = k * (4 * kLogprobThreads) + 4 * l;
        if (aligned && i + 4 <= len) {
            const float4 q = *reinterpret_cast<const float4*>(blk + i);
            x[k][0] = q.x, x[k][1] = q.y, x[k][2] = q.z, x[k][3] = q.w;
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) x[k][c] = i + c < len ? blk[i + c] : -INFINITY; // (behind the end: a term of +0)
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) {
            x[k][c] = logprob_value(x[k][c]);
            m = x[k][c] > m ? x[k][c] : m;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((l & 63) == 0) wmax[l >> 6] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (uint32_t w = 1; w < kLpWaves; w++) m = wmax[w] > m ? wmax[w] : m;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) acc[c] = acc[c] + logprob_term(x[k][c], m);
    fold[l] = logprob_thread_sum(acc);
    __syncthreads();
    if (l < 128) fold[l] = fold[l] + fold[l + 128];
    __syncthreads();
    if (l >= 64) return;
    float p = fold[l] + fold[l + 64];
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) p = p + __shfl_down(p, h, 64); // (lane l < h: p[l] + p[l + h]; the lanes behind hold nothing of use)
    if (l == 0) {
        float* out = part + 2 * ((uint64_t)blockIdx.y * gridDim.x + b);
        out[0] = m, out[1] = p;
    }
}

__global__ void __launch_bounds__(64) logprob_finish_kernel(const float* __restrict__ v, uint32_t n, uint32_t nb, const float* __restrict__ part, LogprobTarget t) {
    __shared__ float term[kLogprobMaxBlocks];
    const uint32_t row = blockIdx.y, lane = threadIdx.x;
    LogprobSlot slot; // which token, and where its value goes (uniform over the wave)
    if (!logprob_resolve(t, row, slot)) return;
    const float M = logprob_row_terms(part + 2 * (uint64_t)row * nb, nb, lane, term);
    __syncthreads();
    if (lane != 0) return;
    logprob_store_chosen(t, slot, row, v + (uint64_t)row * n, n, M, logprob_row_sum(term, nb));
}

} // namespace

void launch_logprob(hipStream_t s, const float* v, uint64_t n, uint32_t rows, float* part) {
    if (!n || n > kLogprobMaxN || !rows) return; // (the callers refuse these)
    logprob_partial_kernel<<<dim3(logprob_blocks(n), rows), kLogprobThreads, 0, s>>>(v, (uint32_t)n, part);
}

void launch_logprob_finish(hipStream_t s, const float* v, uint64_t n, uint32_t rows, const float* part, const LogprobTarget& t) {
    if (!n || n > kLogprobMaxN || !rows) return;
    logprob_finish_kernel<<<dim3(1, rows), 64, 0, s>>>(v, (uint32_t)n, logprob_blocks(n), part, t);
}

} // namespace zgml
