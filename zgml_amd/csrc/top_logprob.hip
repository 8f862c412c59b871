// top_logprob.hip — the top-n alternatives of a logits row with their log-probabilities (the `top_logprobs` word of zgml_sampling,
// zgml_hip_top_logprobs; runtime_resident.hip): the finish launch of logprob.hip in its top form, a kernel of its own beside the
// untouched logprob_finish_kernel. The rule is sample.h's ("THE ALTERNATIVES"); here is only how a workgroup evaluates its sliced
// form, and a device entry equals the header's over the same logits bits, to the bit. No workgroup waits for another, there are
// no atomics and no last-arriver stage (section 4.15).
//   [finish + top]  grid (1, rows), 1024 threads: the first 64 keys of each of the row's slice lists — what a select launch over
//              the RAW row left in its scratch, at most 32 x 64 keys, 16 KiB of LDS — are loaded with every second list reversed,
//              the state of a bitonic sort after its 64-runs: the merge stages from 128 up leave the row's largest keys in
//              front (why the heads are enough: sample.h). Wave 0 meanwhile computes M and the blocks' terms exactly as the
//              finish does, thread 0 the sum over ascending b. Then lane j < 64 writes alternative j and thread 0 the chosen
//              token's value, under the finish's guard: only the step that emitted a token writes.
//              (A pair per thread as 64-bit LDS words: for j >= 32 a half-wave reads 32 consecutive words, all 64 banks once; for
//              j < 32 it reads runs of j words with gaps of j, 64 words in all — two bank rows, a 2-way conflict, the usual price
//              of a bitonic stage; the stores, banked in 16-lane groups, likewise for j < 16. One workgroup per row and a few
//              microseconds in all: not worth a swizzle.)
#include "kernels.h"
#include "sample.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace zgml {
namespace {

constexpr uint32_t kTopBlock = 1024, kTopKeys = kSampleMaxSlices * kTopLogprobsMax;
static_assert(kTopKeys == 2 * kTopBlock, "a thread per pair of the widest merge");
static_assert(kTopLogprobsMax == 64 && kTopLogprobsMax <= kSampleMaxK, "a list's head is a wave wide and lies inside the list");

// one compare-exchange stage (k, j) of a bitonic sort that ends DESCENDING (sample.hip's, over at most one pair per thread)
__device__ __forceinline__ void top_bitonic_stage(uint64_t* s, uint32_t pairs, uint32_t k, uint32_t j) {
    const uint32_t t = threadIdx.x;
    if (t < pairs) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
        const uint64_t a = s[i], b = s[x];
        if ((i & k) == 0 ? a < b : a > b) s[i] = b, s[x] = a;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kTopBlock) logprob_finish_top_kernel(const float* __restrict__ v, uint32_t n, uint32_t nb, const float* __restrict__ part,
                                                                       const uint64_t* __restrict__ lists, uint32_t slices, uint32_t P, TopLogprobTarget tt) {
    __shared__ uint64_t s[kTopKeys];
    __shared__ float term[kLogprobMaxBlocks];
    __shared__ float ms[2];
    const uint32_t row = blockIdx.y, lane = threadIdx.x;
    const LogprobTarget& t = tt.chosen;
    // which token, and where its value and its alternatives go (uniform over the workgroup): logprob_finish_kernel's forms
    uint32_t tok = 0, produced = 0;
    float* dst = nullptr;
    uint64_t entry = row;
    if (t.tokens) {
        tok = t.tokens[row], dst = t.out + row;
    } else if (t.token64) {
        tok = (uint32_t)t.token64[0], dst = t.out, entry = 0;
    } else if (t.picks) {
        tok = t.picks[row], dst = t.out + row;
    } else if (t.state) {
        // the loops: only the step that emitted a token writes its entry (before the first barrier: the whole workgroup leaves)
        const uint32_t B = t.n_seqs;
        produced = B ? t.state[3 * B + row] : t.state[2];
        const uint32_t cap = B ? t.state[4 * B] : t.cap;
        if (produced <= t.written[row] || produced > cap) return;
        entry = (uint64_t)(B ? row : 0) * cap + (produced - 1);
        tok = (uint32_t)t.emitted[entry], dst = t.out + entry;
    }
    const uint64_t* heads = lists + (uint64_t)row * slices * kSampleMaxK;
    for (uint32_t i = lane; i < P; i += kTopBlock) { // P = the power of two >= slices * 64, <= kTopKeys
        const uint32_t l = i >> 6, off = i & 63;
        s[i] = l < slices ? heads[(uint64_t)l * kSampleMaxK + ((l & 1) ? 63 - off : off)] : 0;
    }
    if (lane < 64) { // wave 0: M and the blocks' terms, as logprob_finish_kernel
        const float* pr = part + 2 * (uint64_t)row * nb;
        float M = -INFINITY;
        for (uint32_t b = lane; b < nb; b += 64) M = pr[2 * b] > M ? pr[2 * b] : M;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(M, off, 64);
            M = o > M ? o : M;
        }
        for (uint32_t b = lane; b < nb; b += 64) term[b] = logprob_block_term(pr[2 * b], pr[2 * b + 1], M);
        if (lane == 0) ms[0] = M;
    }
    __syncthreads();
    if (lane == 0) {
        float S = 0.0f;
        for (uint32_t b = 0; b < nb; b++) S = S + term[b];
        ms[1] = S;
    }
    for (uint32_t k = 2 * kTopLogprobsMax; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) top_bitonic_stage(s, P / 2, k, j);
    __syncthreads(); // (P = 64: no stage, and ms[1] must be seen)
    // s[0, 64): the row's largest keys, descending
    if (lane >= kTopLogprobsMax) return;
    const float M = ms[0], S = ms[1];
    const uint32_t a = tt.params ? tt.params[tt.shared_params ? 0 : row].top_logprobs : tt.top_n;
    const uint32_t ae = top_logprobs_count(a, n);
    uint32_t alt = 0xFFFFFFFFu;
    float val = sample_bits_f32(kLogprobNaNBits);
    if (lane < ae) top_logprobs_entry(s[lane], M, S, &alt, &val);
    tt.top_tok[entry * kTopLogprobsMax + lane] = alt;
    tt.top_val[entry * kTopLogprobsMax + lane] = val;
    if (lane != 0) return;
    if (dst) *dst = tok < n ? logprob_of(v[(uint64_t)row * n + tok], M, S) : sample_bits_f32(kLogprobNaNBits); // (a token is an index of its row: the guard never acts)
    if (t.written) t.written[row] = produced;
}

} // namespace

void launch_logprob_finish_top(hipStream_t s, const float* v, uint64_t n, uint32_t rows, const float* part, const uint64_t* lists, const TopLogprobTarget& t) {
    if (!n || n > kLogprobMaxN || !rows) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    uint32_t P = kTopLogprobsMax;
    while (P < slices * kTopLogprobsMax) P <<= 1;
    logprob_finish_top_kernel<<<dim3(1, rows), kTopBlock, 0, s>>>(v, (uint32_t)n, logprob_blocks(n), part, lists, slices, P, t);
}

} // namespace zgml
