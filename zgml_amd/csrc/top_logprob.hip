// top_logprob.hip — the top-n alternatives of a logits row with their log-probabilities (the `top_logprobs` word of zgml_sampling,
// zgml_hip_top_logprobs; runtime_resident.hip): the finish launch of logprob.hip in its top form — the same target resolution,
// M, terms and sum (tail_device.h's bodies, called by both kernels), with the merge of the lists' heads around them. The rule is
// sample.h's ("THE ALTERNATIVES"); here is only how a workgroup evaluates its sliced form, and a device entry equals the header's
// over the same logits bits, to the bit. No workgroup waits for another, there are no atomics and no last-arriver stage (DESIGN
// section 0.2 item 5; section 4.15).
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
#include "tail_device.h"

namespace zgml {
namespace {

constexpr uint32_t kTopBlock = 1024, kTopKeys = kSampleMaxSlices * kTopLogprobsMax;
static_assert(kTopKeys == 2 * kTopBlock, "a thread per pair of the widest merge");
static_assert(kTopLogprobsMax == 64 && kTopLogprobsMax <= kSampleMaxK, "a list's head is a wave wide and lies inside the list");

__global__ void __launch_bounds__(kTopBlock) logprob_finish_top_kernel(const float* __restrict__ v, uint32_t n, uint32_t nb, const float* __restrict__ part,
                                                                       const uint64_t* __restrict__ lists, uint32_t slices, uint32_t P, TopLogprobTarget tt) {
    __shared__ uint64_t s[kTopKeys];
    __shared__ float term[kLogprobMaxBlocks];
    __shared__ float ms[2];
    const uint32_t row = blockIdx.y, lane = threadIdx.x;
    __builtin_assume(P <= kTopKeys); // (a bitonic stage is then one pair per thread at the most, no loop)
    // which token, and where its value and its alternatives go (uniform over the workgroup; before the first barrier: the
    // whole workgroup leaves a step that emitted nothing)
    LogprobSlot slot;
    if (!logprob_resolve(tt.chosen, row, slot)) return;
    const uint64_t* heads = lists + (uint64_t)row * slices * kSampleMaxK;
    for (uint32_t i = lane; i < P; i += kTopBlock) { // P = the power of two >= slices * 64, <= kTopKeys
        const uint32_t l = i >> 6, off = i & 63;
        s[i] = l < slices ? heads[(uint64_t)l * kSampleMaxK + ((l & 1) ? 63 - off : off)] : 0;
    }
    if (lane < 64) { // wave 0: M and the blocks' terms, as logprob_finish_kernel
        const float M = logprob_row_terms(part + 2 * (uint64_t)row * nb, nb, lane, term);
        if (lane == 0) ms[0] = M;
    }
    __syncthreads();
    if (lane == 0) ms[1] = logprob_row_sum(term, nb);
    for (uint32_t k = 2 * kTopLogprobsMax; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kTopBlock>(s, P / 2, k, j);
    __syncthreads(); // (P = 64: no stage, and ms[1] must be seen)
    // s[0, 64): the row's largest keys, descending
    if (lane >= kTopLogprobsMax) return;
    const float M = ms[0], S = ms[1];
    const uint32_t a = tt.params ? tt.params[tt.shared_params ? 0 : row].top_logprobs : tt.top_n;
    const uint32_t ae = top_logprobs_count(a, n);
    uint32_t alt = 0xFFFFFFFFu;
    float val = sample_bits_f32(kLogprobNaNBits);
    if (lane < ae) top_logprobs_entry(s[lane], M, S, &alt, &val);
    tt.top_tok[slot.entry * kTopLogprobsMax + lane] = alt;
    tt.top_val[slot.entry * kTopLogprobsMax + lane] = val;
    if (lane == 0) logprob_store_chosen(tt.chosen, slot, row, v + (uint64_t)row * n, n, M, S);
}

} // namespace

void launch_logprob_finish_top(hipStream_t s, const float* v, uint64_t n, uint32_t rows, const float* part, const uint64_t* lists, const TopLogprobTarget& t) {
    if (!n || n > kLogprobMaxN || !rows) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    logprob_finish_top_kernel<<<dim3(1, rows), kTopBlock, 0, s>>>(v, (uint32_t)n, logprob_blocks(n), part, lists, slices, sample_merge_keys(slices, kTopLogprobsMax), t);
}

} // namespace zgml
