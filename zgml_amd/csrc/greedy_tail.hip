// greedy_tail.hip — the greedy token tail of the device-resident loops (runtime_resident.hip) and the stand-alone argmax op: the
// prep launches that produce a step's patches on the device, and the argmax family — first index of the maximum — in its three
// shapes, all written over tail_device.h's bodies (a thread's scan, the block reductions, the advances):
//   launch_argmax               [stage 1: a pair per workgroup] [stage 2: the pairs' fold + the single loop's advance]
//   launch_argmax_batch         the same two stages over B rows (blockIdx.y = sequence), the batched loop's advance;
//   launch_argmax_rows_stage1   its stage 1 alone (a greedy verify step: spec_accept_kernel folds the pairs)
//   launch_argmax_tail          both stages in ONE launch — the last workgroup to arrive does the second — with the advance and
//                               the next token's patches
// Every workgroup has 256 threads and the same two LDS arrays; a row takes n / 1024 + 1 workgroups, at most 256.
#include "kernels.h"
#include "tail_device.h"

namespace zgml {

namespace {

constexpr int kBlock = kArgBlock, kArgBlocks = 256;

// one element of the flat prep index space (kernels.h: ResidentPrepArgs) at position `pos` with the chunk's tokens `tokens`
__device__ __forceinline__ void resident_prep_element(const ResidentPrepArgs& a, uint32_t i, uint32_t pos, const uint32_t* tokens, uint32_t token0, bool use_token0) {
    if (i < a.T * a.d) {
        const uint32_t j = i / a.d, e = i - j * a.d;
        a.tok_in[i] = a.embed[(uint64_t)(use_token0 ? token0 : tokens[j]) * a.d + e];
        return;
    }
    i -= a.T * a.d;
    if (i < a.T * a.max_seq) {
        const uint32_t j = i / a.max_seq, sidx = i - j * a.max_seq;
        a.mask[i] = sidx <= pos + j ? 0.0f : -INFINITY;
        return;
    }
    i -= a.T * a.max_seq;
    if (i < a.n_rope * a.T * 2 * a.dh) {
        const uint32_t l = i / (a.T * 2 * a.dh), rem = i - l * (a.T * 2 * a.dh), j = rem / (2 * a.dh), e = rem - j * 2 * a.dh;
        a.rope_bufs[l][rem] = e < a.dh ? a.cos[(uint64_t)(pos + j) * a.dh + e] : a.sin[(uint64_t)(pos + j) * a.dh + e - a.dh];
        return;
    }
    i -= a.n_rope * a.T * 2 * a.dh;
    if (i < a.n_ops) {
        if (a.dyn_kind[i] == 1) a.dyn[i] = a.dyn_base[i] + pos * a.dyn_stride[i];
        if (a.dyn_kind[i] == 2) a.dyn[i] = pos + a.T;
    }
}
__global__ void __launch_bounds__(256) resident_prep_kernel(ResidentPrepArgs a) {
    resident_prep_element(a, blockIdx.x * 256 + threadIdx.x, a.state[1], a.tokens, 0, false);
}

// the batched form (kernels.h: ResidentBatchPrepArgs): column j / dynamic op i takes token and position of its own sequence
__global__ void __launch_bounds__(256) resident_batch_prep_kernel(ResidentBatchPrepArgs a) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t* const tok = a.state;
    const uint32_t* const pos = a.state + a.B;
    if (i < a.B * a.d) {
        const uint32_t j = i / a.d, e = i - j * a.d;
        a.tok_in[i] = a.embed[(uint64_t)tok[j] * a.d + e];
        return;
    }
    i -= a.B * a.d;
    if (i < a.B * a.max_seq) {
        const uint32_t j = i / a.max_seq, sidx = i - j * a.max_seq;
        a.mask[i] = sidx <= pos[j] ? 0.0f : -INFINITY;
        return;
    }
    i -= a.B * a.max_seq;
    if (i < a.n_rope * a.B * 2 * a.dh) {
        const uint32_t l = i / (a.B * 2 * a.dh), rem = i - l * (a.B * 2 * a.dh), j = rem / (2 * a.dh), e = rem - j * 2 * a.dh;
        a.rope_bufs[l][rem] = e < a.dh ? a.cos[(uint64_t)pos[j] * a.dh + e] : a.sin[(uint64_t)pos[j] * a.dh + e - a.dh];
        return;
    }
    i -= a.n_rope * a.B * 2 * a.dh;
    if (i < a.n_ops) {
        const uint32_t kind = a.dyn_kind[i];
        if (kind == 0) return;
        const uint32_t ps = pos[a.dyn_seq[i]];
        a.dyn[i] = kind == 1 ? a.dyn_base[i] + ps * a.dyn_stride[i] : ps + 1;
    }
}

// stage 1 of row `row` (row stride n): this workgroup's pair to slot row * gridDim.x + blockIdx.x
__device__ __forceinline__ void argmax_stage1_body(float* sv, int64_t* si, uint32_t row, const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx) {
    float bv;
    int64_t bi;
    arg_scan(v + (uint64_t)row * n, n, bv, bi);
    arg_block_reduce<false>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        out_val[row * gridDim.x + blockIdx.x] = sv[0];
        out_idx[row * gridDim.x + blockIdx.x] = si[0];
    }
}
// stage 2 of row `row`: the fold of its nblk pairs, some of them empty; the token in thread 0 (-1: no pair at all)
__device__ __forceinline__ int64_t argmax_stage2_body(float* sv, int64_t* si, uint32_t row, const float* vals, const int64_t* idxs, int nblk) {
    vals += (uint64_t)row * nblk, idxs += (uint64_t)row * nblk;
    float bv = -INFINITY;
    int64_t bi = INT64_MAX;
    for (int i = threadIdx.x; i < nblk; i += kBlock) arg_fold(bv, bi, vals[i], idxs[i]);
    arg_block_reduce<true>(sv, si, bv, bi);
    return si[0] == INT64_MAX ? -1 : si[0];
}

__global__ void __launch_bounds__(kBlock) argmax_stage1(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    argmax_stage1_body(sv, si, 0, v, n, out_val, out_idx);
}

__global__ void __launch_bounds__(kBlock) argmax_stage2(const float* vals, const int64_t* idxs, int nblk, int64_t* out, ArgmaxAdvance adv) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body(sv, si, 0, vals, idxs, nblk);
    if (threadIdx.x != 0) return;
    *out = next;
    if (adv.state) tail_advance_single(adv.state, adv.tokens, adv.cap, next); // the resident loop's advance step
}

// argmax_stage1 / argmax_stage2 over B rows of n values at once: blockIdx.y = row (sequence); same (value, index) ordering
__global__ void __launch_bounds__(kBlock) argmax_batch_stage1(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    argmax_stage1_body(sv, si, blockIdx.y, v, n, out_val, out_idx);
}

__global__ void __launch_bounds__(kBlock) argmax_batch_stage2(const float* vals, const int64_t* idxs, int nblk, uint32_t* state, int64_t* tokens) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body(sv, si, blockIdx.y, vals, idxs, nblk);
    if (threadIdx.x != 0) return;
    // the advance step of sequence b: only while it has steps left (else it repeats the same token at the same position)
    const uint32_t b = blockIdx.y, B = gridDim.y;
    if (state[2 * B + b] > 0) tail_advance_batched(state, tokens, B, b, next);
}

// argmax_stage1 + (last arriver) argmax_stage2 + advance + the next token's prep (kernels.h: launch_argmax_tail)
__global__ void __launch_bounds__(kBlock) argmax_tail_kernel(const float* __restrict__ v, uint64_t n, float* vals, int64_t* idxs, uint32_t* cnt, int64_t* out,
                                                             ArgmaxAdvance adv, ResidentPrepArgs prep, uint32_t prep_total, uint32_t has_prep) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    __shared__ uint32_t bc[2];
    using gu32 = __attribute__((address_space(1))) uint32_t;
    using gu64 = __attribute__((address_space(1))) unsigned long long;
    // The next token's patches that depend on its POSITION only — mask column, RoPE rows, dynamic words: everything but the
    // embedding row — are written here by ALL workgroups (the position is known: state[1] + 1, read before this workgroup's
    // arrival is counted, i.e. before the last arriver advances it; the plan that read the current token's patches has finished).
    // Round 5's first form left the whole prep to the last arriver: one workgroup walking 8-16 K elements alone was a longer chain
    // than the two launches it replaced. What is left for the last arriver is the embedding row of the token it has just found.
    const uint32_t prep_tok = has_prep ? prep.T * prep.d : 0;
    if (has_prep && adv.state) {
        const uint32_t pos_next = adv.state[1] + 1;
        if (pos_next < prep.max_seq)
            for (uint32_t i = prep_tok + blockIdx.x * kBlock + threadIdx.x; i < prep_total; i += gridDim.x * kBlock) resident_prep_element(prep, i, pos_next, nullptr, 0, true);
    }
    float bv;
    int64_t bi;
    arg_scan(v, n, bv, bi); // ---- stage 1 (as argmax_stage1)
    arg_block_reduce<false>(sv, si, bv, bi);
    if (threadIdx.x == 0) { // publish this workgroup's pair write-through, drain, count (the guide's fan-in form: sc1 payload + vmcnt(0) + agent atomic)
        __hip_atomic_store((gu32*)vals + blockIdx.x, __float_as_uint(sv[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((gu64*)idxs + blockIdx.x, (unsigned long long)si[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bc[0] = __hip_atomic_fetch_add((gu32*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!bc[0]) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // compiler only: the agent-scope loads below stay below the count
    bv = -INFINITY, bi = INT64_MAX; // ---- stage 2 (as argmax_stage2), every pair read with agent-scope loads
    for (uint32_t i = threadIdx.x; i < gridDim.x; i += kBlock) {
        const int64_t ix = (int64_t)__hip_atomic_load((gu64*)idxs + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float vx = __uint_as_float(__hip_atomic_load((gu32*)vals + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        arg_fold(bv, bi, vx, ix);
    }
    arg_block_reduce<true>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        const int64_t next = si[0] == INT64_MAX ? -1 : si[0];
        *out = next;
        const uint32_t pos_next = adv.state ? tail_advance_single(adv.state, adv.tokens, adv.cap, next) : 0; // the resident loop's advance step
        __hip_atomic_store((gu32*)cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-arm
        bc[0] = (uint32_t)next, bc[1] = pos_next;
    }
    __syncthreads();
    if (!has_prep) return;
    const uint32_t token = bc[0], pos = bc[1];
    if (pos >= prep.max_seq || token >= 0x7FFFFFFFu) return; // (the context is full, or no finite logit: nothing to prepare)
    for (uint32_t i = threadIdx.x; i < prep_tok; i += kBlock) resident_prep_element(prep, i, pos, nullptr, token, true); // the embedding row(s)
}
} // namespace

void launch_resident_prep(hipStream_t s, const ResidentPrepArgs& a, uint32_t total) {
    if (total) resident_prep_kernel<<<(total + 255) / 256, 256, 0, s>>>(a);
}

void launch_resident_batch_prep(hipStream_t s, const ResidentBatchPrepArgs& a, uint32_t total) {
    if (total) resident_batch_prep_kernel<<<(total + 255) / 256, 256, 0, s>>>(a);
}

int argmax_batch_blocks(uint64_t n) {
    const int nblk = (int)(n / (kBlock * 4) + 1);
    return nblk > kArgBlocks ? kArgBlocks : nblk;
}
void launch_argmax_batch(hipStream_t s, const float* v, uint64_t n, uint32_t B, float* scratch_val, int64_t* scratch_idx, uint32_t* state, int64_t* tokens) {
    const int nblk = argmax_batch_blocks(n);
    argmax_batch_stage1<<<dim3(nblk, B), kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
    argmax_batch_stage2<<<dim3(1, B), kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, state, tokens);
}

void launch_argmax_rows_stage1(hipStream_t s, const float* v, uint64_t n, uint32_t rows, float* scratch_val, int64_t* scratch_idx) {
    argmax_batch_stage1<<<dim3(argmax_batch_blocks(n), rows), kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
}

void launch_argmax_tail(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, uint32_t* cnt, int64_t* out,
                        const ArgmaxAdvance& adv, const ResidentPrepArgs* prep, uint32_t prep_total) {
    argmax_tail_kernel<<<argmax_batch_blocks(n), kBlock, 0, s>>>(v, n, scratch_val, scratch_idx, cnt, out, adv, prep ? *prep : ResidentPrepArgs{}, prep_total, prep ? 1u : 0u);
}

void launch_argmax(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, int64_t* out, const ArgmaxAdvance& adv) {
    const int nblk = argmax_batch_blocks(n);
    argmax_stage1<<<nblk, kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
    argmax_stage2<<<1, kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, out, adv);
}

} // namespace zgml
