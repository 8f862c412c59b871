// greedy_tail.hip — the greedy token tail of the device-resident loops (runtime_resident.hip) and the stand-alone argmax op: the
// prep launches that produce a step's patches on the device (single, batched, batched verify step), and the argmax family — first index of the maximum — in its three
// shapes, all written over tail_device.h's bodies (a thread's scan, the block reductions, the advances):
//   launch_argmax               [stage 1: a pair per workgroup] [stage 2: the pairs' fold + the single loop's advance and the
//                               token's embedding row]; stage 1 may carry the position part of the next step's prep
//   launch_argmax_fold          its stage 2 alone (the pairs came from the streaming LM head: kernels_generic.hip)
//   launch_argmax_draft         the two stages behind a draft program's execution inside a verify step: stage 2 ends with the
//                               draft advance (the draft's next token and position, the target's next candidate)
//   launch_argmax_batch_draft   ... behind a BATCHED draft program's execution: B rows, sequence b's draft advance
//   launch_argmax_draft_constrained  ... under the target's constraint: stage 1 masked by the walk's state, the constrained draft advance
//   launch_argmax_batch         the same two stages over B rows (blockIdx.y = sequence), the batched loop's advance;
//   launch_argmax_rows_stage1   its stage 1 alone (a greedy verify step: spec_accept_kernel folds the pairs)
// Every workgroup has 256 threads and the same two LDS arrays; a row takes n / 1024 + 1 workgroups, at most 256.
#include "kernels.h"
#include "tail_device.h"

namespace zgml {

namespace {

constexpr int kBlock = kArgBlock, kArgBlocks = 256;

// one element of the flat prep index space (kernels.h: ResidentPrepArgs) at position `pos` with the chunk's tokens: the token
// part, then the position part (tail_device.h)
__device__ __forceinline__ void resident_prep_element(const ResidentPrepArgs& a, uint32_t i, uint32_t pos) {
    if (i < a.T * a.d)
        resident_prep_token(a, i);
    else
        resident_prep_position(a, i - a.T * a.d, pos);
}
__global__ void __launch_bounds__(256) resident_prep_kernel(ResidentPrepArgs a) {
    resident_prep_element(a, blockIdx.x * 256 + threadIdx.x, a.state[1]);
}

// the batched forms (kernels.h: ResidentBatchPrepArgs, ResidentBatchSpecPrepArgs), stated once: `cols` columns, Ts of them per
// sequence — column c is token j = c % Ts of sequence c / Ts, at that sequence's position + j; dynamic op i takes the position of
// its own sequence, a SeqKv word pos + Ts. tok_of(column) and pos_of(sequence) read the loop's device state
template <class A, class TokOf, class PosOf>
__device__ __forceinline__ void resident_batch_prep_element(const A& a, uint32_t i, uint32_t cols, uint32_t Ts, TokOf tok_of, PosOf pos_of) {
    if (i < cols * a.d) {
        const uint32_t j = i / a.d, e = i - j * a.d;
        a.tok_in[i] = a.embed[(uint64_t)tok_of(j) * a.d + e];
        return;
    }
    i -= cols * a.d;
    if (i < cols * a.max_seq) {
        const uint32_t j = i / a.max_seq, sidx = i - j * a.max_seq;
        a.mask[i] = sidx <= pos_of(j / Ts) + j % Ts ? 0.0f : -INFINITY;
        return;
    }
    i -= cols * a.max_seq;
    if (i < a.n_rope * cols * 2 * a.dh) {
        const uint32_t l = i / (cols * 2 * a.dh), rem = i - l * (cols * 2 * a.dh), j = rem / (2 * a.dh), e = rem - j * 2 * a.dh;
        const uint64_t at = pos_of(j / Ts) + j % Ts;
        a.rope_bufs[l][rem] = e < a.dh ? a.cos[at * a.dh + e] : a.sin[at * a.dh + e - a.dh];
        return;
    }
    i -= a.n_rope * cols * 2 * a.dh;
    if (i < a.n_ops) {
        const uint32_t kind = a.dyn_kind[i];
        if (kind == 0) return;
        const uint32_t ps = pos_of(a.dyn_seq[i]);
        a.dyn[i] = kind == 1 ? a.dyn_base[i] + ps * a.dyn_stride[i] : ps + Ts;
    }
}
// one column per sequence: token and position from the batched loop's state
__global__ void __launch_bounds__(256) resident_batch_prep_kernel(ResidentBatchPrepArgs a) {
    const uint32_t* const tok = a.state;
    const uint32_t* const pos = a.state + a.B;
    resident_batch_prep_element(a, blockIdx.x * 256 + threadIdx.x, a.B, 1u, [&](uint32_t j) { return tok[j]; }, [&](uint32_t b) { return pos[b]; });
}
// T columns per sequence (a batched verify step): the candidates, from the run position the draft launch chose for the sequence
__global__ void __launch_bounds__(256) resident_batch_spec_prep_kernel(ResidentBatchSpecPrepArgs a) {
    resident_batch_prep_element(a, blockIdx.x * 256 + threadIdx.x, a.B * a.T, a.T, [&](uint32_t j) { return a.cand[j]; },
                                [&](uint32_t b) { return a.words[b * kSpecWords + kSpecRunPos]; });
}

// stage 1 of row `row` (row stride n), shared by `nblk` workgroups: this workgroup's pair to slot row * nblk + blockIdx.x
__device__ __forceinline__ void argmax_stage1_body(float* sv, int64_t* si, uint32_t row, const float* __restrict__ v, uint64_t n, uint32_t nblk, float* out_val, int64_t* out_idx) {
    float bv;
    int64_t bi;
    arg_scan(v + (uint64_t)row * n, n, nblk, bv, bi);
    arg_block_reduce<false>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        out_val[row * nblk + blockIdx.x] = sv[0];
        out_idx[row * nblk + blockIdx.x] = si[0];
    }
}
// stage 2 of row `row`: the fold of its nblk pairs, some of them empty; the token in every thread (-1: no pair at all).
// kWide (the pairs of the streaming LM head, at most kArgPairs of them): every thread reads its kWidePairs pairs in ONE memory
// round trip — clamped loads, a dead one made empty by a select — not one dependent trip per 256 pairs
constexpr int kWidePairs = (int)kArgPairs / kBlock;
template <bool kWide = false>
__device__ __forceinline__ int64_t argmax_stage2_body(float* sv, int64_t* si, uint32_t row, const float* vals, const int64_t* idxs, int nblk) {
    vals += (uint64_t)row * nblk, idxs += (uint64_t)row * nblk;
    float bv = -INFINITY;
    int64_t bi = INT64_MAX;
    if (kWide) {
        float v[kWidePairs];
        int64_t ix[kWidePairs];
#pragma unroll
        for (int u = 0; u < kWidePairs; u++) {
            const int i = threadIdx.x + u * kBlock, at = i < nblk ? i : 0;
            v[u] = vals[at];
            ix[u] = i < nblk ? idxs[at] : INT64_MAX;
        }
#pragma unroll
        for (int u = 0; u < kWidePairs; u++) arg_fold(bv, bi, v[u], ix[u]);
    } else {
        for (int i = threadIdx.x; i < nblk; i += kBlock) arg_fold(bv, bi, vals[i], idxs[i]);
    }
    arg_block_reduce<true>(sv, si, bv, bi);
    return si[0] == INT64_MAX ? -1 : si[0];
}

__global__ void __launch_bounds__(kBlock) argmax_stage1(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    argmax_stage1_body(sv, si, 0, v, n, gridDim.x, out_val, out_idx);
}

// ... with the position part of the next step's prep in the workgroups behind the row's `nblk` (the resident greedy loop over a
// head that is not the streaming dense form)
__global__ void __launch_bounds__(kBlock) argmax_stage1_ahead(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx, uint32_t nblk, ResidentAhead ahead) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    if (blockIdx.x >= nblk) {
        resident_prep_ahead(ahead, (blockIdx.x - nblk) * kBlock + threadIdx.x);
        return;
    }
    argmax_stage1_body(sv, si, 0, v, n, nblk, out_val, out_idx);
}

// kWide: the fold launch behind the streaming head (launch_argmax_fold); the stand-alone op and the two-stage tail keep the plain walk
template <bool kWide>
__global__ void __launch_bounds__(kBlock) argmax_stage2(const float* vals, const int64_t* idxs, int nblk, int64_t* out, ArgmaxAdvance adv) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body<kWide>(sv, si, 0, vals, idxs, nblk);
    // the token part of the next step's prep: its embedding row, by all threads
    if (adv.embed && next >= 0)
        for (uint32_t e = threadIdx.x; e < adv.d; e += kBlock) adv.tok_in[e] = adv.embed[(uint64_t)next * adv.d + e];
    if (threadIdx.x != 0) return;
    *out = next;
    if (adv.state) tail_advance_single(adv.state, adv.tokens, adv.cap, next); // the resident loop's advance step
}

// stage 2 behind one execution of a draft program inside a verify step: the fold, then the draft advance (tail_device.h). A row
// has n > 0 entries, so a pair exists and the index is one of the row's: the clamp is for the embedding gather's sake
__global__ void __launch_bounds__(kBlock) argmax_stage2_draft(const float* vals, const int64_t* idxs, int nblk, uint64_t n, DraftAdvance adv) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body(sv, si, 0, vals, idxs, nblk);
    if (threadIdx.x == 0) tail_advance_draft(adv, 0, (uint64_t)next < n ? (uint32_t)next : 0u);
}

// argmax_stage1 / argmax_stage2 over B rows of n values at once: blockIdx.y = row (sequence); same (value, index) ordering
__global__ void __launch_bounds__(kBlock) argmax_batch_stage1(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    argmax_stage1_body(sv, si, blockIdx.y, v, n, gridDim.x, out_val, out_idx);
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

// ... behind one execution of a batched draft program: workgroup blockIdx.y folds row b's pairs and advances sequence b's draft
// state. No gate on the steps-left word and no token table (argmax_batch_stage2 has both): an idling sequence's draft runs on,
// over columns nobody reads
__global__ void __launch_bounds__(kBlock) argmax_batch_stage2_draft(const float* vals, const int64_t* idxs, int nblk, uint64_t n, DraftAdvance adv) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body(sv, si, blockIdx.y, vals, idxs, nblk);
    if (threadIdx.x == 0) tail_advance_draft(adv, blockIdx.y, (uint64_t)next < n ? (uint32_t)next : 0u);
}

// ... behind one execution of a draft program under the target's constraint (kernels.h: DraftConstraint): workgroup (x, b) scans
// its share of row b over the tokens that the walk's state allows. The state word is read here, at run time. A dead state leaves
// in front of any barrier and any table read — next + s * n_classes is never formed with it —, its pair empty; the row
// next[s] is staged as sample.hip's select_body stages it (global loads: the pointers come from a device table). A sequence
// without an automaton scans the plain way.
// LDS: 3 KiB of pairs, at most 16 KiB of state row
__global__ void __launch_bounds__(kBlock) argmax_batch_stage1_masked(const float* __restrict__ v, uint64_t n, float* out_val, int64_t* out_idx, DraftConstraint dc) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    __shared__ uint16_t crow[kConstraintMaxClasses];
    const uint32_t b = blockIdx.y, nblk = gridDim.x;
    const SampleConstraintRow cr = dc.rows[b];
    if (!cr.con_active) { // (uniform)
        argmax_stage1_body(sv, si, b, v, n, nblk, out_val, out_idx);
        return;
    }
    const uint32_t s = dc.row_state[(uint64_t)b * dc.stride];
    if (s == kConstraintDead) { // (uniform) no draft: the advance does not look at the pairs, they are empty all the same
        if (threadIdx.x == 0) out_val[b * nblk + blockIdx.x] = -INFINITY, out_idx[b * nblk + blockIdx.x] = INT64_MAX;
        return;
    }
    using global_u16 = const __attribute__((address_space(1))) uint16_t;
    global_u16* const class_of = (global_u16*)cr.class_of;
    global_u16* const from = (global_u16*)cr.next + (uint64_t)s * cr.n_classes;
    for (uint32_t t = threadIdx.x; t < cr.n_classes; t += kBlock) crow[t] = from[t];
    __syncthreads(); // crow is whole before the scan reads it
    float bv;
    int64_t bi;
    arg_scan_masked(v + (uint64_t)b * n, n, nblk, crow, class_of, bv, bi);
    arg_block_reduce<true>(sv, si, bv, bi);
    if (threadIdx.x == 0) {
        out_val[b * nblk + blockIdx.x] = sv[0];
        out_idx[b * nblk + blockIdx.x] = si[0];
    }
}

// ... and its stage 2: the empty-aware fold, then the constrained draft advance (tail_device.h). An empty fold, or an index that
// is not one of the row's, is "no draft"
__global__ void __launch_bounds__(kBlock) argmax_batch_stage2_draft_constrained(const float* vals, const int64_t* idxs, int nblk, uint64_t n, DraftAdvance adv, DraftConstraint dc) {
    __shared__ float sv[kBlock];
    __shared__ int64_t si[kBlock];
    const int64_t next = argmax_stage2_body(sv, si, blockIdx.y, vals, idxs, nblk);
    if (threadIdx.x != 0) return;
    const uint32_t b = blockIdx.y;
    const SampleConstraintRow cr = dc.rows[b];
    if (!cr.con_active)
        tail_advance_draft(adv, b, (uint64_t)next < n ? (uint32_t)next : 0u);
    else
        tail_advance_draft_constrained(adv, dc, cr, b, (uint64_t)next < n ? next : -1);
}

} // namespace

void launch_resident_prep(hipStream_t s, const ResidentPrepArgs& a, uint32_t total) {
    if (total) resident_prep_kernel<<<(total + 255) / 256, 256, 0, s>>>(a);
}

void launch_resident_batch_prep(hipStream_t s, const ResidentBatchPrepArgs& a, uint32_t total) {
    if (total) resident_batch_prep_kernel<<<(total + 255) / 256, 256, 0, s>>>(a);
}

void launch_resident_batch_spec_prep(hipStream_t s, const ResidentBatchSpecPrepArgs& a, uint32_t total) {
    if (total) resident_batch_spec_prep_kernel<<<(total + 255) / 256, 256, 0, s>>>(a);
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

void launch_argmax(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, int64_t* out, const ArgmaxAdvance& adv,
                   const ResidentAhead* ahead) {
    const int nblk = argmax_batch_blocks(n);
    if (ahead && ahead->total)
        argmax_stage1_ahead<<<nblk + (ahead->total + kBlock - 1) / kBlock, kBlock, 0, s>>>(v, n, scratch_val, scratch_idx, (uint32_t)nblk, *ahead);
    else
        argmax_stage1<<<nblk, kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
    argmax_stage2<false><<<1, kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, out, adv);
}

void launch_argmax_draft(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, const DraftAdvance& adv) {
    const int nblk = argmax_batch_blocks(n);
    argmax_stage1<<<nblk, kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
    argmax_stage2_draft<<<1, kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, n, adv);
}

void launch_argmax_batch_draft(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, const DraftAdvance& adv) {
    const int nblk = argmax_batch_blocks(n);
    argmax_batch_stage1<<<dim3(nblk, adv.n_seqs), kBlock, 0, s>>>(v, n, scratch_val, scratch_idx);
    argmax_batch_stage2_draft<<<dim3(1, adv.n_seqs), kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, n, adv);
}

void launch_argmax_draft_constrained(hipStream_t s, const float* v, uint64_t n, float* scratch_val, int64_t* scratch_idx, const DraftAdvance& adv,
                                     const DraftConstraint& dc) {
    const int nblk = argmax_batch_blocks(n);
    argmax_batch_stage1_masked<<<dim3(nblk, adv.n_seqs), kBlock, 0, s>>>(v, n, scratch_val, scratch_idx, dc);
    argmax_batch_stage2_draft_constrained<<<dim3(1, adv.n_seqs), kBlock, 0, s>>>(scratch_val, scratch_idx, nblk, n, adv, dc);
}

void launch_argmax_fold(hipStream_t s, const float* scratch_val, const int64_t* scratch_idx, uint32_t nblk, int64_t* out, const ArgmaxAdvance& adv) {
    argmax_stage2<true><<<1, kBlock, 0, s>>>(scratch_val, scratch_idx, (int)nblk, out, adv); // (nblk <= kArgPairs: the head's workgroups)
}

} // namespace zgml
