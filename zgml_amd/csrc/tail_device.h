// tail_device.h — the device bodies the token tail's kernels share (greedy_tail.hip, sample.hip, logprob.hip, top_logprob.hip,
// spec_decode.hip, and kernels_generic.hip's streaming LM head), each stated once. Included by .hip files only: threadIdx,
// barriers and wave shuffles live here, never in sample.h / sample_params.h, the rule headers the CPU tests compile.
//   the single-sequence prep     its token part and its position part, and the position part a token ahead
//   the bitonic stage            sample.hip's select and merge sorts, top_logprob.hip's merge of the lists' heads
//   the argmax pieces            first maximum wins: a thread's scan, the block reductions, the empty-aware fold, its wave form
//   the advances                 of the single loop's and of the batched loop's device state, behind a greedy or a sampled pick,
//                                and of a draft program's state words behind one of its executions inside a verify step, plain
//                                and under the target's constraint; the masked form of a thread's scan goes with the latter
//   the log-probability finish   which token and where its value goes; M, the blocks' terms and their sum over ascending b
#pragma once
#include "kernels.h"
#include "sample.h"
#include "spec.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace zgml {

// one compare-exchange stage (k, j) of a bitonic sort that ends DESCENDING, over `pairs` = keys / 2 pairs; ends with a barrier
template <uint32_t kThreads>
__device__ __forceinline__ void bitonic_stage(uint64_t* s, uint32_t pairs, uint32_t k, uint32_t j) {
    for (uint32_t t = threadIdx.x; t < pairs; t += kThreads) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
        const uint64_t a = s[i], b = s[x];
        if ((i & k) == 0 ? a < b : a > b) s[i] = b, s[x] = a;
    }
    __syncthreads();
}

// ── the single-sequence prep (kernels.h: ResidentPrepArgs), in its two parts ──
// the token part: element i < T d of the T embedding rows
__device__ __forceinline__ void resident_prep_token(const ResidentPrepArgs& a, uint32_t i) {
    const uint32_t j = i / a.d, e = i - j * a.d;
    a.tok_in[i] = a.embed[(uint64_t)a.tokens[j] * a.d + e];
}
// the position part: element i of its index space (kernels.h: ResidentAhead) — the T mask columns, the T RoPE rows per layer leaf and the dynamic
// words at position `pos`; it reads no token, so a launch of the token BEFORE may write it (kernels.h: ResidentAhead)
__device__ __forceinline__ void resident_prep_position(const ResidentPrepArgs& a, uint32_t i, uint32_t pos) {
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
// ... a token ahead: element i of `total`, for the position behind the one the running step is at. Past the last position there
// is nothing to prepare (a call's last step may stand there): nothing is written, so no index leaves the mask or the tables
__device__ __forceinline__ void resident_prep_ahead(const ResidentAhead& h, uint32_t i) {
    if (i >= h.total) return;
    const uint32_t pos = h.a.state[1] + 1;
    if ((uint64_t)pos + h.a.T <= h.a.max_seq) resident_prep_position(h.a, i, pos);
}

// ── argmax: first index of the maximum (strict >), nn.zig:122-138 ──────────────────────────
constexpr int kArgBlock = 256; // threads of every argmax workgroup: the reductions below are this wide

__device__ __forceinline__ void arg_combine(float& bv, int64_t& bi, float v, int64_t i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}
// ... where a pair whose index is INT64_MAX is empty (a thread, or a workgroup, that saw no element)
__device__ __forceinline__ void arg_fold(float& bv, int64_t& bi, float v, int64_t i) {
    if (i == INT64_MAX) return;
    if (bi == INT64_MAX)
        bv = v, bi = i;
    else
        arg_combine(bv, bi, v, i);
}

// this thread's pair over row[0, n), which nblk workgroups share: elements blockIdx.x * 256 + threadIdx.x, then nblk * 256 apart
__device__ __forceinline__ void arg_scan(const float* __restrict__ row, uint64_t n, uint32_t nblk, float& bv, int64_t& bi) {
    bv = -INFINITY, bi = INT64_MAX;
    for (uint64_t i = (uint64_t)blockIdx.x * kArgBlock + threadIdx.x; i < n; i += (uint64_t)nblk * kArgBlock) {
        const float x = row[i];
        if (x > bv || bi == INT64_MAX) { // strict >: earlier index wins within a thread's ascending walk
            bv = x;
            bi = (int64_t)i;
        }
    }
}

// ... over the tokens a state row allows (spec.h: DRAFTS FROM A MODEL UNDER A CONSTRAINT): crow = next[s], staged in LDS, class_of
// a global-address-space pointer (sample.hip: select_body). Both loads stand in front of the test; a thread that saw no allowed
// token keeps the empty pair, and an allowed -inf is taken while the pair is empty: the first allowed token wins when nothing beats it
template <class ClassOf>
__device__ __forceinline__ void arg_scan_masked(const float* __restrict__ row, uint64_t n, uint32_t nblk, const uint16_t* crow, ClassOf class_of, float& bv, int64_t& bi) {
    bv = -INFINITY, bi = INT64_MAX;
    for (uint64_t i = (uint64_t)blockIdx.x * kArgBlock + threadIdx.x; i < n; i += (uint64_t)nblk * kArgBlock) {
        const float x = row[i];
        const uint16_t cls = class_of[i];
        if (constraint_row_allows(crow, cls) && (x > bv || bi == INT64_MAX)) {
            bv = x;
            bi = (int64_t)i;
        }
    }
}

// the workgroup's pair from its 256 threads' into sv[0], si[0] (two LDS arrays of 256); kEmptyAware: with arg_fold, for pairs
// that may be empty. Ends with a barrier
template <bool kEmptyAware>
__device__ __forceinline__ void arg_block_reduce(float* sv, int64_t* si, float bv, int64_t bi) {
    sv[threadIdx.x] = bv, si[threadIdx.x] = bi;
    __syncthreads();
    for (int off = kArgBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            if constexpr (kEmptyAware)
                arg_fold(sv[threadIdx.x], si[threadIdx.x], sv[threadIdx.x + off], si[threadIdx.x + off]);
            else
                arg_combine(sv[threadIdx.x], si[threadIdx.x], sv[threadIdx.x + off], si[threadIdx.x + off]);
        }
        __syncthreads();
    }
}

// the empty-aware fold of nblk stage-1 pairs by one wave: every lane ends with the row's pair
__device__ __forceinline__ void arg_wave_fold(const float* vals, const int64_t* idxs, uint32_t nblk, uint32_t lane, float& bv, int64_t& bi) {
    bv = -INFINITY, bi = INT64_MAX;
    for (uint32_t i = lane; i < nblk; i += 64) arg_fold(bv, bi, vals[i], idxs[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int64_t oi = __shfl_xor(bi, off, 64);
        arg_fold(bv, bi, ov, oi);
    }
}

// ── the advance of the loops' device state behind a pick, by one thread ──
// The single loop (kernels.h: ArgmaxAdvance, SampleAdvance): st[0] token, [1] position, [2] produced, tokens[cap]; `stop` — a
// sampled stop token — sets st[3] behind its own advance and freezes the sequence. Returns the advanced position.
__device__ __forceinline__ uint32_t tail_advance_single(uint32_t* st, int64_t* tokens, uint32_t cap, int64_t next, bool stop = false) {
    const uint32_t produced = st[2], pos_next = st[1] + 1;
    if (produced < cap) tokens[produced] = next;
    st[0] = (uint32_t)next;
    st[1] = pos_next;
    st[2] = produced + 1;
    if (stop) st[3] = 1;
    return pos_next;
}
// Sequence b of the batched loop (kernels.h): st[b] token, [B + b] position, [2 B + b] steps left, [3 B + b] produced, row length
// st[4 B]. For a sequence with steps left only: the caller has seen left > 0 (one without repeats its step at the same position).
// `stop` leaves it no steps.
__device__ __forceinline__ void tail_advance_batched(uint32_t* st, int64_t* tokens, uint32_t B, uint32_t b, int64_t next, bool stop = false) {
    const uint32_t left = st[2 * B + b], produced = st[3 * B + b], cap = st[4 * B];
    if (produced < cap) tokens[(uint64_t)b * cap + produced] = next;
    st[b] = (uint32_t)next;
    st[B + b] += 1;
    st[2 * B + b] = stop ? 0 : left - 1;
    st[3 * B + b] = produced + 1;
}

// One execution of the draft program inside a verify step (kernels.h: DraftAdvance; spec.h: DRAFTS FROM A MODEL): the draft's
// greedy token d becomes the token of its next execution, a position further, and — every execution but the step's last — the
// next candidate of the target's verify step. No count, no table: what is emitted is the accept launch's business.
// Sequence b of adv.n_seqs, over the batched loop's first two state rows (token, position); a plain draft is b = 0 of 1.
__device__ __forceinline__ void tail_advance_draft(const DraftAdvance& adv, uint32_t b, uint32_t d) {
    adv.state[b] = d;
    adv.state[adv.n_seqs + b] += 1;
    if (adv.cand_next) adv.cand_next[(uint64_t)b * adv.cand_stride] = d;
}

// ... under the target's constraint (kernels.h: DraftConstraint; spec.h: DRAFTS FROM A MODEL UNDER A CONSTRAINT): d is the masked
// first maximum under the row state the walk stands at, -1 when the fold was empty. No draft — a dead state, or one that allows
// no token — repeats the draft's token and makes the next row dead. The step's last execution (no cand_next) writes no row state
// and counts nothing
__device__ __forceinline__ void tail_advance_draft_constrained(const DraftAdvance& adv, const DraftConstraint& dc, const SampleConstraintRow& cr, uint32_t b, int64_t d) {
    uint32_t* const rs = dc.row_state + (uint64_t)b * dc.stride;
    uint32_t c_next, s_next;
    const uint32_t placed = spec_draft_advance_constrained(adv.state[b], rs[0], d, cr.class_of, cr.next, cr.n_classes, &c_next, &s_next);
    tail_advance_draft(adv, b, c_next);
    if (adv.cand_next) rs[1] = s_next, dc.drafted[(uint64_t)b * dc.drafted_stride] += placed;
}

// ── the log-probability finish (the rule: sample.h, THE LOG-PROBABILITY) ──
// Which token row `row` of a finish launch evaluates and where its value goes (kernels.h: LogprobTarget, the first form whose
// pointer is set; none — zgml_hip_top_logprobs — there is no chosen token, dst stays null and the entry is the row).
struct LogprobSlot {
    uint32_t tok = 0, produced = 0;
    float* dst = nullptr;
    uint64_t entry = 0;
};
// false: a step of the loops that emitted nothing writes nothing — the whole workgroup leaves (uniform: call it before any barrier).
// A frozen sequence's produced count stands still, and the logits of its later steps are those of another position
__device__ __forceinline__ bool logprob_resolve(const LogprobTarget& t, uint32_t row, LogprobSlot& s) {
    s.entry = row;
    if (t.tokens) {
        s.tok = t.tokens[row], s.dst = t.out + row;
    } else if (t.token64) {
        s.tok = (uint32_t)t.token64[0], s.dst = t.out, s.entry = 0;
    } else if (t.picks) {
        s.tok = t.picks[row], s.dst = t.out + row;
    } else if (t.state) {
        const uint32_t B = t.n_seqs;
        s.produced = B ? t.state[3 * B + row] : t.state[2];
        const uint32_t cap = B ? t.state[4 * B] : t.cap;
        if (s.produced <= t.written[row] || s.produced > cap) return false;
        s.entry = (uint64_t)(B ? row : 0) * cap + (s.produced - 1);
        s.tok = (uint32_t)t.emitted[s.entry], s.dst = t.out + s.entry;
    }
    return true;
}
// One wave, lane `lane`: the row's M (order-free) into every lane, and the blocks' terms s_b * sample_exp(m_b - M) into term[0, nb)
// (LDS; a barrier before they are read). pr: the row's nb (m_b, s_b) pairs
__device__ __forceinline__ float logprob_row_terms(const float* __restrict__ pr, uint32_t nb, uint32_t lane, float* term) {
    float M = -INFINITY;
    for (uint32_t b = lane; b < nb; b += 64) M = pr[2 * b] > M ? pr[2 * b] : M;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(M, off, 64);
        M = o > M ? o : M;
    }
    for (uint32_t b = lane; b < nb; b += 64) term[b] = logprob_block_term(pr[2 * b], pr[2 * b + 1], M);
    return M;
}
// ... and their sum over ascending b, by one thread
__device__ __forceinline__ float logprob_row_sum(const float* term, uint32_t nb) {
    float S = 0.0f;
    for (uint32_t b = 0; b < nb; b++) S = S + term[b];
    return S;
}
// ... and the chosen token's value, by one thread; `row`: the row's n logits
__device__ __forceinline__ void logprob_store_chosen(const LogprobTarget& t, const LogprobSlot& s, uint32_t row_index, const float* __restrict__ row, uint32_t n, float M, float S) {
    if (s.dst) *s.dst = s.tok < n ? logprob_of(row[s.tok], M, S) : sample_bits_f32(kLogprobNaNBits); // (a token is an index of its row — or, the picks form under a constraint, kSpecNoPick, a row without a pick: the NaN, and nothing indexes the row with it)
    if (t.written) t.written[row_index] = s.produced;
}

} // namespace zgml
