// spec_decode.hip — the two serial tails of a speculative verify step (zgml_hip_resident_decode_speculative, runtime_resident.hip:
// per step [draft] [prep, T tokens] [plan] [argmax stage 1 over T rows] [accept + advance]; the sampled form has sample.hip's
// [select] [merge + pick] over the T rows in the place of the argmax stage). Both are one workgroup and launches of
// their own: DESIGN section 0.2 item 5 measured that folding such tails into a neighbouring launch is slower. The rules themselves
// (which tokens are drafted, how many are accepted) are spec.h's; here is only how a workgroup evaluates them.
// Each body is stated once, as a device function over ONE sequence's SpecArgs: the single-sequence kernels hand it their
// arguments, the batched kernels (zgml_hip_resident_decode_batch_speculative, its sampled and its constrained form; blockIdx.x =
// sequence) the sequence's view of theirs.
#include "kernels.h"
#include "spec.h"
#include "tail_device.h"

namespace zgml {
namespace {

constexpr int kSpecBlock = 256;
constexpr int kSpecWaves = kSpecBlock / 64;

// (thread 0, the constrained form) the pass of spec.h's rule behind the mode's candidates: the candidates a forced token or a
// re-evaluated pad replaces, the rows' states, and what `drafted` grows by beside the mode's `real`
__device__ __forceinline__ uint32_t spec_constrain(const SpecArgs& a, uint32_t real) {
    if (!a.con_row) return 0;
    const SampleConstraintRow cr = *a.con_row;
    if (!cr.con_active) return spec_free_rows(a.row_state, a.T); // (a batched sequence without an automaton beside others: spec.h)
    return spec_constrain_candidates(a.cand, a.T, real, *a.con_state, cr.class_of, cr.next, cr.n_classes, cr.forced, a.row_state);
}

// (thread 0, the model mode) what the draft launch leaves of the rows' states, and what `drafted` grows by up front. Without a
// constraint: nothing, and the mode's T - 1. Under one (spec.h: DRAFTS FROM A MODEL UNDER A CONSTRAINT) row 0 gets the sequence's
// state — the walk starts there; the masked draft executions write the rows behind it and count their own drafts —, and nothing
// is counted here
__device__ __forceinline__ uint32_t spec_model_rows(const SpecArgs& a, uint32_t real) {
    if (!a.con_row) return real;
    if (!a.con_row->con_active) return real + spec_free_rows(a.row_state, a.T);
    a.row_state[0] = *a.con_state;
    return 0;
}

// The candidates of this step into a.cand (what the prep launch reads as its T token ids) and the position it runs at into the
// run words. Lookup mode: for n = ngram .. 1 the threads walk the match positions [n - 1, pos - 1] downwards, 256 apart — a
// thread's first hit is its largest —, the largest hit of the workgroup is folded with wave shuffles and one pass over LDS, and
// the first n with a hit wins. Provided mode is a table read. The model mode (spec.h: DRAFTS FROM A MODEL) writes c[0] and hands
// (c[0], position) to the draft program's state words — token at draft_state[0], position a.draft_pos words behind it: a plain
// draft's two words, or sequence b's of a batched draft's state —: the draft executions between this launch and the prep fill in the rest.
// Under the target's constraint it also hands the walk its first state, row_state[0] (spec_model_rows).
// Thread 0 writes. fold: kSpecWaves LDS words.
// kIdleAtEnd: where a sequence that has its count runs its idle steps (below).
template <bool kIdleAtEnd>
__device__ __forceinline__ void spec_draft_body(const SpecArgs& a, int32_t* fold) {
    uint32_t* const w = a.words;
    const uint32_t pos = w[kSpecPos], lo = w[kSpecHistLo];
    if (w[kSpecProduced] >= w[kSpecWanted]) {
        // nothing left to produce: the step still runs (it is part of a graph the host has already launched), so it repeats the
        // last confirmed token at its own position — that KV column is rewritten from the same context, everything behind it is
        // unspecified anyway — and the accept launch leaves the state alone. (produced >= 1 here: pos - 1 >= start_pos >= lo.)
        // kIdleAtEnd, the batched loop, where a sequence may want no token at all and hist[pos - 1] need not exist: the token
        // that IS confirmed but not yet cached, hist[pos], at pos — the T columns from the sequence's end position are unspecified.
        if (threadIdx.x == 0) {
            const uint32_t at = !kIdleAtEnd && pos > lo ? pos - 1 : pos;
            for (uint32_t j = 0; j < a.T; j++) a.cand[j] = a.hist[at];
            for (uint32_t j = 0; a.row_state && j < a.T; j++) a.row_state[j] = kConstraintDead; // (no row of an idle step picks)
            w[kSpecRunPos] = at;
            if (a.draft_state) a.draft_state[0] = a.hist[at], a.draft_state[a.draft_pos] = at; // (the draft program idles from the same token and position)
        }
        return;
    }
    if (w[kSpecMode] == 2) { // drafts from a model: c[0] and the draft program's first execution; its advances write c[1..T-1]
        if (threadIdx.x == 0) {
            const uint32_t real = spec_candidates_model(a.hist[pos], a.T, a.cand);
            w[kSpecDrafted] += spec_model_rows(a, real);
            w[kSpecRunPos] = pos;
            a.draft_state[0] = a.hist[pos], a.draft_state[a.draft_pos] = pos;
        }
        return;
    }
    if (w[kSpecMode] == 1) {
        if (threadIdx.x == 0) {
            const uint32_t real = spec_candidates_provided(a.hist[pos], pos, w[kSpecStart], a.drafts, w[kSpecNDrafts], a.T, a.cand);
            w[kSpecDrafted] += real + spec_constrain(a, real);
            w[kSpecRunPos] = pos;
        }
        return;
    }
    // the lookup sees positions [lo, pos]: re-based to start at 0
    const uint32_t* const h = a.hist + lo;
    const uint32_t p = pos - lo;
    int32_t best = -1;
    for (uint32_t n = w[kSpecNgram]; n >= 1 && best < 0; n--) { // (uniform: every thread reads the same fold[])
        if (!spec_ngram_applies(p, n)) continue;
        int32_t hit = -1;
        for (int64_t i = (int64_t)p - 1 - threadIdx.x; i >= (int64_t)n - 1; i -= kSpecBlock)
            if (spec_ngram_equal(h, p, n, (uint32_t)i)) {
                hit = (int32_t)i;
                break;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) hit = max(hit, __shfl_xor(hit, off, 64));
        if ((threadIdx.x & 63) == 0) fold[threadIdx.x >> 6] = hit;
        __syncthreads();
        best = fold[0];
#pragma unroll
        for (int k = 1; k < kSpecWaves; k++) best = max(best, fold[k]);
        __syncthreads(); // fold[] is rewritten by the next n
    }
    if (threadIdx.x == 0) {
        const uint32_t real = spec_candidates_lookup(h, p, best, a.T, a.cand);
        w[kSpecDrafted] += real + spec_constrain(a, real);
        w[kSpecRunPos] = pos;
    }
}

// g[j] from the nblk stage-1 partials of logits row j (a wave per row, rows kSpecWaves apart) — or, the sampled form, read from
// a.picks —, then thread 0: how many candidates were the row's choice, what is emitted, and the advance of the state, the history
// and the counters. The sampled form cuts the emission behind the first stop token and then sets wanted = produced: every later
// step of the round idles, and the host's round loop ends on the words it reads back. With a.lp_out the log-probabilities of the
// emitted tokens go next to them: row k's value of g[k], computed for all T rows behind the pick (logprob.hip). The constrained
// form keeps kSpecNoPick through the clamp, cuts the emission in front of a reached row without a pick — which finishes the call
// too — and advances the sequence's automaton state over what came out.
// g: T LDS words; emitted: one.
__device__ __forceinline__ void spec_accept_body(const SpecArgs& a, uint32_t* g, uint32_t* emitted_word) {
    uint32_t& emitted = *emitted_word; // (the form with alternatives only) m, for the copy below
    uint32_t* const w = a.words;
    const uint32_t produced = w[kSpecProduced], wanted = w[kSpecWanted];
    if (produced >= wanted) return; // (uniform) an idle step changes nothing
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t j = threadIdx.x; a.picks && j < a.T; j += kSpecBlock) g[j] = a.picks[j] < a.vocab || a.picks[j] == kSpecNoPick ? a.picks[j] : 0u; // (a pick is an index of its row or no pick at all: the clamp never acts)
    for (uint32_t j = threadIdx.x >> 6; !a.picks && j < a.T; j += kSpecWaves) {
        float bv;
        int64_t bi;
        arg_wave_fold(a.pval + (uint64_t)j * a.nblk, a.pidx + (uint64_t)j * a.nblk, a.nblk, lane, bv, bi); // (first maximum wins: tail_device.h)
        if (lane == 0) g[j] = (uint64_t)bi < a.vocab ? (uint32_t)bi : 0u; // (a row always has vocab > 0 entries: the clamp is for the embedding gather's sake)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t pos = w[kSpecPos];
        const uint32_t acc = spec_accept(a.cand, g, a.T);
        uint32_t m = spec_emit_count(acc, wanted, produced);
        bool stopped = false, dead = false;
        m = spec_dead_end_cut(g, acc, m, &dead); // (the constrained form alone has rows without a pick) possibly nothing is left
        if (a.sparams) m = spec_stop_cut(g, m, a.sparams->n_stop, a.sparams->stop, &stopped); // (read in place, as the merge kernel does)
        for (uint32_t k = 0; k < m; k++) {
            if (produced + k < a.tokens_cap) a.tokens[produced + k] = (int64_t)g[k];
            if (a.lp_out && produced + k < a.tokens_cap) a.lp_out[produced + k] = a.lp_rows[k];
            if (pos + 1 + k < a.hist_cap) a.hist[pos + 1 + k] = g[k];
        }
        if (m) w[kSpecTok] = g[m - 1];
        w[kSpecPos] = pos + m;
        w[kSpecProduced] = produced + m;
        if (stopped || dead) w[kSpecWanted] = produced + m; // the call is finished
        if (a.con_row && a.con_row->con_active) // the sequence's state, over exactly the emitted tokens (a stop token too)
            *a.con_state = spec_state_advance(g, m, *a.con_state, a.con_row->class_of, a.con_row->next, a.con_row->n_classes);
        w[kSpecSteps] += 1;
        w[kSpecAccepted] += acc;
        emitted = m;
    }
    if (!a.top_tok_out) return; // (uniform)
    // the alternatives of the emitted tokens next to them: row k's 64 pairs to entry produced + k, all threads
    __syncthreads();
    const uint32_t m = emitted;
    for (uint32_t i = threadIdx.x; i < m * kTopLogprobsMax; i += kSpecBlock) {
        const uint32_t k = i / kTopLogprobsMax, j = i % kTopLogprobsMax;
        if (produced + k >= a.tokens_cap) continue;
        a.top_tok_out[(uint64_t)(produced + k) * kTopLogprobsMax + j] = a.top_rows_tok[i];
        a.top_val_out[(uint64_t)(produced + k) * kTopLogprobsMax + j] = a.top_rows_val[i];
    }
}

// sequence b's view of a batched launch's arguments (kernels.h: SpecBatchArgs)
__device__ __forceinline__ SpecArgs spec_seq_view(const SpecBatchArgs& ba, uint32_t b) {
    SpecArgs v = ba.a;
    const uint32_t cap = ba.a.words[(uint64_t)ba.n_seqs * kSpecWords]; // row length of this call's token table
    v.words += (uint64_t)b * kSpecWords;
    v.hist += (uint64_t)b * v.hist_cap;
    v.drafts += (uint64_t)b * ba.drafts_stride;
    v.cand += (uint64_t)b * v.T;
    v.tokens += (uint64_t)b * cap, v.tokens_cap = cap;
    v.pval += (uint64_t)b * v.T * v.nblk, v.pidx += (uint64_t)b * v.T * v.nblk;
    // the sampled form: the sequence's T picks, its parameter set (the stop tokens), its T row values and its values' row
    if (v.picks) v.picks += (uint64_t)b * v.T, v.sparams += b;
    if (v.lp_out) v.lp_rows += (uint64_t)b * v.T, v.lp_out += (uint64_t)b * cap;
    // the constrained form: the sequence's row of the table (con_active = 0: none attached to it), its state word, its T row states
    if (v.con_row) v.con_row += b, v.con_state += b, v.row_state += (uint64_t)b * v.T;
    // drafts from a batched draft model: the sequence's token word of the draft's state (its position word draft_pos = n_seqs behind it)
    if (v.draft_state) v.draft_state += b;
    return v;
}

__global__ void __launch_bounds__(kSpecBlock) spec_draft_kernel(SpecArgs a) {
    __shared__ int32_t fold[kSpecWaves];
    spec_draft_body<false>(a, fold);
}
__global__ void __launch_bounds__(kSpecBlock) spec_accept_kernel(SpecArgs a) {
    extern __shared__ uint32_t g[]; // [T]
    __shared__ uint32_t emitted;
    spec_accept_body(a, g, &emitted);
}
// the batched forms: workgroup b is sequence b
__global__ void __launch_bounds__(kSpecBlock) spec_batch_draft_kernel(SpecBatchArgs ba) {
    __shared__ int32_t fold[kSpecWaves];
    spec_draft_body<true>(spec_seq_view(ba, blockIdx.x), fold);
}
__global__ void __launch_bounds__(kSpecBlock) spec_batch_accept_kernel(SpecBatchArgs ba) {
    extern __shared__ uint32_t g[]; // [T]
    __shared__ uint32_t emitted;
    spec_accept_body(spec_seq_view(ba, blockIdx.x), g, &emitted);
}

} // namespace

void launch_spec_draft(hipStream_t s, const SpecArgs& a) { spec_draft_kernel<<<1, kSpecBlock, 0, s>>>(a); }

void launch_spec_accept(hipStream_t s, const SpecArgs& a) { spec_accept_kernel<<<1, kSpecBlock, a.T * sizeof(uint32_t), s>>>(a); }

void launch_spec_batch_draft(hipStream_t s, const SpecBatchArgs& a) { spec_batch_draft_kernel<<<a.n_seqs, kSpecBlock, 0, s>>>(a); }

void launch_spec_batch_accept(hipStream_t s, const SpecBatchArgs& a) {
    spec_batch_accept_kernel<<<a.n_seqs, kSpecBlock, a.a.T * sizeof(uint32_t), s>>>(a);
}

} // namespace zgml
