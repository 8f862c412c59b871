// sample.hip — the sampled token tail (zgml_hip_sample, zgml_hip_resident_decode_sampled / _batch_sampled and the rows of a
// sampled verify step — T of one sequence, zgml_hip_resident_decode_speculative_sampled, or T of each of B sequences,
// zgml_hip_resident_decode_batch_speculative_sampled; runtime_resident.hip): two launches per row of logits, the
// shape of launch_argmax / launch_argmax_batch. The rule — candidate order, pick, random number — is sample.h's; here is only
// how workgroups find the candidates. Keys are unique 64-bit words (sample_key), so the largest 256 of a row are one
// well-defined list whatever the slicing: nothing below depends on arrival order, no workgroup waits for another and there is
// no last-arriver stage.
//   (the rows of a verify step lie in grid planes, one per sequence — (.., rows_per_seq, sequences), SampleRow below; everything else is (.., rows))
//   [select]  grid (slices, rows), 256 threads: a workgroup walks its slice of the row in chunks of kSampleChunk logits; the 256
//             best keys so far and the chunk's keys are one 2048-key bitonic sort in LDS (16 KiB); the slice's 256 largest keys,
//             descending, go to the scratch (0 pads a slice of fewer: every real key is > 0). ONE body, select_body<form>, and
//             four kernels that instantiate it (SampledSel, kernels.h); a form only adds to the one before it:
//     sample_select_kernel              the plain form, nothing else.
//     sample_select_penalized_kernel    when a row has penalties (sample.h): the workgroup loads its row's
//             window — at most 256 token ids, one per thread — into LDS (select_window), every thread counts its entry
//             (sample_window_count), and behind the fill of every chunk each first occurrence whose token lies in the chunk
//             rewrites that one key with the key of the penalised logit. The cost does not depend on the vocabulary: there is no
//             table of counts.
//     sample_select_constrained_kernel  when a row has a token automaton attached (sample.h: THE CONSTRAINT; DESIGN section
//             4.16): the workgroup also stages the row next[state] of its sequence's current state — at most 8192 u16 words,
//             16 KiB — into LDS, reads class_of[i] beside row[i] when it fills a chunk and writes the pad 0 for a token that is
//             not allowed: it is no candidate at all; the penalty rewrite acts on the allowed window tokens alone.
//     sample_select_constrained_rows_kernel  the T rows of a constrained sequence's verify step (spec.h: UNDER A CONSTRAINT;
//             DESIGN section 4.18), or the T rows of each of B sequences (zgml_hip_resident_decode_batch_speculative_constrained;
//             DESIGN section 4.21): the constrained form with the automaton of the row's SEQUENCE — the grid plane — and a state
//             word per ROW — every workgroup stages next[row_state[b]] —, the sequence's parameter row and the verify step's
//             window. A dead row (no state) writes its 256 pads and skips the fill; the rows of a sequence without an automaton
//             are free (spec.h) and go through the penalised instantiation of the body inside this kernel.
//   [merge + pick + advance]  grid (1, rows), 1024 threads, the same launch behind every form: the slices' lists — at most
//             32 x 256 keys, 64 KiB of LDS — are loaded with every second list reversed, which is the state of a bitonic sort
//             after its 256-runs: only the merge stages from 512 up remain. Then the threads fill p[j] (sample_prob), thread 0
//             counts the real keys among the first top_k (fewer allowed tokens than top_k shorten the list), walks
//             sample_pick_probs at the form's position, advances the constraint's state word — it lives on the device — and the
//             loop's state (tail_device.h).
#include "kernels.h"
#include "spec.h"
#include "tail_device.h"

namespace zgml {
namespace {

constexpr uint32_t kSelBlock = 256, kSelKeys = 2048;   // kSelKeys = kSampleMaxK + kSampleChunk
constexpr uint32_t kMergeBlock = 1024, kMergeKeys = kSampleMaxSlices * kSampleMaxK;
static_assert(kSelKeys == kSampleMaxK + kSampleChunk, "a select sort holds the best so far and one chunk");
static_assert(kMergeKeys * sizeof(uint64_t) <= 65536, "the merge's lists must fit the static LDS limit");
static_assert(kSelBlock == kSamplePenaltyMaxWindow, "a thread per window entry");
static_assert(sizeof(uint64_t) * kSelKeys + 4 * kSamplePenaltyMaxWindow + 2 * kConstraintMaxClasses <= 65536, "keys, window and state row must fit the static LDS limit");

// The logits row of a workgroup of either launch. The grids are (.., rows, 1) — row = blockIdx.y, as ever — or, the picks form
// (kernels.h: SampleAdvance), (.., rows_per_seq, sequences): row = seq * rows_per_seq + cand with seq = blockIdx.z, cand = blockIdx.y.
// One sequence's verify step is the case sequences = 1.
struct SampleRow {
    uint32_t row, seq, cand;
};
__device__ __forceinline__ SampleRow sample_row() { return {blockIdx.z * gridDim.y + blockIdx.y, blockIdx.z, blockIdx.y}; }

// Row b's window from where SampleWindow says (kernels.h): its length m, and entry t < m into thread t's `tok`. kVerifyRows: the
// rows may be those of a verify step (the constrained form never serves one; the constrained-rows form serves nothing else)
template <bool kVerifyRows>
__device__ __forceinline__ uint32_t select_window(const SampleParamsDev& sp, const SampleAdvance& adv, const SampleWindow& w, uint32_t b, uint32_t& tok) {
    uint32_t m, first;
    if (kVerifyRows && adv.picks) { // row b of a verify step: candidate row j of its sequence
        const uint32_t seq = sample_row().seq, j = sample_row().cand;
        const uint32_t run = adv.pos_word[(uint64_t)seq * adv.pos_stride], P = run + j;
        const uint32_t* const hist = w.hist + (uint64_t)seq * w.hist_stride;
        const uint32_t* const cand = w.cand + (uint64_t)seq * adv.rows_per_seq;
        m = sample_window_span(P, w.lo_word[(uint64_t)seq * adv.pos_stride], sp.window, &first);
        if (threadIdx.x < m) {
            const uint32_t q = first + threadIdx.x;
            tok = q <= run ? hist[q] : cand[q - run];
        }
    } else if (!adv.state) { // the blocking form: the list is the window
        m = w.n_list < sp.window ? w.n_list : sp.window;
        if (threadIdx.x < m) tok = w.list[w.n_list - m + threadIdx.x];
    } else { // the loops: the sequence's ring, and the token being fed, which this launch files at its position
        const uint32_t B = adv.n_seqs;
        const uint32_t cur = B ? adv.state[b] : adv.state[0], P = B ? adv.state[B + b] : adv.state[1];
        uint32_t* const ring = w.ring + (uint64_t)b * kSamplePenaltyMaxWindow;
        m = sample_window_span(P, w.lo[b], sp.window, &first);
        if (threadIdx.x < m) {
            const uint32_t q = first + threadIdx.x;
            tok = q == P ? cur : ring[q & (kSamplePenaltyMaxWindow - 1)];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) ring[P & (kSamplePenaltyMaxWindow - 1)] = cur; // (the slot of P - 256: outside every window read here)
    }
    return m;
}

// The select launch of row b = sample_row().row, slice blockIdx.x, in its four forms. s: kSelKeys keys of LDS; win: the window's 256
// words (from kSelPenalized on); crow: the state row's kConstraintMaxClasses words (kSelConstrained). `active` (the row has
// penalties) and `constrained` are uniform over the workgroup: the barriers hang on them. A row with neither computes what the
// plain form computes, a row with penalties alone what the penalised form computes — a batched sequence beside others.
// kSelConstrainedRows: cr is the automaton of the row's SEQUENCE and con_state[b] the state of ROW b (spec.h: dead, or a state of
// cr). A FREE row — its sequence has no automaton — selects as the penalised or the plain form does: the rows kernel hands it to
// the penalised instantiation (below), so here `constrained` holds for every row that is not all pads, as in the one-sequence call.
template <SampledSel kForm>
__device__ __forceinline__ void select_body(uint64_t* s, uint32_t* win, uint16_t* crow, const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                            const SampleParamsDev* __restrict__ params, const SampleAdvance& adv, const SampleWindow& w, const SampleConstraintRow& cr, const uint32_t* con_state) {
    constexpr bool kRows = kForm == kSelConstrainedRows, kMask = kForm == kSelConstrained || kRows, kWindow = kForm != kSelPlain;
    const uint32_t b = sample_row().row;
    const bool constrained = kMask && cr.con_active != 0;
    if (kRows && (!constrained || !spec_row_selects(con_state[b]))) { // (uniform, before any barrier) a dead row has no candidates: all pads
        uint64_t* out = part + ((uint64_t)b * gridDim.x + blockIdx.x) * kSampleMaxK;
        for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) out[t] = 0;
        return;
    }
    // (cr's pointers were read from a device table, and inside a function the compiler takes such a pointer for a generic one:
    // the type says that they point to global memory, so the loads of the fill loop are global loads, not flat ones)
    using global_u16 = const __attribute__((address_space(1))) uint16_t;
    global_u16* const class_of = (global_u16*)cr.class_of;
    // (class_of[token] < n_classes: zgml_hip_constraint_create refuses a table where it is not)
    [[maybe_unused]] const auto allowed = [&](uint32_t token) { return constraint_row_allows(crow, class_of[token]); };
    if (constrained) { // the row of the sequence's current state (the word is known only now, never at capture)
        global_u16* const from = (global_u16*)cr.next + (uint64_t)con_state[b] * cr.n_classes;
        for (uint32_t t = threadIdx.x; t < cr.n_classes; t += kSelBlock) crow[t] = from[t];
    }
    // (read in place; the plain form has no parameters and reads none)
    // (a verify row reads its sequence's parameter row: the block index, a scalar — nothing divides)
    const SampleParamsDev* const sp = kWindow ? params + (kRows || (!kMask && adv.picks) ? sample_row().seq : b) : nullptr;
    const bool active = kWindow && sp->pen_active != 0;
    uint32_t tok = 0, count = 0;
    if (active) {
        const uint32_t m = select_window<!kMask || kRows>(*sp, adv, w, b, tok);
        if (threadIdx.x < m) win[threadIdx.x] = tok;
        __syncthreads();
        if (threadIdx.x < m) count = sample_window_count(win, m, threadIdx.x);
    }
    if (constrained) __syncthreads(); // crow is whole before the first fill reads it
    const float* row = v + (uint64_t)b * n;
    const uint64_t lo = (uint64_t)blockIdx.x * len, hi = lo + len < n ? lo + len : n; // (lo may lie behind n: an empty slice, all pads)
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) s[t] = 0;
    for (uint64_t base = lo; base == lo || base < hi; base += kSampleChunk) {
        for (uint32_t t = threadIdx.x; t < kSampleChunk; t += kSelBlock) {
            const uint64_t i = base + t;
            s[kSampleMaxK + t] = i < hi && (!constrained || allowed((uint32_t)i)) ? sample_key(row[i], (uint32_t)i) : 0;
        }
        if (active) {
            __syncthreads(); // the slot below was filled by another thread
            // distinct tokens, distinct slots: no two threads write one key. A token >= n lies in no chunk; a token that is
            // not allowed keeps its pad
            if (count && tok >= base && tok < hi && tok - base < kSampleChunk && (!constrained || allowed(tok)))
                s[kSampleMaxK + (uint32_t)(tok - base)] = sample_key(sample_penalize(row[tok], count, sp->repeat, sp->inv_repeat, sp->presence, sp->frequency), tok);
        }
        __syncthreads();
        for (uint32_t k = 2; k <= kSelKeys; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kSelBlock>(s, kSelKeys / 2, k, j);
    }
    uint64_t* out = part + ((uint64_t)b * gridDim.x + blockIdx.x) * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) out[t] = s[t];
}

__global__ void __launch_bounds__(kSelBlock) sample_select_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part) {
    __shared__ uint64_t s[kSelKeys];
    select_body<kSelPlain>(s, nullptr, nullptr, v, n, len, part, nullptr, SampleAdvance{}, SampleWindow{}, SampleConstraintRow{}, nullptr);
}

__global__ void __launch_bounds__(kSelBlock) sample_select_penalized_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                                                            const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleWindow w) {
    __shared__ uint64_t s[kSelKeys];
    __shared__ uint32_t win[kSamplePenaltyMaxWindow];
    select_body<kSelPenalized>(s, win, nullptr, v, n, len, part, params, adv, w, SampleConstraintRow{}, nullptr);
}

// LDS: 16 KiB of keys, 1 KiB of window, at most 16 KiB of state row — 33 KiB, four workgroups of 256 threads per CU still fit the 160 KiB
__global__ void __launch_bounds__(kSelBlock) sample_select_constrained_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                                                              const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleWindow w,
                                                                              SampleConstraint con) {
    __shared__ uint64_t s[kSelKeys];
    __shared__ uint32_t win[kSamplePenaltyMaxWindow];
    __shared__ uint16_t crow[kConstraintMaxClasses];
    const SampleConstraintRow cr = con.rows[blockIdx.y];
    select_body<kSelConstrained>(s, win, crow, v, n, len, part, params, adv, w, cr, con.state);
}

// the rows of a verify step: plane blockIdx.z holds the rows of sequence blockIdx.z, which walk that sequence's automaton (one
// plane: the single-sequence call, sequence 0's); con.state = the row states of all planes
__global__ void __launch_bounds__(kSelBlock) sample_select_constrained_rows_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                                                                   const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleWindow w,
                                                                                   SampleConstraint con) {
    __shared__ uint64_t s[kSelKeys];
    __shared__ uint32_t win[kSamplePenaltyMaxWindow];
    __shared__ uint16_t crow[kConstraintMaxClasses];
    const SampleConstraintRow cr = con.rows[blockIdx.z];
    if (!cr.con_active && spec_row_selects(con.state[sample_row().row])) { // (uniform) a free row: what the penalised form computes
        select_body<kSelPenalized>(s, win, nullptr, v, n, len, part, params, adv, w, SampleConstraintRow{}, nullptr);
        return;
    }
    select_body<kSelConstrainedRows>(s, win, crow, v, n, len, part, params, adv, w, cr, con.state);
}

__global__ void __launch_bounds__(kMergeBlock) sample_merge_pick_kernel(const uint64_t* __restrict__ part, uint32_t n, uint32_t slices, uint32_t P,
                                                                        const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleConstraint con) {
    __shared__ uint64_t s[kMergeKeys];
    const uint32_t b = sample_row().row;
    const uint64_t* lists = part + (uint64_t)b * slices * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < P; t += kMergeBlock) { // P = sample_merge_keys(slices, 256), <= kMergeKeys
        const uint32_t l = t >> 8, off = t & 255;
        s[t] = l < slices ? lists[(uint64_t)l * kSampleMaxK + ((l & 1) ? 255 - off : off)] : 0;
    }
    __syncthreads();
    for (uint32_t k = 2 * kSampleMaxK; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kMergeBlock>(s, P / 2, k, j);
    // s[0, 256): the row's largest keys, descending
    const SampleParamsDev& sp = params[adv.picks ? sample_row().seq : b]; // (read in place: a copy with its indexed stop[] would live in scratch)
    // The row's k: the real (non-zero) keys among the first sample_top_k(top_k, n). A row without a constraint has n >= that many
    // real keys — the lists hold the 256 largest of every slice — so for it kc == kc0 and nothing changes to the bit; a constrained
    // row may have fewer allowed tokens than top_k, down to none.
    const uint32_t kc0 = sample_top_k(sp.top_k, n);
    float* const p = (float*)(s + kSampleMaxK); // (the keys behind the first 256 are done with)
    const float v0 = sample_key_value(s[0]);
    if (threadIdx.x < kc0 && s[threadIdx.x] != 0) {
        p[threadIdx.x] = sample_prob(sample_key_value(s[threadIdx.x]), v0, sp.inv_temperature);
        if (adv.cand) adv.cand[1 + threadIdx.x] = sample_key_index(s[threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t kc = sample_real_keys(s, kc0);
    if (adv.cand) adv.cand[0] = kc;
    // the form's position (kernels.h: SampleAdvance), behind the form's early exits: a frozen sequence, or kc == 0 — the state
    // allows no token
    uint32_t* const st = adv.state;
    const uint32_t B = adv.n_seqs;
    uint32_t position;
    if (adv.picks) { // row b of a verify step: candidate row blockIdx.y of sequence blockIdx.z
        if (kc == 0) { // (a constrained row alone) no candidate, no pick: nothing walks sample_pick_probs over nothing
            adv.picks[b] = kSpecNoPick;
            return;
        }
        position = adv.pos_word[(uint64_t)sample_row().seq * adv.pos_stride] + sample_row().cand;
    } else if (!st) {
        if (kc == 0) {
            adv.out[0] = -1;
            return;
        }
        position = adv.position;
    } else if (B == 0) { // state[3]: a stop token was emitted, the sequence is frozen
        if (st[3]) return;
        if (kc == 0) { // frozen as behind a stop token, nothing produced, the state stays
            st[3] = 1;
            return;
        }
        position = st[1];
    } else { // only while the sequence has steps left (else it repeats the same token at the same position)
        if (st[2 * B + b] == 0) return;
        if (kc == 0) { // no steps left, nothing produced
            st[2 * B + b] = 0;
            return;
        }
        position = st[B + b];
    }
    const float u = sample_uniform(sp.seed_lo, sp.seed_hi, sp.stream, position);
    const uint32_t next = sample_key_index(s[sample_pick_probs(p, kc, sp.top_p, u)]);
    if (adv.picks) { // the pick alone, the advance is spec_accept_kernel's
        adv.picks[b] = next;
        return;
    }
    // the constraint's advance, behind the pick and before the stop check: a stop token advances the state too
    if (con.rows && con.rows[b].con_active) {
        const SampleConstraintRow& cr = con.rows[b];
        con.state[b] = constraint_advance(cr.next, cr.n_classes, cr.class_of, con.state[b], next);
    }
    if (!st)
        adv.out[0] = (int64_t)next;
    else if (B == 0)
        tail_advance_single(st, adv.tokens, adv.cap, (int64_t)next, sample_is_stop(next, sp.n_stop, sp.stop));
    else
        tail_advance_batched(st, adv.tokens, B, b, (int64_t)next, sample_is_stop(next, sp.n_stop, sp.stop));
}

} // namespace

void launch_sample(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch, const SampleParamsDev* params, const SampleAdvance& adv,
                   SampledSel sel, const SampleWindow& win, const SampleConstraint& con) {
    if (!n || n > 0xFFFFFFFFull || !rows) return; // (the callers refuse these)
    if (adv.picks && (!adv.rows_per_seq || rows % adv.rows_per_seq)) return; // (whole sequences of verify rows)
    if (sel == kSelConstrained && (adv.picks || !con.rows || !con.state)) return;
    if (sel == kSelConstrainedRows && (!adv.picks || !con.rows || !con.state)) return;
    const uint32_t slices = sample_slices(n), len = sample_slice_len(n);
    // (the picks form: whole sequences of rows_per_seq verify rows, one grid plane per sequence)
    const dim3 rows_grid = adv.picks ? dim3(1, adv.rows_per_seq, rows / adv.rows_per_seq) : dim3(1, rows, 1);
    const dim3 grid(slices, rows_grid.y, rows_grid.z);
    if (sel == kSelConstrainedRows)
        sample_select_constrained_rows_kernel<<<grid, kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch, params, adv, win, con);
    else if (sel == kSelConstrained)
        sample_select_constrained_kernel<<<grid, kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch, params, adv, win, con);
    else if (sel == kSelPenalized)
        sample_select_penalized_kernel<<<grid, kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch, params, adv, win);
    else
        sample_select_kernel<<<grid, kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch);
    sample_merge_pick_kernel<<<rows_grid, kMergeBlock, 0, s>>>(scratch, (uint32_t)n, slices, sample_merge_keys(slices, kSampleMaxK), params, adv,
                                                                   sel == kSelConstrained ? con : SampleConstraint{});
}

void launch_sample_select(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch) {
    if (!n || n > 0xFFFFFFFFull || !rows) return; // (the callers refuse these)
    sample_select_kernel<<<dim3(sample_slices(n), rows), kSelBlock, 0, s>>>(v, (uint32_t)n, sample_slice_len(n), scratch);
}

} // namespace zgml
