// sample.hip — the sampled token tail (zgml_hip_sample, zgml_hip_resident_decode_sampled / _batch_sampled and the T rows of a
// sampled verify step, zgml_hip_resident_decode_speculative_sampled; runtime_resident.hip): two launches per row of logits, the
// shape of launch_argmax / launch_argmax_batch. The rule — candidate order, pick, random number — is sample.h's; here is only
// how workgroups find the candidates. Keys are unique 64-bit words (sample_key), so the largest 256 of a row are one
// well-defined list whatever the slicing: nothing below depends on arrival order, no workgroup waits for another and there is
// no last-arriver stage.
//   [select]  grid (slices, rows), 256 threads: a workgroup walks its slice of the row in chunks of kSampleChunk logits; the 256
//             best keys so far and the chunk's keys are one 2048-key bitonic sort in LDS (16 KiB); the slice's 256 largest keys,
//             descending, go to the scratch (0 pads a slice of fewer: every real key is > 0).
//   [merge + pick + advance]  grid (1, rows), 1024 threads: the slices' lists — at most 32 x 256 keys, 64 KiB of LDS — are loaded
//             with every second list reversed, which is the state of a bitonic sort after its 256-runs: only the merge stages
//             from 512 up remain. Then the threads fill p[j] (sample_prob), thread 0 walks sample_pick_probs and advances.
//   [select, penalised]  sample_select_penalized_kernel, a kernel of its own in the place of [select] when a row has penalties
//             (sample.h): the workgroup loads its row's window — at most 256 token ids, one per thread — into
//             LDS, every thread counts its entry (sample_window_count), and behind the fill of every chunk each first occurrence
//             whose token lies in the chunk rewrites that one key with the key of the penalised logit. The cost does not depend
//             on the vocabulary: there is no table of counts. The merge launch is the same launch either way.
//   [select, constrained]  sample_select_constrained_kernel, a kernel of its own again, when a row has a token automaton attached
//             (sample.h: THE CONSTRAINT): the workgroup stages the row next[state] of its sequence's current
//             state — at most 8192 u16 words, 16 KiB — into LDS, reads class_of[i] beside row[i] when it fills a chunk and writes the
//             pad 0 for a token that is not allowed: it is no candidate at all. The penalty rewrite, for the allowed window tokens,
//             and the sort are the penalised kernel's. The state word lives on the device; thread 0 of the merge launch advances
//             it behind the pick, and counts the real keys among the first top_k: fewer allowed tokens than top_k shorten the list.
#include "kernels.h"
#include "sample.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace zgml {
namespace {

constexpr uint32_t kSelBlock = 256, kSelKeys = 2048;   // kSelKeys = kSampleMaxK + kSampleChunk
constexpr uint32_t kMergeBlock = 1024, kMergeKeys = kSampleMaxSlices * kSampleMaxK;
static_assert(kSelKeys == kSampleMaxK + kSampleChunk, "a select sort holds the best so far and one chunk");
static_assert(kMergeKeys * sizeof(uint64_t) <= 65536, "the merge's lists must fit the static LDS limit");

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

__global__ void __launch_bounds__(kSelBlock) sample_select_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part) {
    __shared__ uint64_t s[kSelKeys];
    const float* row = v + (uint64_t)blockIdx.y * n;
    const uint64_t lo = (uint64_t)blockIdx.x * len, hi = lo + len < n ? lo + len : n; // (lo may lie behind n: an empty slice, all pads)
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) s[t] = 0;
    for (uint64_t base = lo; base == lo || base < hi; base += kSampleChunk) {
        for (uint32_t t = threadIdx.x; t < kSampleChunk; t += kSelBlock) {
            const uint64_t i = base + t;
            s[kSampleMaxK + t] = i < hi ? sample_key(row[i], (uint32_t)i) : 0;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= kSelKeys; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kSelBlock>(s, kSelKeys / 2, k, j);
    }
    uint64_t* out = part + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) out[t] = s[t];
}

// The penalised form of sample_select_kernel (which stays as it is: a call without penalties launches that one). Row b's window
// comes from where SampleWindow says (kernels.h); entry t is thread t's. A row whose pen_active is 0 — a batched sequence
// without penalties beside one with them — takes no branch below and computes what sample_select_kernel computes.
__global__ void __launch_bounds__(kSelBlock) sample_select_penalized_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                                                            const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleWindow w) {
    __shared__ uint64_t s[kSelKeys];
    __shared__ uint32_t win[kSamplePenaltyMaxWindow];
    static_assert(kSelBlock == kSamplePenaltyMaxWindow, "a thread per window entry");
    const uint32_t b = blockIdx.y;
    const SampleParamsDev& sp = params[adv.picks ? 0 : b];
    const bool active = sp.pen_active != 0; // (uniform over the workgroup: the barriers below hang on it)
    uint32_t tok = 0, count = 0;
    if (active) {
        uint32_t m = 0;
        if (adv.picks) { // row b of a verify step
            const uint32_t run = *adv.pos_word, P = run + b;
            uint32_t first;
            m = sample_window_span(P, *w.lo_word, sp.window, &first);
            if (threadIdx.x < m) {
                const uint32_t q = first + threadIdx.x;
                tok = q <= run ? w.hist[q] : w.cand[q - run];
            }
        } else if (!adv.state) { // the blocking form: the list is the window
            m = w.n_list < sp.window ? w.n_list : sp.window;
            if (threadIdx.x < m) tok = w.list[w.n_list - m + threadIdx.x];
        } else { // the loops: the sequence's ring, and the token being fed, which this launch files at its position
            const uint32_t B = adv.n_seqs;
            const uint32_t cur = B ? adv.state[b] : adv.state[0], P = B ? adv.state[B + b] : adv.state[1];
            uint32_t* const ring = w.ring + (uint64_t)b * kSamplePenaltyMaxWindow;
            uint32_t first;
            m = sample_window_span(P, w.lo[b], sp.window, &first);
            if (threadIdx.x < m) {
                const uint32_t q = first + threadIdx.x;
                tok = q == P ? cur : ring[q & (kSamplePenaltyMaxWindow - 1)];
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) ring[P & (kSamplePenaltyMaxWindow - 1)] = cur; // (the slot of P - 256: outside every window read here)
        }
        if (threadIdx.x < m) win[threadIdx.x] = tok;
        __syncthreads();
        if (threadIdx.x < m) count = sample_window_count(win, m, threadIdx.x);
    }
    const float* row = v + (uint64_t)b * n;
    const uint64_t lo = (uint64_t)blockIdx.x * len, hi = lo + len < n ? lo + len : n; // (lo may lie behind n: an empty slice, all pads)
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) s[t] = 0;
    for (uint64_t base = lo; base == lo || base < hi; base += kSampleChunk) {
        for (uint32_t t = threadIdx.x; t < kSampleChunk; t += kSelBlock) {
            const uint64_t i = base + t;
            s[kSampleMaxK + t] = i < hi ? sample_key(row[i], (uint32_t)i) : 0;
        }
        if (active) {
            __syncthreads(); // the slot below was filled by another thread
            // distinct tokens, distinct slots: no two threads write one key. A token >= n lies in no chunk
            if (count && tok >= base && tok < hi && tok - base < kSampleChunk)
                s[kSampleMaxK + (uint32_t)(tok - base)] = sample_key(sample_penalize(row[tok], count, sp.repeat, sp.inv_repeat, sp.presence, sp.frequency), tok);
        }
        __syncthreads();
        for (uint32_t k = 2; k <= kSelKeys; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kSelBlock>(s, kSelKeys / 2, k, j);
    }
    uint64_t* out = part + ((uint64_t)b * gridDim.x + blockIdx.x) * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) out[t] = s[t];
}

// The constrained form of the select launch (the two kernels above stay as they are: a call without a constraint launches what
// it launched before). LDS: 16 KiB of keys, 1 KiB of window, at most 16 KiB of state row — 33 KiB, four workgroups of 256 threads
// per CU still fit the 160 KiB. `constrained` and `active` are uniform over the workgroup: the barriers hang on them. A row
// with neither computes what sample_select_kernel computes, a row with penalties alone what the penalised kernel computes.
__global__ void __launch_bounds__(kSelBlock) sample_select_constrained_kernel(const float* __restrict__ v, uint32_t n, uint32_t len, uint64_t* __restrict__ part,
                                                                              const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleWindow w,
                                                                              SampleConstraint con) {
    __shared__ uint64_t s[kSelKeys];
    __shared__ uint32_t win[kSamplePenaltyMaxWindow];
    __shared__ uint16_t crow[kConstraintMaxClasses];
    static_assert(kSelBlock == kSamplePenaltyMaxWindow, "a thread per window entry");
    static_assert(sizeof(uint64_t) * kSelKeys + 4 * kSamplePenaltyMaxWindow + 2 * kConstraintMaxClasses <= 65536, "keys, window and state row must fit the static LDS limit");
    const uint32_t b = blockIdx.y;
    const SampleParamsDev& sp = params[b];
    const SampleConstraintRow cr = con.rows[b];
    const bool constrained = cr.con_active != 0, active = sp.pen_active != 0;
    if (constrained) { // the row of the sequence's current state (the word is known only now, never at capture)
        const uint16_t* const from = cr.next + (uint64_t)con.state[b] * cr.n_classes;
        for (uint32_t t = threadIdx.x; t < cr.n_classes; t += kSelBlock) crow[t] = from[t];
    }
    uint32_t tok = 0, count = 0;
    if (active) {
        uint32_t m = 0;
        if (!adv.state) { // the blocking form: the list is the window
            m = w.n_list < sp.window ? w.n_list : sp.window;
            if (threadIdx.x < m) tok = w.list[w.n_list - m + threadIdx.x];
        } else { // the loops: the sequence's ring, and the token being fed, which this launch files at its position
            const uint32_t B = adv.n_seqs;
            const uint32_t cur = B ? adv.state[b] : adv.state[0], P = B ? adv.state[B + b] : adv.state[1];
            uint32_t* const ring = w.ring + (uint64_t)b * kSamplePenaltyMaxWindow;
            uint32_t first;
            m = sample_window_span(P, w.lo[b], sp.window, &first);
            if (threadIdx.x < m) {
                const uint32_t q = first + threadIdx.x;
                tok = q == P ? cur : ring[q & (kSamplePenaltyMaxWindow - 1)];
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) ring[P & (kSamplePenaltyMaxWindow - 1)] = cur; // (the slot of P - 256: outside every window read here)
        }
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
            // (class_of[i] < n_classes: zgml_hip_constraint_create refuses a table where it is not)
            s[kSampleMaxK + t] = i < hi && (!constrained || constraint_allowed(crow, cr.class_of, (uint32_t)i)) ? sample_key(row[i], (uint32_t)i) : 0;
        }
        if (active) {
            __syncthreads(); // the slot below was filled by another thread
            // distinct tokens, distinct slots: no two threads write one key. A token >= n lies in no chunk; a token that is
            // not allowed keeps its pad
            if (count && tok >= base && tok < hi && tok - base < kSampleChunk && (!constrained || constraint_allowed(crow, cr.class_of, tok)))
                s[kSampleMaxK + (uint32_t)(tok - base)] = sample_key(sample_penalize(row[tok], count, sp.repeat, sp.inv_repeat, sp.presence, sp.frequency), tok);
        }
        __syncthreads();
        for (uint32_t k = 2; k <= kSelKeys; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kSelBlock>(s, kSelKeys / 2, k, j);
    }
    uint64_t* out = part + ((uint64_t)b * gridDim.x + blockIdx.x) * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < kSampleMaxK; t += kSelBlock) out[t] = s[t];
}

__global__ void __launch_bounds__(kMergeBlock) sample_merge_pick_kernel(const uint64_t* __restrict__ part, uint32_t n, uint32_t slices, uint32_t P,
                                                                        const SampleParamsDev* __restrict__ params, SampleAdvance adv, SampleConstraint con) {
    __shared__ uint64_t s[kMergeKeys];
    const uint32_t b = blockIdx.y;
    const uint64_t* lists = part + (uint64_t)b * slices * kSampleMaxK;
    for (uint32_t t = threadIdx.x; t < P; t += kMergeBlock) { // P = the power of two >= slices * 256, <= kMergeKeys
        const uint32_t l = t >> 8, off = t & 255;
        s[t] = l < slices ? lists[(uint64_t)l * kSampleMaxK + ((l & 1) ? 255 - off : off)] : 0;
    }
    __syncthreads();
    for (uint32_t k = 2 * kSampleMaxK; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_stage<kMergeBlock>(s, P / 2, k, j);
    // s[0, 256): the row's largest keys, descending
    const SampleParamsDev& sp = params[adv.picks ? 0 : b]; // (read in place: a copy with its indexed stop[] would live in scratch)
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
    if (adv.picks) { // row b of one sequence's verify step: the pick alone, the advance is spec_accept_kernel's
        const float u = sample_uniform(sp.seed_lo, sp.seed_hi, sp.stream, *adv.pos_word + b);
        adv.picks[b] = sample_key_index(s[sample_pick_probs(p, kc, sp.top_p, u)]);
        return;
    }
    // the constraint's advance, behind the pick and before the stop check: a stop token advances the state too
    const bool constrained = con.rows && con.rows[b].con_active;
    const auto advance_constraint = [&](uint32_t token) {
        if (!constrained) return;
        const SampleConstraintRow& cr = con.rows[b];
        con.state[b] = constraint_advance(cr.next, cr.n_classes, cr.class_of, con.state[b], token);
    };
    if (!adv.state) {
        if (kc == 0) { // the state allows no token
            adv.out[0] = -1;
            return;
        }
        const float u = sample_uniform(sp.seed_lo, sp.seed_hi, sp.stream, adv.position);
        const uint32_t next = sample_key_index(s[sample_pick_probs(p, kc, sp.top_p, u)]);
        adv.out[0] = (int64_t)next;
        advance_constraint(next);
        return;
    }
    if (adv.n_seqs == 0) { // argmax_stage2's advance; state[3]: a stop token was emitted, the sequence is frozen
        uint32_t* const st = adv.state;
        if (st[3]) return;
        if (kc == 0) { // the state allows no token: frozen as behind a stop token, nothing produced, the state stays
            st[3] = 1;
            return;
        }
        const float u = sample_uniform(sp.seed_lo, sp.seed_hi, sp.stream, st[1]);
        const uint32_t next = sample_key_index(s[sample_pick_probs(p, kc, sp.top_p, u)]);
        const uint32_t produced = st[2];
        if (produced < adv.cap) adv.tokens[produced] = (int64_t)next;
        st[0] = next;
        st[1] += 1;
        st[2] = produced + 1;
        advance_constraint(next);
        if (sample_is_stop(next, sp.n_stop, sp.stop)) st[3] = 1;
        return;
    }
    // argmax_batch_stage2's advance: only while the sequence has steps left (else it repeats the same token at the same position)
    uint32_t* const st = adv.state;
    const uint32_t B = adv.n_seqs;
    const uint32_t left = st[2 * B + b], produced = st[3 * B + b], cap = st[4 * B];
    if (left == 0) return;
    if (kc == 0) { // the state allows no token: no steps left, nothing produced
        st[2 * B + b] = 0;
        return;
    }
    const float u = sample_uniform(sp.seed_lo, sp.seed_hi, sp.stream, st[B + b]);
    const uint32_t next = sample_key_index(s[sample_pick_probs(p, kc, sp.top_p, u)]);
    if (produced < cap) adv.tokens[(uint64_t)b * cap + produced] = (int64_t)next;
    st[b] = next;
    st[B + b] += 1;
    advance_constraint(next);
    st[2 * B + b] = sample_is_stop(next, sp.n_stop, sp.stop) ? 0 : left - 1;
    st[3 * B + b] = produced + 1;
}

} // namespace

void launch_sample(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch, const SampleParamsDev* params, const SampleAdvance& adv) {
    if (!n || n > 0xFFFFFFFFull || !rows) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    const uint32_t len = (uint32_t)((n + slices - 1) / slices);
    uint32_t P = kSampleMaxK;
    while (P < slices * kSampleMaxK) P <<= 1;
    sample_select_kernel<<<dim3(slices, rows), kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch);
    sample_merge_pick_kernel<<<dim3(1, rows), kMergeBlock, 0, s>>>(scratch, (uint32_t)n, slices, P, params, adv, SampleConstraint{});
}

void launch_sample_select(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch) {
    if (!n || n > 0xFFFFFFFFull || !rows) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    sample_select_kernel<<<dim3(slices, rows), kSelBlock, 0, s>>>(v, (uint32_t)n, sample_slice_len(n), scratch);
}

void launch_sample_penalized(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch, const SampleParamsDev* params,
                             const SampleAdvance& adv, const SampleWindow& win) {
    if (!n || n > 0xFFFFFFFFull || !rows) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    const uint32_t len = (uint32_t)((n + slices - 1) / slices);
    uint32_t P = kSampleMaxK;
    while (P < slices * kSampleMaxK) P <<= 1;
    sample_select_penalized_kernel<<<dim3(slices, rows), kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch, params, adv, win);
    sample_merge_pick_kernel<<<dim3(1, rows), kMergeBlock, 0, s>>>(scratch, (uint32_t)n, slices, P, params, adv, SampleConstraint{});
}

void launch_sample_constrained(hipStream_t s, const float* v, uint64_t n, uint32_t rows, uint64_t* scratch, const SampleParamsDev* params,
                               const SampleAdvance& adv, const SampleWindow& win, const SampleConstraint& con) {
    if (!n || n > 0xFFFFFFFFull || !rows || adv.picks || !con.rows || !con.state) return; // (the callers refuse these)
    const uint32_t slices = sample_slices(n);
    const uint32_t len = (uint32_t)((n + slices - 1) / slices);
    uint32_t P = kSampleMaxK;
    while (P < slices * kSampleMaxK) P <<= 1;
    sample_select_constrained_kernel<<<dim3(slices, rows), kSelBlock, 0, s>>>(v, (uint32_t)n, len, scratch, params, adv, win, con);
    sample_merge_pick_kernel<<<dim3(1, rows), kMergeBlock, 0, s>>>(scratch, (uint32_t)n, slices, P, params, adv, con);
}

} // namespace zgml
