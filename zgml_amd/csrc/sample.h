// sample.h — the rule of seeded top-k / top-p sampling and of the log-probabilities (zgml_hip_sample, zgml_hip_logprobs,
// zgml_hip_resident_decode_sampled, _batch_sampled; include/zgml_hip.h), written ONCE: the kernels of sample.hip, logprob.hip and
// top_logprob.hip call these functions and so do the host probes tests/cpp/sample_probe.cpp, logprob_probe.cpp and
// top_logprob_probe.cpp (tests/test_sample_host.py, tests/test_logprob_host.py and tests/test_top_logprob_host.py compare them with
// float64 numpy models of the same rule). Plain C++, no device intrinsics: the
// header compiles under g++ as it stands. Both sides must be built with -ffp-contract=off: every
// operation below is then one correctly rounded IEEE operation or an explicit fmaf, and device and host agree to the bit.
//
// THE CANDIDATES. A logit v at vocabulary index i has the 64-bit key (ordered(v + 0.0f) << 32) | (0xFFFFFFFF - i): `ordered` is
// the monotone float -> u32 map, + 0.0f makes -0 equal +0 (as the argmax's `>` does), a NaN counts as -inf. The candidates are
// the k = min(top_k, n) largest keys, descending: value descending, the lower index first among equals. Keys are unique, so the
// list does not depend on how a search for it is parallelised. top_k is 1..256 (0 = 256).
//   DEVIATION from textbook nucleus sampling, the one deliberate one: the candidate set never exceeds the 256 largest logits,
//   also when top_p alone would admit more of them.
//
// THE PICK, sequential and in f32 over the ordered candidates v_0 >= v_1 >= ...: p_j = sample_exp((v_j - v_0) * inv_temperature),
// total = the left-to-right sum; top_p < 1: m = the smallest prefix whose running sum is >= top_p * total, else m = k; the token
// is the first j < m whose running sum is > u * cum_m (cum_m: the running sum of the m), falling back to m - 1.
// inv_temperature = 1.0f / temperature is computed once, on the host.
//   expf / __expf may NOT be used for p_j: the host's libm and the device's expansion differ in the last bits, and one differing
//   bit in a running sum can move the pick to the neighbouring token. sample_exp is this header's own.
//
// THE RANDOM NUMBER. Philox4x32-10, key (seed low word, seed high word), counter (position, stream, 0, 0), where `position` is
// the position whose logits are sampled; u = (word 0 >> 8) * 2^-24 in [0, 1). u depends on (seed, stream, position) alone: a
// generation is the same in one call or several, alone or inside a batch.
//
// THE PENALTIES (repetition, presence, frequency; off unless zgml_sampling says otherwise). The pick at position P — over the
// logits produced by feeding the token at P — sees the tokens at positions max(lo, P + 1 - W) .. P: W = penalty_window
// (1 .. kSamplePenaltyMaxWindow), lo the first position whose token the call knows. count(t) is the number of occurrences of
// token t among them. A logit v of a token with count c > 0 becomes sample_penalize(v, c, ...):
//   v1 = v > 0 ? v * inv_repeat : v * repeat;  v2 = v1 - (float)c * frequency;  v3 = v2 - presence
// — three or four rounded f32 operations —, a logit of a token with count 0 stays as it is to the bit. The candidates, the pick
// and the random number are then exactly the ones above, computed over the penalised values: penalties come before the
// selection (a penalised token may leave the 256 largest, an encouraged one may enter them from below) and before the
// temperature, and the index in a key stays the token's index.
//   DEVIATION from llama.cpp's sampler, the one deliberate one, in the last bit: a positive logit is MULTIPLIED by
//   inv_repeat = 1.0f / repeat, computed once on the host as inv_temperature is, where llama.cpp divides by repeat. Host and
//   device therefore cannot disagree about a division.
// A NaN or an infinity passes through these operations as IEEE says; sample_ordered then maps a NaN to -inf as ever.
//
// THE LOG-PROBABILITY of token t under a row of n logits (zgml_hip_logprobs, the `logprobs` field of zgml_sampling; kernels:
// logprob.hip): log softmax(row)[t] over the WHOLE row and over the RAW logits — before penalties, before the temperature, whatever
// top_k / top_p say: the model's own distribution, independent of how the token was picked. A logit reads as logprob_value(v) =
// v + 0.0f with a NaN as -inf (sample_ordered's convention: -0 is +0). expf, logf and a free-order sum differ between host and
// device in the last bits, so the functions (sample_exp, sample_log) and the ORDER of every sum are part of the rule:
//   blocks:  the row is cut into blocks of kLogprobBlock = 4096 consecutive logits, the last one possibly short. m_b = the block's
//            largest value (exact, order-free). The block has 1024 accumulators: accumulator j sums sample_exp(v_i - m_b) over the
//            block's elements i (counted from the block's start) with i mod 1024 == j, ascending i, starting from 0.0f; an element
//            behind the row's end adds nothing (all terms are >= +0, so adding +0 for it changes no bit). The four accumulators
//            4l .. 4l + 3 of "thread" l are added left to right, and the 256 thread sums are folded by p[l] += p[l + h] for
//            h = 128, 64, .., 1: s_b = p[0]. (The layout is what lets a workgroup of 256 threads read the block once, thread l its
//            k-th 16 bytes at element 1024 k + 4 l, and fold in LDS or with wave shuffles over the same pairs.)
//   finish:  M = max_b m_b;  S = the sum over b ascending, from 0.0f, of s_b * sample_exp(m_b - M);
//            logprob(t) = (v_t - M) - sample_log(S).
//   edges:   M = -inf (no logit above -inf): -inf for every token.  M = +inf: the quiet NaN 0x7FC00000 for every token.  v_t = -inf
//            (or NaN) under a finite M: -inf.  n = 1 with a finite logit: +0.0f (v - v = +0, S = 1, sample_log(1) = +0).
// n is at most kLogprobMaxBlocks blocks = 2^20 logits. Against v_t - logsumexp(v) in float64 the error is at most
// 1e-5 + 2.4e-7 |v_t - M| (the bar of tests/test_logprob_host.py, derived there; measured maximum: 4.5e-7 + the second term).
//
// THE ALTERNATIVES of a row of n logits for a count a (the `top_logprobs` word of zgml_sampling, zgml_hip_top_logprobs; kernel:
// top_logprob.hip): a_eff = min(a, kTopLogprobsMax, n) entries (token_j, value_j), the a_eff largest keys sample_key(v_i, i) over the
// RAW row — before penalties, before the temperature, whatever top_k / top_p say —, descending: the candidate order above.
// token_j = sample_key_index(key_j); value_j = logprob_of(sample_key_value(key_j), M, S) with the row's M and S of the
// log-probability rule. sample_key_value(sample_key(v, i)) is logprob_value(v), so value_j is the log-probability of token_j over
// the same row, to the bit, and entry 0 is the row's first maximum. M = -inf: every value is -inf and the tokens are 0, 1, 2, ..
// (all keys carry the same value word, the lower index first). M = +inf: every value is the quiet NaN, the tokens still the key
// order. Entries a_eff .. of a row hold token -1 and the quiet NaN.
//
// THE CONSTRAINT (zgml_token_dfa, zgml_hip_program_set_constraint; kernel: sample_select_constrained_kernel, sample.hip). A token
// automaton in class-compressed form: class_of[vocab] (u16) gives every token's class in 0 .. n_classes - 1, and
// next[n_states][n_classes] (u16) the state behind a token of that class, kConstraintForbidden = 0xFFFF where the token is not
// allowed in the state; 1 <= n_states <= 65535, 1 <= n_classes <= 8192 (a state's row, 16 KiB at most, lies beside the select sort
// in LDS). A token that is not allowed in the row's current state IS NOT A CANDIDATE AT ALL: its key becomes the pad 0 — not the
// key of -inf, which has p = 0 and still occupies a rank that the m - 1 fall-back of sample_pick_probs could return. The
// candidates are the k = min(top_k, number of allowed tokens) largest keys among the allowed ones (sample_real_keys counts them in
// the merged list); the pick and u are unchanged. An allowed token whose logit is -inf or a NaN stays a candidate with p = 0.
// Penalties apply to the allowed tokens exactly as above; a masked key is gone, so the order of mask and penalty cannot matter.
// Behind a pick the state becomes next[state][class_of[token]] (constraint_advance) — stop tokens advance it too. A state that
// allows no token produces nothing: the loops freeze the sequence as behind a stop token, count no token and leave the state;
// zgml_hip_sample returns -1. Log-probabilities and alternatives stay what they are above: over the RAW row.
// In a verify step (zgml_hip_resident_decode_speculative_constrained) every logits ROW has a state of its own — the one reached by
// walking the step's candidates — and is masked by it exactly as above; a state that allows exactly one token FORCES it
// (forced[], below), which the draft rule uses. The pass, the rows without a pick and the state's advance: spec.h, UNDER A CONSTRAINT.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZGML_SAMPLE_FN __host__ __device__ inline
#else
#define ZGML_SAMPLE_FN inline
#endif

namespace zgml {

constexpr uint32_t kSampleMaxK = 256;   // the candidate set's upper bound
constexpr uint32_t kSampleMaxStop = 4;  // stop tokens per sequence
constexpr uint32_t kSamplePenaltyMaxWindow = 256; // positions a penalty looks back over, the sampled one included

ZGML_SAMPLE_FN uint32_t sample_f32_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}
ZGML_SAMPLE_FN float sample_bits_f32(uint32_t b) {
    float v;
    memcpy(&v, &b, 4);
    return v;
}

// monotone float -> u32: a < b  <=>  ordered(a) < ordered(b); -0 and +0 map to one word, a NaN to -inf's
ZGML_SAMPLE_FN uint32_t sample_ordered(float v) {
    v = v + 0.0f;
    if (v != v) v = -INFINITY;
    const uint32_t b = sample_f32_bits(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ZGML_SAMPLE_FN uint64_t sample_key(float v, uint32_t i) { return ((uint64_t)sample_ordered(v) << 32) | (uint64_t)(0xFFFFFFFFu - i); }
// (every key of a logit is > 0 — ordered(-inf) is 0x007FFFFF — so 0 pads a list below all of them)
ZGML_SAMPLE_FN float sample_key_value(uint64_t key) {
    const uint32_t o = (uint32_t)(key >> 32);
    return sample_bits_f32((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
ZGML_SAMPLE_FN uint32_t sample_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// the number of candidates of a row of n logits
ZGML_SAMPLE_FN uint32_t sample_top_k(uint32_t top_k, uint64_t n) {
    const uint32_t k = top_k == 0 || top_k > kSampleMaxK ? kSampleMaxK : top_k;
    return n < k ? (uint32_t)n : k;
}

// e^x for x <= 0: n = rint(x / ln 2), r = x - n ln 2 (ln 2 in two parts, two fmaf), a degree-6 Horner polynomial in explicit
// fmaf, ldexpf. Arguments below -87 (and a NaN) give 0: the smallest result is e^-87 = 1.40 * 2^-126, so no denormal is ever
// produced. Maximum relative error against exp in float64: 1.9e-7 on [-80, 0].
ZGML_SAMPLE_FN float sample_exp(float x) {
    if (!(x >= -87.0f)) return 0.0f;
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);
    r = fmaf(n, -1.42860682030941723e-6f, r);
    float p = 1.0f / 720.0f;
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return ldexpf(p, (int)n);
}

// the unnormalised probability of a candidate of value v under the largest candidate v0
ZGML_SAMPLE_FN float sample_prob(float v, float v0, float inv_temperature) { return sample_exp((v - v0) * inv_temperature); }

// the pick over p[0..k): the candidate's rank j. (The kernel fills p with all its threads — sample_prob is a pure function — and
// walks this alone; the probe does both alone.)
ZGML_SAMPLE_FN uint32_t sample_pick_probs(const float* p, uint32_t k, float top_p, float u) {
    float total = 0.0f;
    for (uint32_t j = 0; j < k; j++) total = total + p[j];
    uint32_t m = k;
    float cum = total;
    if (top_p < 1.0f) {
        const float thr = top_p * total;
        float run = 0.0f;
        for (uint32_t j = 0; j < k; j++) {
            run = run + p[j];
            if (run >= thr) {
                m = j + 1, cum = run;
                break;
            }
        }
    }
    const float t = u * cum;
    float run = 0.0f;
    for (uint32_t j = 0; j < m; j++) {
        run = run + p[j];
        if (run > t) return j;
    }
    return m - 1;
}

// ... from the ordered candidate keys (k >= 1, k <= kSampleMaxK)
ZGML_SAMPLE_FN uint32_t sample_pick(const uint64_t* keys, uint32_t k, float inv_temperature, float top_p, float u) {
    float p[kSampleMaxK];
    const float v0 = sample_key_value(keys[0]);
    for (uint32_t j = 0; j < k; j++) p[j] = sample_prob(sample_key_value(keys[j]), v0, inv_temperature);
    return sample_pick_probs(p, k, top_p, u);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
ZGML_SAMPLE_FN void sample_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; round++) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)m1, c3 = (uint32_t)m0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

ZGML_SAMPLE_FN float sample_u_of_word(uint32_t word0) { return (float)(word0 >> 8) * 5.9604644775390625e-8f; } // 2^-24: exact

ZGML_SAMPLE_FN float sample_uniform(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t position) {
    const uint32_t ctr[4] = {position, stream, 0, 0}, key[2] = {seed_lo, seed_hi};
    uint32_t w[4];
    sample_philox4x32_10(ctr, key, w);
    return sample_u_of_word(w[0]);
}

ZGML_SAMPLE_FN bool sample_is_stop(uint32_t token, uint32_t n_stop, const uint32_t* stop) {
    for (uint32_t i = 0; i < n_stop && i < kSampleMaxStop; i++)
        if (stop[i] == token) return true;
    return false;
}

// ── the penalties ──

// the logit v of a token that occurs `count` times in the window (inv_repeat = 1.0f / repeat, from the host)
ZGML_SAMPLE_FN float sample_penalize(float v, uint32_t count, float repeat, float inv_repeat, float presence, float frequency) {
    if (count == 0) return v;
    const float v1 = v > 0.0f ? v * inv_repeat : v * repeat;
    const float v2 = v1 - (float)count * frequency;
    return v2 - presence;
}

// Entry i of the window win[0, m), m <= kSamplePenaltyMaxWindow: 0 when the token occurred at an earlier entry, else the number
// of its occurrences in the window. The entries with a result > 0 are the window's distinct tokens, each once, with count(t).
// O(m) per entry, O(m^2) for a window: the kernel gives every entry a thread, the probe walks them.
ZGML_SAMPLE_FN uint32_t sample_window_count(const uint32_t* win, uint32_t m, uint32_t i) {
    const uint32_t t = win[i];
    uint32_t c = 0;
    for (uint32_t j = 0; j < m; j++) {
        if (win[j] != t) continue;
        if (j < i) return 0;
        c++;
    }
    return c;
}

// the window of the pick at `position`: its first position and (the return value) its length. lo > position: nothing is known
ZGML_SAMPLE_FN uint32_t sample_window_span(uint32_t position, uint32_t lo, uint32_t window, uint32_t* first) {
    *first = position;
    if (lo > position) return 0;
    const uint32_t known = position - lo + 1;
    const uint32_t m = known < window ? known : window;
    *first = position + 1 - m;
    return m;
}

// ── the log-probability ──

constexpr uint32_t kLogprobBlock = 4096;    // logits per block
constexpr uint32_t kLogprobThreads = 256;   // "threads" of a block: four accumulators each, 16 elements each
constexpr uint32_t kLogprobMaxBlocks = 256; // blocks per row: n <= 2^20
constexpr uint64_t kLogprobMaxN = (uint64_t)kLogprobBlock * kLogprobMaxBlocks;
constexpr uint32_t kLogprobNaNBits = 0x7FC00000u; // M = +inf, and what an entry of a token that was not produced holds
static_assert(kLogprobBlock == 16 * kLogprobThreads, "a thread reads four times four consecutive elements");

ZGML_SAMPLE_FN uint32_t logprob_blocks(uint64_t n) { return (uint32_t)((n + kLogprobBlock - 1) / kLogprobBlock); }

// ln x for x in [2^-1, 2^32) — all the rule needs: S >= 1, a sum of at most 2^20 terms <= 1 —: frexpf, the mantissa moved to
// [sqrt 1/2, sqrt 2), t = f - 1 (exact), t - t^2 / 2 + t^3 P(t) with the degree-8 P of Cephes' logf as a Horner chain of explicit
// fmaf, the exponent's e ln 2 in two parts (0.693359375 is exact in 11 bits: e times it is exact). sample_log(1) = +0.
// Maximum error against log in float64 on [0.5, 2^32): 7.9e-8 relative where |ln x| >= 1, 4.5e-8 absolute below.
ZGML_SAMPLE_FN float sample_log(float x) {
    int e;
    float f = frexpf(x, &e);
    if (f < 0.707106781186547524f) f = f + f, e -= 1;
    const float t = f - 1.0f, z = t * t, fe = (float)e;
    float p = 7.0376836292e-2f;
    p = fmaf(p, t, -1.1514610310e-1f);
    p = fmaf(p, t, 1.1676998740e-1f);
    p = fmaf(p, t, -1.2420140846e-1f);
    p = fmaf(p, t, 1.4249322787e-1f);
    p = fmaf(p, t, -1.6668057665e-1f);
    p = fmaf(p, t, 2.0000714765e-1f);
    p = fmaf(p, t, -2.4999993993e-1f);
    p = fmaf(p, t, 3.3333331174e-1f);
    float y = (t * z) * p;
    y = fmaf(fe, -2.12194440e-4f, y);
    y = fmaf(-0.5f, z, y);
    return fmaf(fe, 0.693359375f, t + y);
}

// a logit as the rule reads it: -0 is +0, a NaN is -inf
ZGML_SAMPLE_FN float logprob_value(float v) {
    v = v + 0.0f;
    return v != v ? -INFINITY : v;
}

// one element's term under its block's maximum (m = +-inf: the difference is a NaN or -inf, the term 0)
ZGML_SAMPLE_FN float logprob_term(float v, float m) { return sample_exp(logprob_value(v) - m); }

// a thread's sum of its four accumulators
ZGML_SAMPLE_FN float logprob_thread_sum(const float acc[4]) { return ((acc[0] + acc[1]) + acc[2]) + acc[3]; }

// (m_b, s_b) of the block v[0, len), len <= kLogprobBlock, walked alone (the probe; the kernel gives every "thread" a thread)
ZGML_SAMPLE_FN void logprob_block(const float* v, uint32_t len, float* m_out, float* s_out) {
    float m = -INFINITY;
    for (uint32_t i = 0; i < len; i++) {
        const float x = logprob_value(v[i]);
        if (x > m) m = x;
    }
    float p[kLogprobThreads];
    for (uint32_t l = 0; l < kLogprobThreads; l++) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < 4; k++)
            for (uint32_t c = 0; c < 4; c++) {
                const uint32_t i = k * (4 * kLogprobThreads) + 4 * l + c;
                if (i < len) acc[c] = acc[c] + logprob_term(v[i], m);
            }
        p[l] = logprob_thread_sum(acc);
    }
    for (uint32_t h = kLogprobThreads / 2; h > 0; h >>= 1)
        for (uint32_t l = 0; l < h; l++) p[l] = p[l] + p[l + h];
    *m_out = m, *s_out = p[0];
}

// block b's share of S under the row's maximum M
ZGML_SAMPLE_FN float logprob_block_term(float m_b, float s_b, float M) { return s_b * sample_exp(m_b - M); }

// the value from the row's M and S and the token's logit
ZGML_SAMPLE_FN float logprob_of(float v_t, float M, float S) {
    if (M == -INFINITY) return -INFINITY;
    if (M == INFINITY) return sample_bits_f32(kLogprobNaNBits);
    return (logprob_value(v_t) - M) - sample_log(S);
}

// the finish over the nb block pairs: M and S
ZGML_SAMPLE_FN void logprob_finish(const float* m, const float* s, uint32_t nb, float* M_out, float* S_out) {
    float M = -INFINITY, S = 0.0f;
    for (uint32_t b = 0; b < nb; b++)
        if (m[b] > M) M = m[b];
    for (uint32_t b = 0; b < nb; b++) S = S + logprob_block_term(m[b], s[b], M);
    *M_out = M, *S_out = S;
}

// ── the alternatives ──

constexpr uint32_t kTopLogprobsMax = 64; // alternatives per row

// How the select launch cuts a row (sample.hip): sample_slices(n) slices of ceil(n / slices) consecutive logits, a sorted list of
// the 256 largest keys each
constexpr uint32_t kSampleMaxSlices = 32; // partial candidate lists per row
constexpr uint32_t kSampleChunk = 1792;   // logits a select workgroup sorts at a time (with the 256 best so far: 2048 keys)
ZGML_SAMPLE_FN uint32_t sample_slices(uint64_t n) {
    const uint64_t s = (n + kSampleChunk - 1) / kSampleChunk;
    return s < 1 ? 1u : s > kSampleMaxSlices ? kSampleMaxSlices : (uint32_t)s;
}
ZGML_SAMPLE_FN uint32_t sample_slice_len(uint64_t n) {
    const uint32_t slices = sample_slices(n);
    return (uint32_t)((n + slices - 1) / slices);
}

// a_eff
ZGML_SAMPLE_FN uint32_t top_logprobs_count(uint32_t a, uint64_t n) {
    const uint32_t c = a > kTopLogprobsMax ? kTopLogprobsMax : a;
    return n < c ? (uint32_t)n : c;
}

// the `cap` (<= kTopLogprobsMax) largest keys of v[lo, hi), descending, into out[0, cap), 0 behind the last of fewer: the walk
// keeps the best so far sorted and inserts every key above the last of them
ZGML_SAMPLE_FN void top_logprobs_walk(const float* v, uint64_t lo, uint64_t hi, uint32_t cap, uint64_t* out) {
    for (uint32_t j = 0; j < cap; j++) out[j] = 0;
    if (!cap) return;
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t key = sample_key(v[i], (uint32_t)i);
        if (key <= out[cap - 1]) continue;
        uint32_t j = cap - 1;
        for (; j > 0 && out[j - 1] < key; j--) out[j] = out[j - 1];
        out[j] = key;
    }
}

// the direct form: the a_eff largest keys of the row; returns a_eff
ZGML_SAMPLE_FN uint32_t top_logprobs_keys(const float* v, uint64_t n, uint32_t a, uint64_t* keys) {
    const uint32_t ae = top_logprobs_count(a, n);
    top_logprobs_walk(v, 0, n, ae, keys);
    return ae;
}

// The sliced form, what the kernel evaluates. heads: `slices` (<= kSampleMaxSlices) lists of kTopLogprobsMax keys — list l the FIRST
// 64 keys of the sorted list of slice l, 0 behind the last of a shorter slice. The a_eff largest of all heads, descending, go
// to keys[0, a_eff).
//   Why the heads are enough: let x be one of the row's 64 largest keys and l its slice. Every key of slice l above x is a key of
//   the row above x, and there are at most 63 of those: x is among the first 64 keys of list l. So the row's 64 largest keys all
//   lie in the heads, they are the 64 largest keys there (the heads hold keys of the row and pads 0, which lie below every
//   key), and a_eff <= 64 of them are what the direct form finds. Keys are unique: the merge's order of work cannot matter.
ZGML_SAMPLE_FN uint32_t top_logprobs_merge(const uint64_t* heads, uint32_t slices, uint64_t n, uint32_t a, uint64_t* keys) {
    const uint32_t ae = top_logprobs_count(a, n);
    uint32_t at[kSampleMaxSlices];
    for (uint32_t l = 0; l < slices; l++) at[l] = 0;
    for (uint32_t j = 0; j < ae; j++) {
        uint64_t best = 0;
        uint32_t from = 0;
        for (uint32_t l = 0; l < slices; l++)
            if (at[l] < kTopLogprobsMax && heads[l * kTopLogprobsMax + at[l]] > best) best = heads[l * kTopLogprobsMax + at[l]], from = l;
        keys[j] = best, at[from] += 1; // (best > 0: the heads hold at least min(64, n) keys of the row)
    }
    return ae;
}

// ... over a row cut into `slices` (<= kSampleMaxSlices) slices of `len` logits, slices * len >= n: the heads, then the merge
ZGML_SAMPLE_FN uint32_t top_logprobs_keys_cut(const float* v, uint64_t n, uint32_t a, uint32_t slices, uint32_t len, uint64_t* keys, uint64_t* heads /* [32 * 64] */) {
    for (uint32_t l = 0; l < slices; l++) {
        const uint64_t lo = (uint64_t)l * len, hi = lo + len < n ? lo + len : n;
        top_logprobs_walk(v, lo < n ? lo : n, hi, kTopLogprobsMax, heads + l * kTopLogprobsMax); // (lo may lie behind n: an empty slice, all pads)
    }
    return top_logprobs_merge(heads, slices, n, a, keys);
}

// ... as the select launch cuts it
ZGML_SAMPLE_FN uint32_t top_logprobs_keys_sliced(const float* v, uint64_t n, uint32_t a, uint64_t* keys, uint64_t* heads /* [32 * 64] */) {
    return top_logprobs_keys_cut(v, n, a, sample_slices(n), sample_slice_len(n), keys, heads);
}

// entry j of a row from its key: the token and its value under the row's M and S
ZGML_SAMPLE_FN void top_logprobs_entry(uint64_t key, float M, float S, uint32_t* token, float* value) {
    *token = sample_key_index(key);
    *value = logprob_of(sample_key_value(key), M, S);
}

// ── the constraint ──

constexpr uint32_t kConstraintMaxStates = 65535;  // states are u16 words, 0xFFFF is taken
constexpr uint32_t kConstraintMaxClasses = 8192;  // a state's row beside the select sort in LDS: 16 KiB
constexpr uint16_t kConstraintForbidden = 0xFFFF; // next[state][class]: the token is not allowed

// is `token` allowed in the state whose row of the table — next + state * n_classes — is `row`?
// (the test over a class already read: the select kernel reads class_of through a pointer typed for global memory)
ZGML_SAMPLE_FN bool constraint_row_allows(const uint16_t* row, uint16_t cls) { return row[cls] != kConstraintForbidden; }
ZGML_SAMPLE_FN bool constraint_allowed(const uint16_t* row, const uint16_t* class_of, uint32_t token) { return constraint_row_allows(row, class_of[token]); }

// the state behind `token` (an allowed one: else kConstraintForbidden comes back)
ZGML_SAMPLE_FN uint32_t constraint_advance(const uint16_t* next, uint32_t n_classes, const uint16_t* class_of, uint32_t state, uint32_t token) {
    return next[(uint64_t)state * n_classes + class_of[token]];
}

// ── the constraint under speculation (zgml_hip_resident_decode_speculative_constrained; the pass over a step's candidates is spec.h's) ──
// A state that allows EXACTLY ONE token of the vocabulary forces it: forced[state] is that token, kConstraintNoForced otherwise
// (no token, or two and more). A verify row whose state cannot be reached — a candidate in front of it is not allowed — is
// dead: its state is kConstraintDead, it has no candidates and therefore no pick.
constexpr uint32_t kConstraintNoForced = 0xFFFFFFFFu;
constexpr uint32_t kConstraintDead = kConstraintForbidden; // what constraint_advance gives for a token that is not allowed

// forced[] of one state from the per-class token counts: count[c] tokens have class c, first[c] is the lowest of them. A class
// without tokens counts as nothing, so one allowed singleton class beside allowed empty classes still forces. O(n_classes).
ZGML_SAMPLE_FN uint32_t constraint_forced_of(const uint16_t* row, uint32_t n_classes, const uint32_t* count, const uint32_t* first) {
    uint32_t allowed = 0, token = kConstraintNoForced;
    for (uint32_t c = 0; c < n_classes; c++) {
        if (!constraint_row_allows(row, (uint16_t)c) || count[c] == 0) continue;
        allowed += count[c] > 1 ? 2 : 1; // (saturating: only 0, 1 and "more" matter)
        if (allowed > 1) return kConstraintNoForced;
        token = first[c];
    }
    return token;
}

// The number of real (non-zero) keys among the first k0 of a descending list whose pads 0 lie behind every key: the k of a row.
// A row without a constraint has n >= k0 real keys, so the result is k0 and nothing changes for it to the bit.
ZGML_SAMPLE_FN uint32_t sample_real_keys(const uint64_t* keys, uint32_t k0) {
    uint32_t lo = 0, hi = k0;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] != 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

} // namespace zgml
