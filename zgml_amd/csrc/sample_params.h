// sample_params.h — what include/zgml_hip.h refuses of the penalty fields and of the `logprobs` field of a zgml_sampling, and of the
// arguments of zgml_hip_logprobs and zgml_hip_top_logprobs, of a zgml_token_dfa and its attachment, and how the `top_logprobs`
// word is read, as pure host logic: the runtime (runtime_resident.hip) and the CPU probes tests/cpp/penalty_probe.cpp,
// tests/cpp/logprob_probe.cpp, tests/cpp/top_logprob_probe.cpp and tests/cpp/constraint_probe.cpp compile these functions.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sample.h"
#include "zgml_hip.h"

namespace zgml {

// The penalty fields of a zgml_sampling against the header's list of refusals: nullptr, or why the call is refused. form: 0
// zgml_hip_sample, 1 the single and the batched loop (vocab and start_pos are the sequence's), 2 the verify step. *repeat: the
// factor as the rule reads it (0 means 1); *active: whether the penalised launch is needed at all.
inline const char* sample_penalty_check(const zgml_sampling* sp, int form, uint32_t vocab, uint32_t start_pos, float* repeat, uint32_t* active) {
    const float rp = sp->repeat_penalty, pp = sp->presence_penalty, fp = sp->frequency_penalty;
    if (!isfinite(rp) || !isfinite(pp) || !isfinite(fp) || rp < 0.0f) return "the penalties must be finite and repeat_penalty not negative";
    if (sp->penalty_window > kSamplePenaltyMaxWindow) return "penalty_window must be at most 256";
    const bool neutral = (rp == 0.0f || rp == 1.0f) && pp == 0.0f && fp == 0.0f;
    if (!neutral && sp->penalty_window == 0) return "a penalty that is not neutral needs penalty_window > 0";
    if (!sp->recent && sp->n_recent) return "n_recent > 0 without the recent tokens";
    if (form == 2 && sp->recent) return "recent must be NULL (the tokens before a speculative call are opt->history)";
    if (form == 1) {
        if (sp->n_recent > start_pos) return "n_recent exceeds start_pos";
        for (uint32_t i = 0; i < sp->n_recent; i++)
            if (sp->recent[i] >= vocab) return "recent token out of range";
    }
    *repeat = rp == 0.0f ? 1.0f : rp;
    *active = !neutral && sp->penalty_window > 0;
    return nullptr;
}

// What zgml_hip_logprobs refuses: nullptr, or why. buf_size: the elements of the buffer, 0 for one that does not exist.
inline const char* logprobs_check(uint64_t buf_size, uint64_t offset, uint64_t n, uint32_t rows, const uint32_t* tokens, const float* out) {
    if (!tokens || !out) return "tokens and logprobs_out must not be NULL";
    if (!n || n > kLogprobMaxN) return "a row must hold 1 .. 2^20 elements";
    if (!rows) return "rows must be at least 1";
    if (!buf_size || offset > buf_size || n * (uint64_t)rows > buf_size - offset) return "the rows must lie inside the buffer";
    for (uint32_t i = 0; i < rows; i++)
        if (tokens[i] >= n) return "token out of range";
    return nullptr;
}

// ... and what the `logprobs` word of a zgml_sampling asks of the row length of the entry point it is handed to
inline const char* sample_logprobs_check(const zgml_sampling* sp, uint64_t n) {
    if (sp->logprobs && n > kLogprobMaxN) return "logprobs needs a row of at most 2^20 elements";
    return nullptr;
}

// the `top_logprobs` word as the kernels read it: only with `logprobs` set, and a value above kTopLogprobsMax as that — the word
// was padding before, so it is clamped, never refused
inline uint32_t sample_top_logprobs(const zgml_sampling* sp) {
    if (!sp->logprobs) return 0;
    return sp->top_logprobs > kTopLogprobsMax ? kTopLogprobsMax : sp->top_logprobs;
}

// What zgml_hip_top_logprobs refuses: everything logprobs_check refuses of n, rows, the range and NULL pointers, and — a new
// argument, so refused, not clamped — top_n outside 1 .. kTopLogprobsMax
inline const char* top_logprobs_check(uint64_t buf_size, uint64_t offset, uint64_t n, uint32_t rows, uint32_t top_n, const int64_t* tokens_out, const float* out) {
    if (!tokens_out || !out) return "tokens_out and logprobs_out must not be NULL";
    if (!n || n > kLogprobMaxN) return "a row must hold 1 .. 2^20 elements";
    if (!rows) return "rows must be at least 1";
    if (!buf_size || offset > buf_size || n * (uint64_t)rows > buf_size - offset) return "the rows must lie inside the buffer";
    if (!top_n || top_n > kTopLogprobsMax) return "top_n must be 1 .. 64";
    return nullptr;
}

// What zgml_hip_constraint_create refuses of a zgml_token_dfa (include/zgml_hip.h), before anything is uploaded: nullptr, or why
inline const char* constraint_check(const zgml_token_dfa* d) {
    if (!d || !d->class_of || !d->next) return "the automaton and its two tables must not be NULL";
    if (d->n_states < 1 || d->n_states > kConstraintMaxStates) return "n_states must be 1 .. 65535";
    if (d->n_classes < 1 || d->n_classes > kConstraintMaxClasses) return "n_classes must be 1 .. 8192";
    if (d->vocab < 1) return "vocab must be at least 1";
    for (uint32_t i = 0; i < d->vocab; i++)
        if (d->class_of[i] >= d->n_classes) return "a class is not below n_classes";
    for (uint64_t i = 0; i < (uint64_t)d->n_states * d->n_classes; i++)
        if (d->next[i] != kConstraintForbidden && d->next[i] >= d->n_states) return "a next state is neither below n_states nor 0xFFFF";
    return nullptr;
}

// forced[n_states] of a checked automaton (sample.h: the constraint under speculation), what zgml_hip_constraint_create uploads
// beside the two tables: one pass over class_of for the per-class counts, then constraint_forced_of per state —
// O(vocab + n_states n_classes). count, first: n_classes words of scratch each
inline void constraint_forced(const zgml_token_dfa* d, uint32_t* count, uint32_t* first, uint32_t* forced) {
    for (uint32_t c = 0; c < d->n_classes; c++) count[c] = 0, first[c] = kConstraintNoForced;
    for (uint32_t i = 0; i < d->vocab; i++) {
        const uint16_t c = d->class_of[i];
        if (count[c]++ == 0) first[c] = i;
    }
    for (uint32_t s = 0; s < d->n_states; s++) forced[s] = constraint_forced_of(d->next + (uint64_t)s * d->n_classes, d->n_classes, count, first);
}

// ... and zgml_hip_program_set_constraint of an attachment: the automaton's vocab and n_states, the program's vocab and number of
// sequences (1 for a plain plan)
inline const char* constraint_attach_check(uint32_t dfa_vocab, uint32_t dfa_states, uint32_t program_vocab, uint32_t n_seqs, uint32_t seq, uint32_t state) {
    if (seq >= n_seqs) return "seq is not below the program's number of sequences";
    if (dfa_vocab != program_vocab) return "the automaton's vocab differs from the program's";
    if (state >= dfa_states) return "state is not below n_states";
    return nullptr;
}

} // namespace zgml
