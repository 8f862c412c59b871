// spec.h — the draft rule and the acceptance rule of greedy-exact speculative decode (zgml_hip_resident_decode_speculative and
// its sampled form zgml_hip_resident_decode_speculative_sampled, include/zgml_hip.h), written ONCE: the kernels of
// spec_decode.hip call these functions and so does the host probe tests/cpp/spec_probe.cpp (tests/test_spec_decode_host.py
// compares it with a Python model of the same rules). Plain C++, no device intrinsics: the header compiles under g++ as it
// stands.
//
// Vocabulary: hist[0..pos] holds the token at every position, hist[pos] being the last confirmed token (not yet in the KV
// cache). A verify step runs a token_len = T plan over the candidates c[0..T-1]: c[0] = hist[pos], c[j] the draft for position
// pos + j (from the n-gram lookup, the caller's table, or a draft model: the three candidate rules below), or — a position
// without a draft — the pad c[j - 1]. g[j] is the token of logits row j — its first maximum, or in the
// sampled form sample.h's pick at position pos + j —: the token at position pos + j + 1 given c[0..j].
//
// UNDER A CONSTRAINT (zgml_hip_resident_decode_speculative_constrained; sample.h: THE CONSTRAINT). The mode's candidates and its
// count of real drafts are made as ever; then ONE pass (spec_constrain_candidates) walks the sequence's automaton over them and
// gives every row its state: row_state[0] = the sequence's state, and for j >= 1, with s the state of row j - 1:
//   s dead                       row j is dead, c[j] stays
//   forced[s] exists             c[j] = forced[s] — also over a real draft: a different draft is certainly wrong
//   j behind the real drafts     the pad is re-evaluated, c[j] = c[j - 1] (it may now follow a forced token)
//   then row_state[j] = next[s][class_of[c[j]]], dead when c[j] is not allowed in s.
// `drafted` grows by the mode's real drafts plus the forced tokens placed at pad positions. g[j] is sample.h's constrained pick
// under row_state[j] at position pos + j; a dead row, and a row whose state allows no token, has no pick: g[j] = kSpecNoPick,
// which equals no candidate, so spec_accept (unchanged) never walks past it. When g[acc] is kSpecNoPick the reached state allows
// no token: the emission is cut in front of it (spec_dead_end_cut) and the call is finished. The sequence's state then advances
// over exactly the emitted tokens (spec_state_advance); an idle step leaves it alone. Every emitted token is the constrained pick
// over a confirmed context at its own position and state: drafts and forced tokens change how many steps run, never the tokens.
#pragma once

#include <stdint.h>

#include "sample.h"

#if defined(__HIPCC__)
#define ZGML_SPEC_FN __host__ __device__ inline
#else
#define ZGML_SPEC_FN inline
#endif

namespace zgml {

constexpr uint32_t kSpecMaxNgram = 4; // longest suffix the lookup tries
constexpr uint32_t kSpecDefaultNgram = 2;

// does the n-gram that ends at i equal the one that ends at pos? (i - n + 1 >= 0 is the caller's business)
ZGML_SPEC_FN bool spec_ngram_equal(const uint32_t* hist, uint32_t pos, uint32_t n, uint32_t i) {
    for (uint32_t k = 0; k < n; k++)
        if (hist[i - k] != hist[pos - k]) return false;
    return true;
}

// the positions a lookup of length n may end at are [n - 1, pos - 1]; none when n > pos (and a suffix of length n does not even
// exist when n > pos + 1)
ZGML_SPEC_FN bool spec_ngram_applies(uint32_t pos, uint32_t n) { return n >= 1 && n <= pos; }

// the largest i < pos whose n-gram equals the history's last n tokens; -1: none. (The kernel splits this walk over its threads
// and keeps the largest hit; the probe walks it alone.)
ZGML_SPEC_FN int64_t spec_ngram_find(const uint32_t* hist, uint32_t pos, uint32_t n) {
    if (!spec_ngram_applies(pos, n)) return -1;
    for (uint32_t i = pos - 1;; i--) {
        if (spec_ngram_equal(hist, pos, n, i)) return i;
        if (i == n - 1) return -1;
    }
}

// n = ngram down to 1, the first n with a match wins: its match position, -1 when no n has one
ZGML_SPEC_FN int64_t spec_lookup(const uint32_t* hist, uint32_t pos, uint32_t ngram) {
    for (uint32_t n = ngram; n >= 1; n--) {
        const int64_t i = spec_ngram_find(hist, pos, n);
        if (i >= 0) return i;
    }
    return -1;
}

// the T candidates of a lookup step from the match position i (-1: none, every candidate a pad): d[k] = v[i + 1 + k] with v the
// history followed by the drafts chosen so far, so a match that overlaps the end of the history continues periodically through
// its own drafts. Returns the number of real drafts.
ZGML_SPEC_FN uint32_t spec_candidates_lookup(const uint32_t* hist, uint32_t pos, int64_t i, uint32_t T, uint32_t* c) {
    c[0] = hist[pos];
    for (uint32_t j = 1; j < T; j++) {
        if (i < 0) {
            c[j] = c[j - 1];
            continue;
        }
        const uint64_t src = (uint64_t)i + j;              // v[src]: i < pos, so src - pos < j is a candidate already chosen
        c[j] = src <= pos ? hist[src] : c[src - pos];
    }
    return i < 0 ? 0 : T - 1;
}

// ... and of a step with provided drafts: drafts[x] is the caller's guess for position start_pos + 1 + x
ZGML_SPEC_FN uint32_t spec_candidates_provided(uint32_t tok, uint32_t pos, uint32_t start_pos, const uint32_t* drafts, uint32_t n_drafts,
                                               uint32_t T, uint32_t* c) {
    uint32_t real = 0;
    c[0] = tok;
    for (uint32_t j = 1; j < T; j++) {
        const uint64_t x = (uint64_t)pos + j - start_pos - 1; // (pos >= start_pos)
        if (x < n_drafts)
            c[j] = drafts[x], real++;
        else
            c[j] = c[j - 1];
    }
    return real;
}

// ── DRAFTS FROM A MODEL (zgml_hip_resident_decode_speculative_model): a second, token_len = 1 program of the same vocabulary ──
// A verify step runs at (hist[pos], pos); c[0] = hist[pos]. For j = 0 .. T-1 the draft program executes on token c[j] at position
// pos + j — each execution stores the DRAFT's KV column pos + j —, d[j] is the first maximum of its logits row, and
// c[j + 1] = d[j] for j < T - 1. The T-th execution exists for its KV column alone and d[T - 1] is dropped: when all T - 1 drafts
// are accepted the next step starts at pos + T, and the draft must then already hold column pos + T - 1. `drafted` grows by
// T - 1 per step that is not idle; there are no pads. The drafts are the draft program's GREEDY tokens, under a sampled verify
// step too. An idle step executes the draft T times from (hist[at], at), `at` the position the target's idle step runs at:
// column `at` is rewritten from the same token and context, the columns behind it are unspecified, as the target's are.
// Why the draft's cache stays in step: with a candidates accepted, the draft's columns pos .. pos + min(a, T - 1) were computed
// over confirmed tokens — the step emits at most a + 1 —, and every column behind them is stored again, by the next step's
// executions from its own pos, before any attention of the draft reads it.
// Under batching (zgml_hip_resident_decode_batch_speculative_model) this is the rule of every sequence b of a batched target: the
// draft is a batched one-column plan of the same sequences, execution j runs sequence b on its c[j] at its pos + j, d[j] is the
// first maximum of the draft's logits ROW b. A sequence that has its count idles at its end position (kIdleAtEnd) and its draft
// from there.
// What the draft launch leaves of this rule: c[0] (the other candidates are written by the executions' advances; until then they
// repeat c[0]) and the count of drafts.
ZGML_SPEC_FN uint32_t spec_candidates_model(uint32_t tok, uint32_t T, uint32_t* c) {
    for (uint32_t j = 0; j < T; j++) c[j] = tok;
    return T - 1;
}

// the largest a with c[j] == g[j - 1] for all 1 <= j <= a: the candidates that were the greedy choice of the rows in front of them
template <class G>
ZGML_SPEC_FN uint32_t spec_accept(const uint32_t* c, const G* g, uint32_t T) {
    uint32_t a = 0;
    while (a + 1 < T && (G)c[a + 1] == g[a]) a++;
    return a;
}

// tokens a step emits (g[0..a], cut to what is still wanted); 0: nothing left, the step must change nothing
ZGML_SPEC_FN uint32_t spec_emit_count(uint32_t a, uint32_t n_tokens, uint32_t produced) {
    const uint32_t left = produced < n_tokens ? n_tokens - produced : 0;
    return a + 1 < left ? a + 1 : left;
}

// the stop cut of the sampled form: among the m tokens g[0..m-1] a step would emit, the first that is one of the n_stop stop
// tokens ends the emission behind itself. Returns the tokens emitted after the cut (m when none of them stops); *fired: one did
// — also when it is g[m - 1] and cuts nothing. A stop token behind the m is not looked at.
template <class G>
ZGML_SPEC_FN uint32_t spec_stop_cut(const G* g, uint32_t m, uint32_t n_stop, const uint32_t* stop, bool* fired) {
    *fired = false;
    for (uint32_t k = 0; k < m; k++)
        for (uint32_t i = 0; i < n_stop; i++)
            if (g[k] == (G)stop[i]) {
                *fired = true;
                return k + 1;
            }
    return m;
}

// ── under a constraint ──

constexpr uint32_t kSpecNoPick = 0xFFFFFFFFu; // g[j] of a row without candidates: >= 2^31, no token (a token is < vocab <= 2^32 - 1)

// the pass over the mode's candidates c[0..T-1] with `real` real drafts (at c[1..real]) from the sequence's state: rewrites c,
// fills row_state[0..T-1], returns the forced tokens placed at pad positions (what `drafted` grows by beside `real`)
ZGML_SPEC_FN uint32_t spec_constrain_candidates(uint32_t* c, uint32_t T, uint32_t real, uint32_t state, const uint16_t* class_of, const uint16_t* next,
                                                uint32_t n_classes, const uint32_t* forced, uint32_t* row_state) {
    uint32_t s = state, placed = 0;
    row_state[0] = s;
    for (uint32_t j = 1; j < T; j++) {
        if (s != kConstraintDead) {
            const uint32_t f = forced[s];
            if (f != kConstraintNoForced) {
                c[j] = f;
                if (j > real) placed++;
            } else if (j > real) {
                c[j] = c[j - 1];
            }
            s = constraint_advance(next, n_classes, class_of, s, c[j]);
        }
        row_state[j] = s;
    }
    return placed;
}

// Under batching (zgml_hip_resident_decode_batch_speculative_constrained) every sequence walks its OWN automaton, and a sequence
// without one may sit beside sequences with one, in the same launches. Its rows are FREE: the pass leaves its candidates alone,
// places nothing, and gives every row the state kSpecRowFree — no state of any automaton (those are < 0xFFFF) and not dead —,
// so the rows select as the rows of the sampled form do and every one of them has a pick. What the select launch asks of a row's
// state word, whatever its sequence: spec_row_selects — a dead row has no candidates, every other row has its sequence's.
constexpr uint32_t kSpecRowFree = 0xFFFFFFFEu;
ZGML_SPEC_FN uint32_t spec_free_rows(uint32_t* row_state, uint32_t T) {
    for (uint32_t j = 0; j < T; j++) row_state[j] = kSpecRowFree;
    return 0; // (forced tokens placed: `drafted` grows by the mode's real drafts alone)
}
ZGML_SPEC_FN bool spec_row_selects(uint32_t row_state) { return row_state != kConstraintDead; }

// ── DRAFTS FROM A MODEL UNDER A CONSTRAINT (zgml_hip_resident_decode_speculative_model_constrained): the draft is masked ──
// DRAFTS FROM A MODEL with the TARGET's automaton walked between the draft executions. A verify step runs at (hist[pos], pos);
// c[0] = hist[pos], row_state[0] = the sequence's state. For j = 0 .. T-1 the draft program executes on c[j] at pos + j and
// stores its own KV column, as without a constraint. For j < T - 1, with s = row_state[j]:
//   s dead, or s allows no token   there is no draft: c[j + 1] = c[j] (a valid token: the draft's next execution and the target's
//                                  prep stay in range) and row_state[j + 1] = kConstraintDead
//   otherwise                      c[j + 1] = the first maximum of the draft's logits row over the tokens ALLOWED in s
//                                  (constraint_row_allows(next[s], class_of[t])), in the order of the plain first maximum: larger
//                                  value wins, lower index among equals; a forbidden token contributes nothing, so the first allowed
//                                  token wins when nothing beats it (a row of -inf). row_state[j + 1] = next[s][class_of[c[j + 1]]],
//                                  never dead.
// The T-th execution exists for its KV column alone; its maximum is dropped. `drafted` grows, per step that is not idle, by the
// number of j in 1 .. T-1 with row_state[j] != kConstraintDead: no pads are counted and there is no separate count of forced
// tokens. An idle step makes every row dead (so its draft executions repeat one token). Everything behind the drafts is UNDER A
// CONSTRAINT's: g[j] the constrained pick under row_state[j] or kSpecNoPick, spec_accept, spec_emit_count, spec_dead_end_cut,
// spec_stop_cut, spec_state_advance. Every emitted token is the target's constrained pick over a confirmed context at its own
// position and state: the drafts change how many steps run, never the tokens.
// A consequence: in a state with forced[s] != kConstraintNoForced exactly one token is allowed, so the masked first maximum IS
// forced[s] whatever the logits are — the draft rule serves forced tokens without a forced[] lookup and without a placing pass.
// What the draft launch leaves of this rule: c[0] (spec_candidates_model) and row_state[0]; the executions' advances write the rest.

// the first maximum of row[0, vocab) over the tokens allowed by the state row `srow` = next[s]; -1: s allows no token
ZGML_SPEC_FN int64_t spec_masked_first_max(const float* row, uint32_t vocab, const uint16_t* srow, const uint16_t* class_of) {
    int64_t best = -1;
    for (uint32_t t = 0; t < vocab; t++)
        if (constraint_row_allows(srow, class_of[t]) && (best < 0 || row[t] > row[best])) best = t; // strict >: the lower index wins among equals
    return best;
}

// behind execution j < T - 1: d = the masked first maximum under s = row_state[j] (anything when s is dead; -1: none), c_prev =
// c[j] -> c[j + 1], row_state[j + 1]; returns what `drafted` grows by
ZGML_SPEC_FN uint32_t spec_draft_advance_constrained(uint32_t c_prev, uint32_t s, int64_t d, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes,
                                                     uint32_t* c_next, uint32_t* s_next) {
    if (s == kConstraintDead || d < 0) {
        *c_next = c_prev, *s_next = kConstraintDead;
        return 0;
    }
    *c_next = (uint32_t)d, *s_next = constraint_advance(next, n_classes, class_of, s, (uint32_t)d); // (d is allowed in s: never dead)
    return 1;
}

// the whole rule of a step, for the host probe (the kernels evaluate it one execution at a time): draft_row(j, c) is the logits
// row of the draft's execution j given c[0..j]; behind a dead state it is not asked for. Returns what `drafted` grows by
template <class RowOf>
ZGML_SPEC_FN uint32_t spec_candidates_model_constrained(uint32_t tok, uint32_t T, uint32_t vocab, uint32_t state, const uint16_t* class_of, const uint16_t* next,
                                                        uint32_t n_classes, RowOf draft_row, uint32_t* c, uint32_t* row_state) {
    uint32_t drafted = 0;
    spec_candidates_model(tok, T, c);
    row_state[0] = state;
    for (uint32_t j = 0; j + 1 < T; j++) {
        const uint32_t s = row_state[j];
        const int64_t d = s == kConstraintDead ? -1 : spec_masked_first_max(draft_row(j, c), vocab, next + (uint64_t)s * n_classes, class_of);
        drafted += spec_draft_advance_constrained(c[j], s, d, class_of, next, n_classes, &c[j + 1], &row_state[j + 1]);
    }
    return drafted;
}

// the dead-end cut: g[acc] without a pick ends the emission in front of itself — at most acc of the m tokens come out — and
// finishes the call (*dead). m: what spec_emit_count left
template <class G>
ZGML_SPEC_FN uint32_t spec_dead_end_cut(const G* g, uint32_t acc, uint32_t m, bool* dead) {
    *dead = g[acc] == (G)kSpecNoPick;
    return *dead && acc < m ? acc : m;
}

// the sequence's state behind the m emitted tokens g[0..m-1] (each the pick of the state reached: always allowed)
template <class G>
ZGML_SPEC_FN uint32_t spec_state_advance(const G* g, uint32_t m, uint32_t state, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes) {
    for (uint32_t k = 0; k < m && state != kConstraintDead; k++) state = constraint_advance(next, n_classes, class_of, state, (uint32_t)g[k]); // (never dead: no row of the table is read behind it)
    return state;
}

} // namespace zgml
