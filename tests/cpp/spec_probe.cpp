// spec_probe.cpp — a C shim over the draft and acceptance rules of speculative decode (zgml_amd/csrc/spec.h: the very functions
// the kernels of spec_decode.hip call) for tests/test_spec_decode_host.py: the rules are plain C++, so they are checked against a
// Python model without a GPU.
#include <cstdint>

#include "../../zgml_amd/csrc/spec.h"

extern "C" {

// the T candidates of a lookup step over hist[0..pos]; *match receives the match position (-1: none). Returns the real drafts.
uint32_t sp_candidates_lookup(const uint32_t* hist, uint32_t pos, uint32_t ngram, uint32_t T, uint32_t* cand, int64_t* match) {
    *match = zgml::spec_lookup(hist, pos, ngram);
    return zgml::spec_candidates_lookup(hist, pos, *match, T, cand);
}

// the largest match position of ONE suffix length (-1: none, or the length does not apply at this position)
int64_t sp_ngram_find(const uint32_t* hist, uint32_t pos, uint32_t n) { return zgml::spec_ngram_find(hist, pos, n); }

uint32_t sp_candidates_provided(uint32_t tok, uint32_t pos, uint32_t start_pos, const uint32_t* drafts, uint32_t n_drafts, uint32_t T, uint32_t* cand) {
    return zgml::spec_candidates_provided(tok, pos, start_pos, drafts, n_drafts, T, cand);
}

uint32_t sp_accept(const uint32_t* cand, const uint32_t* g, uint32_t T) { return zgml::spec_accept(cand, g, T); }

uint32_t sp_emit_count(uint32_t a, uint32_t n_tokens, uint32_t produced) { return zgml::spec_emit_count(a, n_tokens, produced); }

} // extern "C"
