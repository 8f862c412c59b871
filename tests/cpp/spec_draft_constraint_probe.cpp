// spec_draft_constraint_probe.cpp — the draft rule of speculative decode with a draft model under a constraint
// (zgml_hip_resident_decode_speculative_model_constrained) as zgml_amd/csrc/spec.h states it (DRAFTS FROM A MODEL UNDER A
// CONSTRAINT: spec_masked_first_max, spec_draft_advance_constrained, spec_candidates_model_constrained — the functions the kernels
// of greedy_tail.hip call through tail_device.h), behind a C ABI for tests/test_spec_draft_constraint_host.py.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I include -shared -fPIC. With -DSPEC_DRAFT_CONSTRAINT_PROBE_MAIN the file is a
// stand-alone program that runs random cases (built with -fsanitize=address,undefined by the tests).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../zgml_amd/csrc/spec.h"

using namespace zgml;

extern "C" {

uint32_t sdc_dead() { return kConstraintDead; }
uint32_t sdc_no_forced() { return kConstraintNoForced; }

// the first maximum of row[vocab] over the tokens state `state` allows; -1: none
int64_t sdc_masked_first_max(const float* row, uint32_t vocab, uint32_t state, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes) {
    return spec_masked_first_max(row, vocab, next + (uint64_t)state * n_classes, class_of);
}

// one step's candidates over the draft rows rows[T - 1][vocab] (row j: execution j's, whatever c is): c[T] and row_state[T] out;
// returns what `drafted` grows by. asked[T - 1] out: 1 where the rule asked for execution j's row
uint32_t sdc_candidates(uint32_t tok, uint32_t T, uint32_t vocab, uint32_t state, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes,
                        const float* rows, uint32_t* c, uint32_t* row_state, uint32_t* asked) {
    for (uint32_t j = 0; j + 1 < T; j++) asked[j] = 0;
    return spec_candidates_model_constrained(
        tok, T, vocab, state, class_of, next, n_classes,
        [&](uint32_t j, const uint32_t*) {
            asked[j] = 1;
            return rows + (uint64_t)j * vocab;
        },
        c, row_state);
}

} // extern "C"

#ifdef SPEC_DRAFT_CONSTRAINT_PROBE_MAIN
int main() {
    uint64_t rs = 0x13198A2E03707344ull;
    auto rnd = [&] {
        uint64_t z = (rs += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    uint64_t sum = 0;
    for (int cs = 0; cs < 400; cs++) {
        const uint32_t V = 1 + (uint32_t)(rnd() % 300), S = 1 + (uint32_t)(rnd() % 6), C = cs % 50 == 0 ? 8192 : 1 + (uint32_t)(rnd() % 60), T = 2 + (uint32_t)(rnd() % 7);
        std::vector<uint16_t> class_of(V), next((size_t)S * C);
        for (auto& x : class_of) x = (uint16_t)(rnd() % C);
        const uint32_t forbid = (uint32_t)(rnd() % 5);
        for (auto& x : next) x = rnd() % 4 < forbid ? kConstraintForbidden : (uint16_t)(rnd() % S);
        std::vector<float> rows((size_t)(T - 1) * V);
        for (auto& x : rows) x = rnd() % 5 == 0 ? -INFINITY : (float)(rnd() % 64) / 8.0f; // ties and -inf runs
        std::vector<uint32_t> c(T), row_state(T), asked(T);
        const uint32_t tok = (uint32_t)(rnd() % V), state = cs % 9 == 0 ? kConstraintDead : (uint32_t)(rnd() % S);
        const uint32_t drafted = sdc_candidates(tok, T, V, state, class_of.data(), next.data(), C, rows.data(), c.data(), row_state.data(), asked.data());
        uint32_t live = 0;
        if (c[0] != tok || row_state[0] != state) return 1;
        for (uint32_t j = 1; j < T; j++) {
            if (c[j] >= V) return 2;
            if (row_state[j] == kConstraintDead) {
                if (c[j] != c[j - 1]) return 3;
                continue;
            }
            live++;
            if (row_state[j - 1] == kConstraintDead || row_state[j] >= S) return 4;
            if (constraint_advance(next.data(), C, class_of.data(), row_state[j - 1], c[j]) != row_state[j]) return 5; // (the draft is allowed where it was taken)
        }
        if (drafted != live) return 6;
        sum += drafted;
    }
    printf("spec_draft_constraint_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
