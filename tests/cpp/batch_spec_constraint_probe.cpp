// batch_spec_constraint_probe.cpp — what zgml_amd/csrc/spec.h states for a sequence WITHOUT an automaton inside a constrained
// batched verify step (zgml_hip_resident_decode_batch_speculative_constrained): the free row's state word, the rows of such a
// sequence's step, and the predicate the select launch asks of every row's state word. Behind a C ABI for
// tests/test_batch_spec_constraint_host.py, which holds them to tests/batch_spec_constraint_model.py; bscp_pass is a step's pass
// for either kind of sequence, as spec_decode.hip's spec_constrain takes it: the table row's con_active decides.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I include -shared -fPIC. With -DBATCH_SPEC_CONSTRAINT_PROBE_MAIN the file is a
// stand-alone program (built with -fsanitize=address,undefined by the tests).
#include <stdio.h>

#include <vector>

#include "../../zgml_amd/csrc/spec.h"

using namespace zgml;

extern "C" {

uint32_t bscp_row_free() { return kSpecRowFree; }
uint32_t bscp_free_rows(uint32_t* row_state, uint32_t T) { return spec_free_rows(row_state, T); }
int bscp_row_selects(uint32_t row_state) { return spec_row_selects(row_state) ? 1 : 0; }

// the pass of one sequence's step: c[T] in and out, row_state[T] out; returns what `drafted` grows by beside `real`
uint32_t bscp_pass(uint32_t* c, uint32_t T, uint32_t real, uint32_t attached, uint32_t state, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes,
                   const uint32_t* forced, uint32_t* row_state) {
    if (!attached) return spec_free_rows(row_state, T);
    return spec_constrain_candidates(c, T, real, state, class_of, next, n_classes, forced, row_state);
}

} // extern "C"

#ifdef BATCH_SPEC_CONSTRAINT_PROBE_MAIN
int main() {
    // the free word is no state (states are < 0xFFFF), not dead, no pick's sentinel; every state selects, the dead row alone does not
    if (kSpecRowFree < kConstraintMaxStates || kSpecRowFree == kConstraintDead || kSpecRowFree == kSpecNoPick) return 1;
    if (!spec_row_selects(kSpecRowFree) || spec_row_selects(kConstraintDead)) return 2;
    for (uint32_t s = 0; s < kConstraintMaxStates; s++)
        if (!spec_row_selects(s)) return 3;
    for (uint32_t T = 1; T <= 16; T++) {
        std::vector<uint32_t> c(T, 7), rows(T, 0), before(c);
        if (bscp_pass(c.data(), T, T / 2, 0, 0, nullptr, nullptr, 0, nullptr, rows.data()) != 0 || c != before) return 4;
        for (uint32_t j = 0; j < T; j++)
            if (rows[j] != kSpecRowFree) return 5;
    }
    // an attached sequence beside it: one state that allows every token and forces none — the candidates stay, every row is state 0
    const uint16_t class_of[4] = {0, 0, 0, 0}, next[1] = {0};
    const uint32_t forced[1] = {kConstraintNoForced};
    uint32_t c[4] = {1, 2, 3, 3}, rows[4];
    if (bscp_pass(c, 4, 2, 1, 0, class_of, next, 1, forced, rows) != 0 || c[1] != 2 || c[3] != 3 || rows[0] || rows[3]) return 6;
    printf("batch_spec_constraint_probe ok\n");
    return 0;
}
#endif
