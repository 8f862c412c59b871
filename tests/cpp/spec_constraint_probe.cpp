// spec_constraint_probe.cpp — constrained speculative decode (zgml_hip_resident_decode_speculative_constrained) as the headers state
// it, behind a C ABI for tests/test_spec_constraint_host.py: constraint_forced (zgml_amd/csrc/sample_params.h), the pass over a
// step's candidates, the dead-end cut and the state's advance (zgml_amd/csrc/spec.h) — the functions the runtime and the kernels
// of spec_decode.hip call — and the whole loop over a synthetic model, in the order the draft and the accept launch apply the
// rules. The pick of a row is constraint_probe.cpp's c_constraint_sample, included here as source: one plain way through
// sample.h, not two.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I include -shared -fPIC. With -DSPEC_CONSTRAINT_PROBE_MAIN the file is a stand-alone
// program that runs random cases (built with -fsanitize=address,undefined by the tests).
#include "constraint_probe.cpp"

#include "../../zgml_amd/csrc/spec.h"

namespace {

// the synthetic model: the logits row behind `token` at position `pos` (tests/spec_constraint_model.py: hashed_row, the same bits)
void hashed_row(uint32_t pos, uint32_t token, uint32_t n, float* v) {
    const uint64_t salt = (uint64_t)pos * 0x10001ull + (uint64_t)token * 0x3Dull + 7ull;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t z = ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ull + salt;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        v[i] = (float)((z >> 20) & 0xFFFFull) / 256.0f;
    }
}

} // namespace

extern "C" {

uint32_t scp_no_pick() { return kSpecNoPick; }
uint32_t scp_no_forced() { return kConstraintNoForced; }
uint32_t scp_dead() { return kConstraintDead; }

// forced[n_states] of an automaton that constraint_check accepts; -1: it does not
int scp_forced(const zgml_token_dfa* dfa, uint32_t* forced) {
    if (constraint_check(dfa)) return -1;
    std::vector<uint32_t> count(dfa->n_classes), first(dfa->n_classes);
    constraint_forced(dfa, count.data(), first.data(), forced);
    return 0;
}

// the pass: c[T] in and out, row_state[T] out; returns the forced tokens placed at pad positions
uint32_t scp_constrain(uint32_t* c, uint32_t T, uint32_t real, uint32_t state, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes,
                       const uint32_t* forced, uint32_t* row_state) {
    return spec_constrain_candidates(c, T, real, state, class_of, next, n_classes, forced, row_state);
}

// The loop over the synthetic model. sampling: temperature, top_k, top_p, seed, stream; penalties: repeat, presence, frequency,
// window; drafts == NULL with mode 0: n-gram lookup. tokens_out[n_tokens] (-1 behind the end), stats[3] = steps, drafted,
// accepted, *state the automaton's state in and out. Returns the tokens produced.
uint32_t scp_loop(uint32_t vocab, uint32_t first_token, uint32_t start_pos, uint32_t n_tokens, uint32_t T, const uint32_t* history, uint32_t n_history,
                  uint32_t mode, const uint32_t* drafts, uint32_t n_drafts, uint32_t ngram, const uint32_t* stop, uint32_t n_stop, float temperature, uint32_t top_k,
                  float top_p, uint64_t seed, uint32_t stream, float repeat, float presence, float frequency, uint32_t window, const zgml_token_dfa* dfa,
                  uint32_t* state, int64_t* tokens_out, uint32_t* stats) {
    std::vector<uint32_t> forced(dfa->n_states);
    if (scp_forced(dfa, forced.data())) return 0;
    const uint32_t lo = n_history ? 0 : start_pos;
    std::vector<uint32_t> hist(history, history + n_history); // hist[q - lo] = the token at position q
    hist.push_back(first_token);
    std::vector<uint32_t> c(T), g(T), row_state(T);
    std::vector<float> v(vocab);
    uint32_t pos = start_pos, produced = 0, wanted = n_tokens;
    stats[0] = stats[1] = stats[2] = 0;
    for (uint32_t i = 0; i < n_tokens; i++) tokens_out[i] = -1;
    while (produced < wanted) {
        // [draft]
        uint32_t real;
        if (mode == 1)
            real = spec_candidates_provided(hist.back(), pos, start_pos, drafts, n_drafts, T, c.data());
        else
            real = spec_candidates_lookup(hist.data(), pos - lo, spec_lookup(hist.data(), pos - lo, ngram), T, c.data());
        stats[1] += real + spec_constrain_candidates(c.data(), T, real, *state, dfa->class_of, dfa->next, dfa->n_classes, forced.data(), row_state.data());
        // [plan] [select] [merge + pick]: row j over its own state, its window the history up to pos and the candidates behind it
        for (uint32_t j = 0; j < T; j++) {
            g[j] = kSpecNoPick;
            if (row_state[j] == kConstraintDead) continue;
            hashed_row(pos + j, c[j], vocab, v.data());
            std::vector<uint32_t> recent(hist);
            recent.insert(recent.end(), c.begin() + 1, c.begin() + 1 + j);
            const int64_t t = c_constraint_sample(v.data(), vocab, top_k, temperature, top_p, seed, stream, pos + j, repeat, presence, frequency, window, recent.data(),
                                                  (uint32_t)recent.size(), dfa->class_of, dfa->next, dfa->n_classes, row_state[j], nullptr);
            if (t >= 0) g[j] = (uint32_t)t;
        }
        // [accept]
        const uint32_t acc = spec_accept(c.data(), g.data(), T);
        uint32_t m = spec_emit_count(acc, wanted, produced);
        bool stopped = false, dead = false;
        m = spec_dead_end_cut(g.data(), acc, m, &dead);
        m = spec_stop_cut(g.data(), m, n_stop, stop, &stopped);
        for (uint32_t k = 0; k < m; k++) tokens_out[produced + k] = (int64_t)g[k], hist.push_back(g[k]);
        *state = spec_state_advance(g.data(), m, *state, dfa->class_of, dfa->next, dfa->n_classes);
        pos += m, produced += m;
        if (stopped || dead) wanted = produced;
        stats[0] += 1, stats[2] += acc;
    }
    return produced;
}

} // extern "C"

#ifdef SPEC_CONSTRAINT_PROBE_MAIN
int main() {
    uint64_t rs = 0x243F6A8885A308D3ull;
    auto rnd = [&] {
        uint64_t z = (rs += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    uint64_t sum = 0;
    for (int cs = 0; cs < 200; cs++) {
        const uint32_t V = 40 + (uint32_t)(rnd() % 200), S = 1 + (uint32_t)(rnd() % 6), C = 1 + (uint32_t)(rnd() % 60), T = 2 + (uint32_t)(rnd() % 7);
        std::vector<uint16_t> class_of(V), next((size_t)S * C);
        for (auto& x : class_of) x = (uint16_t)(rnd() % C); // (C up to V: singleton and empty classes occur)
        const uint32_t forbid = (uint32_t)(rnd() % 4);
        for (auto& x : next) x = rnd() % 4 < forbid ? kConstraintForbidden : (uint16_t)(rnd() % S);
        const zgml_token_dfa dfa{S, C, V, 0, class_of.data(), next.data()};
        std::vector<uint32_t> forced(S);
        if (scp_forced(&dfa, forced.data())) return 1;
        for (uint32_t s = 0; s < S; s++) { // against the count over every token
            uint32_t n = 0, tok = kConstraintNoForced;
            for (uint32_t i = 0; i < V; i++)
                if (c_constraint_allowed(next.data(), C, class_of.data(), s, i) && n++ == 0) tok = i;
            if (forced[s] != (n == 1 ? tok : kConstraintNoForced)) return 2;
        }
        const uint32_t n = 1 + (uint32_t)(rnd() % 20), start = (uint32_t)(rnd() % 5);
        std::vector<uint32_t> history(rnd() % 2 ? start : 0), drafts(rnd() % 30), stop(rnd() % 3);
        for (auto& t : history) t = (uint32_t)(rnd() % V);
        for (auto& t : drafts) t = (uint32_t)(rnd() % V);
        for (auto& t : stop) t = (uint32_t)(rnd() % V);
        std::vector<int64_t> toks(n);
        uint32_t stats[3], state = (uint32_t)(rnd() % S);
        const uint32_t state0 = state;
        const uint32_t made = scp_loop(V, (uint32_t)(rnd() % V), start, n, T, history.data(), (uint32_t)history.size(), (uint32_t)(cs % 2), drafts.data(), (uint32_t)drafts.size(),
                                       1 + (uint32_t)(rnd() % 4), stop.data(), (uint32_t)stop.size(), 0.8f, cs % 3 ? 40 : 1, 0.95f, rnd(), 3, cs % 4 ? 0.0f : 1.3f,
                                       cs % 4 ? 0.0f : 0.5f, 0.0f, cs % 4 ? 0 : 16, &dfa, &state, toks.data(), stats);
        if (made > n || stats[0] > n + 1) return 3;
        uint32_t walk = state0; // every emitted token is allowed where it was picked, and the state is the walk's
        for (uint32_t i = 0; i < n; i++) {
            if ((i < made) != (toks[i] >= 0)) return 4;
            if (i >= made) continue;
            walk = constraint_advance(next.data(), C, class_of.data(), walk, (uint32_t)toks[i]);
            if (walk == kConstraintDead) return 5;
            sum += (uint64_t)toks[i];
        }
        if (walk != state) return 6;
    }
    printf("spec_constraint_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
