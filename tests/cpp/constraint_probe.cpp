// constraint_probe.cpp — the constraint of zgml_amd/csrc/sample.h (constraint_allowed, constraint_advance, sample_real_keys) and the
// refusals of zgml_amd/csrc/sample_params.h (constraint_check, constraint_attach_check) behind a C ABI: for the CPU tests
// (tests/test_constraint_host.py) and as the host side of the GPU tests (tests/test_hip_constraint.py compares a device pick with
// c_constraint_sample over the same logits bits, the same window and the same automaton state). The headers are the rule; added
// here is only the plain way through it: copy the logits, penalise the window's distinct tokens, give every token its key or —
// when the state does not allow it — the pad 0, sort every key, count the real ones among the first top_k. The window is handed
// over the way zgml_hip_sample takes it (tests/cpp/penalty_probe.cpp).
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I include -shared -fPIC. With -DCONSTRAINT_PROBE_MAIN the file is a stand-alone
// program that runs random cases (built with -fsanitize=address,undefined by the tests).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "../../zgml_amd/csrc/sample.h"
#include "../../zgml_amd/csrc/sample_params.h"

using namespace zgml;

namespace {

struct Penalties {
    float repeat, presence, frequency; // as zgml_sampling holds them (repeat 0: neutral)
    uint32_t window;
};

struct Automaton {
    const uint16_t* class_of; // nullptr: no constraint
    const uint16_t* next;
    uint32_t n_classes, state;
};

// the logits as the selection sees them (as tests/cpp/penalty_probe.cpp)
std::vector<float> penalized(const float* v, uint32_t n, const Penalties& pn, const uint32_t* recent, uint32_t n_recent) {
    std::vector<float> out(v, v + n);
    const bool neutral = (pn.repeat == 0.0f || pn.repeat == 1.0f) && pn.presence == 0.0f && pn.frequency == 0.0f;
    if (pn.window == 0 || neutral) return out;
    const uint32_t m = std::min(n_recent, pn.window);
    const uint32_t* win = recent + (n_recent - m);
    const float repeat = pn.repeat == 0.0f ? 1.0f : pn.repeat, inv_repeat = 1.0f / repeat;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t count = sample_window_count(win, m, i);
        if (count && win[i] < n) out[win[i]] = sample_penalize(v[win[i]], count, repeat, inv_repeat, pn.presence, pn.frequency);
    }
    return out;
}

// the candidates of v[0, n) in the automaton's state: keys descending, the real ones among the first sample_top_k(top_k, n)
std::vector<uint64_t> candidates(const float* v, uint32_t n, uint32_t top_k, const Automaton& a) {
    std::vector<uint64_t> keys(n);
    const uint16_t* const row = a.class_of ? a.next + (uint64_t)a.state * a.n_classes : nullptr;
    for (uint32_t i = 0; i < n; i++) keys[i] = !row || constraint_allowed(row, a.class_of, i) ? sample_key(v[i], i) : 0;
    const uint32_t k0 = sample_top_k(top_k, n);
    std::partial_sort(keys.begin(), keys.begin() + k0, keys.end(), std::greater<uint64_t>());
    keys.resize(sample_real_keys(keys.data(), k0));
    return keys;
}

} // namespace

extern "C" {

int c_constraint_allowed(const uint16_t* next, uint32_t n_classes, const uint16_t* class_of, uint32_t state, uint32_t token) {
    return constraint_allowed(next + (uint64_t)state * n_classes, class_of, token) ? 1 : 0;
}

uint32_t c_constraint_advance(const uint16_t* next, uint32_t n_classes, const uint16_t* class_of, uint32_t state, uint32_t token) {
    return constraint_advance(next, n_classes, class_of, state, token);
}

uint32_t c_real_keys(const uint64_t* keys, uint32_t k0) { return sample_real_keys(keys, k0); }

// the candidates' indices into out[0, k); returns k (0: the state allows no token). class_of == NULL: no constraint
uint32_t c_constraint_candidates(const float* v, uint32_t n, uint32_t top_k, float repeat, float presence, float frequency, uint32_t window,
                                 const uint32_t* recent, uint32_t n_recent, const uint16_t* class_of, const uint16_t* next, uint32_t n_classes, uint32_t state,
                                 uint32_t* out) {
    const std::vector<float> pv = penalized(v, n, Penalties{repeat, presence, frequency, window}, recent, n_recent);
    const std::vector<uint64_t> keys = candidates(pv.data(), n, top_k, Automaton{class_of, next, n_classes, state});
    for (size_t j = 0; j < keys.size(); j++) out[j] = sample_key_index(keys[j]);
    return (uint32_t)keys.size();
}

// the whole rule: the token sampled from v at `position` in `state` (-1: no token is allowed), and through *state_out (may be
// NULL) the state behind it
int64_t c_constraint_sample(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, uint64_t seed, uint32_t stream, uint32_t position,
                            float repeat, float presence, float frequency, uint32_t window, const uint32_t* recent, uint32_t n_recent,
                            const uint16_t* class_of, const uint16_t* next, uint32_t n_classes, uint32_t state, uint32_t* state_out) {
    const std::vector<float> pv = penalized(v, n, Penalties{repeat, presence, frequency, window}, recent, n_recent);
    const std::vector<uint64_t> keys = candidates(pv.data(), n, top_k, Automaton{class_of, next, n_classes, state});
    if (state_out) *state_out = state;
    if (keys.empty()) return -1;
    const float u = sample_uniform((uint32_t)seed, (uint32_t)(seed >> 32), stream, position);
    const uint32_t tok = sample_key_index(keys[sample_pick(keys.data(), (uint32_t)keys.size(), 1.0f / temperature, top_p, u)]);
    if (state_out && class_of) *state_out = constraint_advance(next, n_classes, class_of, state, tok);
    return (int64_t)tok;
}

// the pick alone at a given u over the candidates in `state`: the token (-1: none) and, through *rank (may be NULL), its rank
int64_t c_constraint_pick(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, float u, const uint16_t* class_of, const uint16_t* next,
                          uint32_t n_classes, uint32_t state, uint32_t* rank) {
    const std::vector<uint64_t> keys = candidates(v, n, top_k, Automaton{class_of, next, n_classes, state});
    if (keys.empty()) return -1;
    const uint32_t j = sample_pick(keys.data(), (uint32_t)keys.size(), 1.0f / temperature, top_p, u);
    if (rank) *rank = j;
    return (int64_t)sample_key_index(keys[j]);
}

// sample_params.h's verdicts: NULL, or why it is refused
const char* c_constraint_check(const zgml_token_dfa* dfa) { return constraint_check(dfa); }
const char* c_constraint_attach_check(uint32_t dfa_vocab, uint32_t dfa_states, uint32_t program_vocab, uint32_t n_seqs, uint32_t seq, uint32_t state) {
    return constraint_attach_check(dfa_vocab, dfa_states, program_vocab, n_seqs, seq, state);
}

} // extern "C"

#ifdef CONSTRAINT_PROBE_MAIN
int main() {
    uint64_t rs = 0x13198A2E03707344ull; // (splitmix64: the cases need no more than a fixed stream of bits)
    auto rnd = [&] {
        uint64_t z = (rs += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const uint32_t sizes[] = {1, 2, 255, 256, 257, 1000, 4097}, ks[] = {0, 1, 40, 256}, classes[] = {1, 2, 7, 64, 8192}, states[] = {1, 2, 5, 30};
    uint64_t sum = 0;
    for (int c = 0; c < 300; c++) {
        const uint32_t n = sizes[rnd() % 7], k = ks[rnd() % 4], C = classes[rnd() % 5], S = states[rnd() % 4];
        std::vector<float> v(n);
        for (auto& x : v) {
            const uint64_t r = rnd();
            x = (float)((int64_t)(r % 2001) - 1000) * 0.01f;
            if (r % 11 == 0) x = (r >> 20) % 4 == 0 ? -INFINITY : (r >> 20) % 4 == 1 ? NAN : (r >> 20) % 4 == 2 ? -0.0f : 0.0f;
        }
        std::vector<uint16_t> class_of(n), next((size_t)S * C);
        for (auto& x : class_of) x = (uint16_t)(rnd() % C);
        const uint32_t forbid = (uint32_t)(rnd() % 4); // 0: nothing forbidden .. 3: three quarters
        for (auto& x : next) x = rnd() % 4 < forbid ? kConstraintForbidden : (uint16_t)(rnd() % S);
        const zgml_token_dfa dfa{S, C, n, 0, class_of.data(), next.data()};
        if (c_constraint_check(&dfa)) return 1;
        std::vector<uint32_t> recent(rnd() % 40);
        for (auto& t : recent) t = (uint32_t)(rnd() % (n + 2));
        const Penalties pn{c % 3 ? 1.3f : 0.0f, c % 3 ? 0.5f : 0.0f, c % 3 == 2 ? 0.25f : 0.0f, (uint32_t)(rnd() % 65)};
        uint32_t state = (uint32_t)(rnd() % S);
        // a walk: every token is allowed in the state it was picked in, a candidate, and the walk ends in a state without tokens
        for (int step = 0; step < 12; step++) {
            std::vector<uint32_t> cand(kSampleMaxK);
            const uint32_t kc = c_constraint_candidates(v.data(), n, k, pn.repeat, pn.presence, pn.frequency, pn.window, recent.data(), (uint32_t)recent.size(),
                                                        class_of.data(), next.data(), C, state, cand.data());
            uint32_t allowed = 0;
            for (uint32_t i = 0; i < n; i++) allowed += (uint32_t)c_constraint_allowed(next.data(), C, class_of.data(), state, i);
            if (kc != std::min(sample_top_k(k, n), allowed)) return 2;
            for (uint32_t j = 0; j < kc; j++)
                if (cand[j] >= n || !c_constraint_allowed(next.data(), C, class_of.data(), state, cand[j])) return 3;
            uint32_t after = 0;
            const int64_t tok = c_constraint_sample(v.data(), n, k, 0.8f, 0.95f, rnd(), (uint32_t)rnd(), (uint32_t)(rnd() % 4096), pn.repeat, pn.presence, pn.frequency,
                                                    pn.window, recent.data(), (uint32_t)recent.size(), class_of.data(), next.data(), C, state, &after);
            if ((tok < 0) != (kc == 0)) return 4;
            if (tok < 0) {
                if (after != state) return 5;
                break;
            }
            if (std::find(cand.begin(), cand.begin() + kc, (uint32_t)tok) == cand.begin() + kc) return 6;
            if (after >= S || after != next[(size_t)state * C + class_of[(size_t)tok]]) return 7;
            state = after;
            recent.push_back((uint32_t)tok);
            sum += (uint64_t)tok;
        }
        // without an automaton the list is the unconstrained one
        std::vector<uint32_t> plain(kSampleMaxK);
        if (c_constraint_candidates(v.data(), n, k, 0.0f, 0.0f, 0.0f, 0, nullptr, 0, nullptr, nullptr, 0, 0, plain.data()) != sample_top_k(k, n)) return 8;
    }
    // the refusals, every table the check reads
    const uint16_t cls[4] = {0, 1, 2, 1}, nxt[6] = {0, 1, kConstraintForbidden, 1, 1, 0};
    zgml_token_dfa d{2, 3, 4, 0, cls, nxt};
    if (c_constraint_check(&d)) return 9;
    d.n_classes = 2; // class 2 is out of range
    if (!c_constraint_check(&d)) return 10;
    d = zgml_token_dfa{1, 3, 4, 0, cls, nxt}; // next state 1 is out of range
    if (!c_constraint_check(&d)) return 11;
    d = zgml_token_dfa{0, 3, 4, 0, cls, nxt};
    if (!c_constraint_check(&d) || !c_constraint_check(nullptr)) return 12;
    if (c_constraint_attach_check(4, 2, 4, 1, 0, 1) || !c_constraint_attach_check(4, 2, 5, 1, 0, 1) || !c_constraint_attach_check(4, 2, 4, 1, 1, 1) ||
        !c_constraint_attach_check(4, 2, 4, 1, 0, 2))
        return 13;
    printf("constraint_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
