// penalty_probe.cpp — the penalties of zgml_amd/csrc/sample.h (sample_penalize, sample_window_count, sample_window_span) and the
// refusals of zgml_amd/csrc/sample_params.h behind a C ABI: for the CPU tests (tests/test_penalty_host.py) and as the host side of
// the GPU tests (tests/test_hip_penalty.py compares a device pick with c_sample_penalized over the same logits bits and the same
// window). The headers are the rule; added here is only the plain way through it: copy the logits, penalise the window's
// distinct tokens, sort every key. The window is handed over the way zgml_hip_sample takes it: recent[0, n_recent) end with the
// token whose logits these are, the last W of them are read, a token >= n touches nothing.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -I include -shared -fPIC. With -DPENALTY_PROBE_MAIN the file is a stand-alone
// program that runs random cases (built with -fsanitize=address,undefined by the tests).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <vector>

#include "../../zgml_amd/csrc/sample.h"
#include "../../zgml_amd/csrc/sample_params.h"

using namespace zgml;

namespace {

struct Penalties {
    float repeat, presence, frequency; // as zgml_sampling holds them (repeat 0: neutral)
    uint32_t window;
};

bool active(const Penalties& pn) {
    const bool neutral = (pn.repeat == 0.0f || pn.repeat == 1.0f) && pn.presence == 0.0f && pn.frequency == 0.0f;
    return pn.window > 0 && !neutral;
}

// the logits as the selection sees them
std::vector<float> penalized(const float* v, uint32_t n, const Penalties& pn, const uint32_t* recent, uint32_t n_recent) {
    std::vector<float> out(v, v + n);
    if (!active(pn)) return out;
    const uint32_t m = std::min(n_recent, pn.window);
    const uint32_t* win = recent + (n_recent - m);
    const float repeat = pn.repeat == 0.0f ? 1.0f : pn.repeat, inv_repeat = 1.0f / repeat;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t count = sample_window_count(win, m, i);
        if (count && win[i] < n) out[win[i]] = sample_penalize(v[win[i]], count, repeat, inv_repeat, pn.presence, pn.frequency);
    }
    return out;
}

// the k = min(top_k, n) largest keys of v[0, n), descending
std::vector<uint64_t> candidates(const float* v, uint32_t n, uint32_t top_k) {
    std::vector<uint64_t> keys(n);
    for (uint32_t i = 0; i < n; i++) keys[i] = sample_key(v[i], i);
    const uint32_t k = sample_top_k(top_k, n);
    std::partial_sort(keys.begin(), keys.begin() + k, keys.end(), std::greater<uint64_t>());
    keys.resize(k);
    return keys;
}

} // namespace

extern "C" {

float c_penalize(float v, uint32_t count, float repeat, float presence, float frequency) {
    return sample_penalize(v, count, repeat, 1.0f / repeat, presence, frequency);
}

// out[i] = sample_window_count(win, m, i)
void c_window_counts(const uint32_t* win, uint32_t m, uint32_t* out) {
    for (uint32_t i = 0; i < m; i++) out[i] = sample_window_count(win, m, i);
}

uint32_t c_window_span(uint32_t position, uint32_t lo, uint32_t window, uint32_t* first) { return sample_window_span(position, lo, window, first); }

// the penalised logits themselves into out[0, n)
void c_penalized_logits(const float* v, uint32_t n, float repeat, float presence, float frequency, uint32_t window, const uint32_t* recent,
                        uint32_t n_recent, float* out) {
    const std::vector<float> pv = penalized(v, n, Penalties{repeat, presence, frequency, window}, recent, n_recent);
    std::copy(pv.begin(), pv.end(), out);
}

// the candidates' indices into out[0, k); returns k
uint32_t c_candidates_penalized(const float* v, uint32_t n, uint32_t top_k, float repeat, float presence, float frequency, uint32_t window,
                                const uint32_t* recent, uint32_t n_recent, uint32_t* out) {
    const std::vector<float> pv = penalized(v, n, Penalties{repeat, presence, frequency, window}, recent, n_recent);
    const std::vector<uint64_t> keys = candidates(pv.data(), n, top_k);
    for (size_t j = 0; j < keys.size(); j++) out[j] = sample_key_index(keys[j]);
    return (uint32_t)keys.size();
}

// the whole rule: the token sampled from v at `position` behind the window
uint32_t c_sample_penalized(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, uint64_t seed, uint32_t stream, uint32_t position,
                            float repeat, float presence, float frequency, uint32_t window, const uint32_t* recent, uint32_t n_recent) {
    const std::vector<float> pv = penalized(v, n, Penalties{repeat, presence, frequency, window}, recent, n_recent);
    const std::vector<uint64_t> keys = candidates(pv.data(), n, top_k);
    const float u = sample_uniform((uint32_t)seed, (uint32_t)(seed >> 32), stream, position);
    return sample_key_index(keys[sample_pick(keys.data(), (uint32_t)keys.size(), 1.0f / temperature, top_p, u)]);
}

// sample_params.h's verdict on a zgml_sampling: NULL, or why it is refused
const char* c_penalty_check(const zgml_sampling* sp, int form, uint32_t vocab, uint32_t start_pos, float* repeat, uint32_t* is_active) {
    return sample_penalty_check(sp, form, vocab, start_pos, repeat, is_active);
}

} // extern "C"

#ifdef PENALTY_PROBE_MAIN
int main() {
    uint64_t state = 0x243F6A8885A308D3ull; // (splitmix64: the cases need no more than a fixed stream of bits)
    auto next = [&] {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const uint32_t sizes[] = {1, 2, 255, 256, 257, 1000, 4097}, ks[] = {0, 1, 40, 256}, windows[] = {1, 2, 4, 64, 255, 256};
    const float repeats[] = {0.0f, 0.5f, 1.0f, 1.1f, 2.0f}, shifts[] = {0.0f, 0.5f, -0.75f};
    uint64_t sum = 0;
    for (int c = 0; c < 400; c++) {
        const uint32_t n = sizes[next() % 7], k = ks[next() % 4], W = windows[next() % 6];
        std::vector<float> v(n);
        for (auto& x : v) {
            const uint64_t r = next();
            x = (float)((int64_t)(r % 2001) - 1000) * 0.01f;
            if (r % 11 == 0) x = (r >> 20) % 4 == 0 ? -INFINITY : (r >> 20) % 4 == 1 ? NAN : (r >> 20) % 4 == 2 ? -0.0f : 0.0f;
        }
        // a history of 0 .. 300 tokens from a small alphabet (repeats are the point), some of them >= n
        std::vector<uint32_t> recent(next() % 301);
        const uint32_t alphabet = 1 + (uint32_t)(next() % 40);
        for (auto& t : recent) t = (uint32_t)(next() % alphabet) * (n / alphabet + 1) + (next() % 9 == 0 ? n : 0);
        // the counts against a map over the same slice
        const uint32_t m = std::min<uint32_t>((uint32_t)recent.size(), W);
        const uint32_t* win = recent.data() + (recent.size() - m);
        std::map<uint32_t, uint32_t> want;
        for (uint32_t i = 0; i < m; i++) want[win[i]]++;
        std::vector<uint32_t> counts(m + 1);
        c_window_counts(win, m, counts.data());
        std::map<uint32_t, uint32_t> got;
        for (uint32_t i = 0; i < m; i++)
            if (counts[i]) {
                if (got.count(win[i])) return 1; // a token reported twice
                got[win[i]] = counts[i];
            }
        if (got != want) return 2;
        const Penalties pn{repeats[next() % 5], shifts[next() % 3], shifts[next() % 3], W};
        std::vector<uint32_t> cand(kSampleMaxK);
        const uint32_t kc = c_candidates_penalized(v.data(), n, k, pn.repeat, pn.presence, pn.frequency, pn.window, recent.data(), (uint32_t)recent.size(), cand.data());
        if (kc != sample_top_k(k, n)) return 3;
        for (uint32_t j = 0; j < kc; j++)
            if (cand[j] >= n) return 4;
        // a token outside the window keeps its bits
        const std::vector<float> pv = penalized(v.data(), n, pn, recent.data(), (uint32_t)recent.size());
        for (uint32_t i = 0; i < n; i++)
            if (!want.count(i) && sample_f32_bits(pv[i]) != sample_f32_bits(v[i])) return 5;
        const uint32_t tok = c_sample_penalized(v.data(), n, k, 0.8f, 0.95f, next(), (uint32_t)next(), (uint32_t)(next() % 4096), pn.repeat, pn.presence,
                                                pn.frequency, pn.window, recent.data(), (uint32_t)recent.size());
        if (std::find(cand.begin(), cand.begin() + kc, tok) == cand.begin() + kc) return 6;
        uint32_t first = 0;
        const uint32_t pos = (uint32_t)(next() % 600), lo = (uint32_t)(next() % (pos + 1));
        const uint32_t span = c_window_span(pos, lo, W, &first);
        if (span != std::min(W, pos - lo + 1) || first != pos + 1 - span) return 7;
        sum += tok;
    }
    // the refusals, every pointer and count that the check reads
    zgml_sampling sp{};
    float repeat = 0.0f;
    uint32_t on = 0;
    const uint32_t toks[3] = {1, 2, 3};
    sp.repeat_penalty = 1.1f, sp.penalty_window = 4, sp.recent = toks, sp.n_recent = 3;
    if (c_penalty_check(&sp, 1, 4, 3, &repeat, &on) || !on || repeat != 1.1f) return 8;
    if (!c_penalty_check(&sp, 1, 3, 3, &repeat, &on) || !c_penalty_check(&sp, 1, 4, 2, &repeat, &on) || !c_penalty_check(&sp, 2, 4, 3, &repeat, &on)) return 9;
    printf("penalty_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
