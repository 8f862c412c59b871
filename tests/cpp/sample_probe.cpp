// sample_probe.cpp — zgml_amd/csrc/sample.h behind a C ABI for the CPU tests (tests/test_sample_host.py) and as the host side of
// the GPU tests (tests/test_hip_sample.py compares a device pick with sp_sample over the same logits bits). The header is the
// rule; the only thing added here is the plain way to the candidate list: every key, sorted.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -shared -fPIC. With -DSAMPLE_PROBE_MAIN the file is a stand-alone program that runs
// random cases (built with -fsanitize=address,undefined by the tests).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "../../zgml_amd/csrc/sample.h"

using namespace zgml;

// the k = min(top_k, n) largest keys of v[0, n), descending
static std::vector<uint64_t> candidates(const float* v, uint32_t n, uint32_t top_k) {
    std::vector<uint64_t> keys(n);
    for (uint32_t i = 0; i < n; i++) keys[i] = sample_key(v[i], i);
    const uint32_t k = sample_top_k(top_k, n);
    std::partial_sort(keys.begin(), keys.begin() + k, keys.end(), std::greater<uint64_t>());
    keys.resize(k);
    return keys;
}

extern "C" {

void sp_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { sample_philox4x32_10(ctr, key, out); }
float sp_u_of_word(uint32_t w) { return sample_u_of_word(w); }
float sp_uniform(uint64_t seed, uint32_t stream, uint32_t position) { return sample_uniform((uint32_t)seed, (uint32_t)(seed >> 32), stream, position); }
float sp_exp(float x) { return sample_exp(x); }

// the candidates' indices into out[0, k); returns k
uint32_t sp_candidates(const float* v, uint32_t n, uint32_t top_k, uint32_t* out) {
    const std::vector<uint64_t> keys = candidates(v, n, top_k);
    for (size_t j = 0; j < keys.size(); j++) out[j] = sample_key_index(keys[j]);
    return (uint32_t)keys.size();
}

// the pick for a given u: the token; *rank_out (may be null) its rank among the candidates
uint32_t sp_pick(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, float u, uint32_t* rank_out) {
    const std::vector<uint64_t> keys = candidates(v, n, top_k);
    const uint32_t j = sample_pick(keys.data(), (uint32_t)keys.size(), 1.0f / temperature, top_p, u);
    if (rank_out) *rank_out = j;
    return sample_key_index(keys[j]);
}

// the whole rule: the token sampled from v at `position`
uint32_t sp_sample(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, uint64_t seed, uint32_t stream, uint32_t position) {
    return sp_pick(v, n, top_k, temperature, top_p, sp_uniform(seed, stream, position), nullptr);
}

} // extern "C"

#ifdef SAMPLE_PROBE_MAIN
int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull; // (splitmix64: the cases need no more than a fixed stream of bits)
    auto next = [&] {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const uint32_t sizes[] = {1, 2, 255, 256, 257, 1000, 4097}, ks[] = {0, 1, 2, 40, 256};
    const float temps[] = {0.25f, 1.0f, 4.0f}, ps[] = {0.5f, 0.95f, 1.0f};
    uint64_t sum = 0;
    for (int c = 0; c < 400; c++) {
        const uint32_t n = sizes[next() % 7], k = ks[next() % 5];
        std::vector<float> v(n);
        const uint32_t kind = (uint32_t)(next() % 4);
        for (auto& x : v) {
            const uint64_t r = next();
            x = kind == 0 ? 0.0f : (float)((int64_t)(r % 2001) - 1000) * (kind == 1 ? 0.01f : 1.0f);
            if (kind == 3 && r % 7 == 0) x = (r >> 20) % 3 == 0 ? -INFINITY : (r >> 20) % 3 == 1 ? NAN : -0.0f;
        }
        std::vector<uint32_t> cand(kSampleMaxK);
        const uint32_t kc = sp_candidates(v.data(), n, k, cand.data());
        if (kc != sample_top_k(k, n)) return 1;
        for (uint32_t j = 0; j < kc; j++)
            if (cand[j] >= n) return 2;
        const uint32_t tok = sp_sample(v.data(), n, k, temps[next() % 3], ps[next() % 3], next(), (uint32_t)next(), (uint32_t)(next() % 4096));
        if (std::find(cand.begin(), cand.begin() + kc, tok) == cand.begin() + kc) return 3;
        sum += tok;
    }
    printf("sample_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
