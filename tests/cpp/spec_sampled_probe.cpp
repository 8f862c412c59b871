// spec_sampled_probe.cpp — the rules of sampled speculative decode (zgml_hip_resident_decode_speculative_sampled) behind a C ABI
// for tests/test_spec_sampled_host.py: the stop cut and the acceptance of zgml_amd/csrc/spec.h and the pick of
// zgml_amd/csrc/sample.h, the very functions the kernels call. One verify step's bookkeeping (sp_step) is those functions in the
// order spec_accept_kernel applies them.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -shared -fPIC. With -DSPEC_SAMPLED_PROBE_MAIN the file is a stand-alone program that
// runs random cases (built with -fsanitize=address,undefined by the tests).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "../../zgml_amd/csrc/sample.h"
#include "../../zgml_amd/csrc/spec.h"

using namespace zgml;

extern "C" {

// the cut m of g[0..m-1] under the stop set; *fired (may be null): a stop token was among them
uint32_t ssp_stop_cut(const uint32_t* g, uint32_t m, uint32_t n_stop, const uint32_t* stop, int32_t* fired) {
    bool f = false;
    const uint32_t cut = spec_stop_cut(g, m, n_stop, stop, &f);
    if (fired) *fired = f ? 1 : 0;
    return cut;
}

// the token of one logits row: the header's pick at `position` (every key, sorted: the plain way to the candidate list)
uint32_t ssp_sample(const float* v, uint32_t n, uint32_t top_k, float temperature, float top_p, uint64_t seed, uint32_t stream, uint32_t position) {
    std::vector<uint64_t> keys(n);
    for (uint32_t i = 0; i < n; i++) keys[i] = sample_key(v[i], i);
    const uint32_t k = sample_top_k(top_k, n);
    std::partial_sort(keys.begin(), keys.begin() + k, keys.end(), std::greater<uint64_t>());
    const float u = sample_uniform((uint32_t)seed, (uint32_t)(seed >> 32), stream, position);
    return sample_key_index(keys[sample_pick(keys.data(), k, 1.0f / temperature, top_p, u)]);
}

// what a verify step does with its candidates c[0..T) and its rows' tokens g[0..T): out[0] = accepted (before any cut),
// out[1] = tokens emitted, out[2] = a stop token fired
void ssp_step(const uint32_t* c, const uint32_t* g, uint32_t T, uint32_t wanted, uint32_t produced, uint32_t n_stop, const uint32_t* stop, uint32_t* out) {
    bool fired = false;
    out[0] = spec_accept(c, g, T);
    out[1] = spec_stop_cut(g, spec_emit_count(out[0], wanted, produced), n_stop, stop, &fired);
    out[2] = fired ? 1 : 0;
}

} // extern "C"

#ifdef SPEC_SAMPLED_PROBE_MAIN
int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull; // (splitmix64: the cases need no more than a fixed stream of bits)
    auto next = [&] {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    uint64_t sum = 0;
    for (int c = 0; c < 2000; c++) {
        const uint32_t T = 2 + (uint32_t)(next() % 5), n_stop = (uint32_t)(next() % 5);
        std::vector<uint32_t> cand(T), g(T), stop(n_stop); // (exact sizes: a read past T or n_stop is a heap overflow)
        for (auto& x : cand) x = (uint32_t)(next() % 4);
        for (auto& x : g) x = (uint32_t)(next() % 4);
        for (auto& x : stop) x = (uint32_t)(next() % 6);
        const uint32_t wanted = (uint32_t)(next() % 12), produced = (uint32_t)(next() % 12);
        uint32_t out[3];
        ssp_step(cand.data(), g.data(), T, wanted, produced, n_stop, stop.data(), out);
        if (out[0] >= T || out[1] > out[0] + 1 || (wanted > produced && out[1] > wanted - produced) || (wanted <= produced && out[1] != 0)) return 1;
        if (out[2] && (out[1] == 0 || !sample_is_stop(g[out[1] - 1], n_stop, stop.data()))) return 2; // a fired stop is the last token emitted
        for (uint32_t k = 0; k + 1 < out[1]; k++)
            if (sample_is_stop(g[k], n_stop, stop.data())) return 3; // ... and nothing in front of it is one
        sum += out[0] + 7 * out[1] + 31 * out[2];
    }
    const uint32_t sizes[] = {1, 2, 255, 257, 1000};
    for (int c = 0; c < 200; c++) {
        const uint32_t n = sizes[next() % 5];
        std::vector<float> v(n);
        for (auto& x : v) x = (float)((int64_t)(next() % 2001) - 1000) * 0.01f;
        const uint32_t tok = ssp_sample(v.data(), n, (uint32_t)(next() % 257), 0.8f, 0.95f, next(), (uint32_t)next(), (uint32_t)(next() % 4096));
        if (tok >= n) return 4;
        sum += tok;
    }
    printf("spec_sampled_probe ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
