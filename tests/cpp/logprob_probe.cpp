// logprob_probe.cpp — the log-probability rule of zgml_amd/csrc/sample.h behind a C ABI for the CPU tests
// (tests/test_logprob_host.py) and as the host side of the GPU tests (tests/test_hip_logprob.py compares a device value with
// lp_logprob over the same logits bits), and the refusals of zgml_amd/csrc/sample_params.h. The header is the rule; the only thing
// added here is the walk over a row's blocks.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -shared -fPIC -I include. With -DLOGPROB_PROBE_MAIN the file is a stand-alone program
// that runs random cases (built with -fsanitize=address,undefined by the tests).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../zgml_amd/csrc/sample_params.h"

using namespace zgml;

// (m_b, s_b) of every block of v[0, n)
static uint32_t partials(const float* v, uint64_t n, std::vector<float>& m, std::vector<float>& s) {
    const uint32_t nb = logprob_blocks(n);
    m.assign(nb, 0.0f), s.assign(nb, 0.0f);
    for (uint32_t b = 0; b < nb; b++) {
        const uint64_t start = (uint64_t)b * kLogprobBlock;
        logprob_block(v + start, (uint32_t)(n - start < kLogprobBlock ? n - start : kLogprobBlock), &m[b], &s[b]);
    }
    return nb;
}

extern "C" {

float lp_log(float x) { return sample_log(x); }

// the block pairs of a row into m_out / s_out (logprob_blocks(n) words each); returns their number
uint32_t lp_partials(const float* v, uint64_t n, float* m_out, float* s_out) {
    std::vector<float> m, s;
    const uint32_t nb = partials(v, n, m, s);
    for (uint32_t b = 0; b < nb; b++) m_out[b] = m[b], s_out[b] = s[b];
    return nb;
}

// out[i] = the log-probability of tokens[i] under the row v[0, n)
void lp_logprobs(const float* v, uint64_t n, const uint32_t* tokens, uint32_t n_tokens, float* out) {
    std::vector<float> m, s;
    const uint32_t nb = partials(v, n, m, s);
    float M, S;
    logprob_finish(m.data(), s.data(), nb, &M, &S);
    for (uint32_t i = 0; i < n_tokens; i++) out[i] = logprob_of(v[tokens[i]], M, S);
}

float lp_logprob(const float* v, uint64_t n, uint32_t token) {
    float out;
    lp_logprobs(v, n, &token, 1, &out);
    return out;
}

// the refusals: the reason (a static string) or NULL
const char* lp_check(uint64_t buf_size, uint64_t offset, uint64_t n, uint32_t rows, const uint32_t* tokens, const float* out) {
    return logprobs_check(buf_size, offset, n, rows, tokens, out);
}
const char* lp_field_check(int has_field, uint64_t n) {
    zgml_sampling sp{};
    sp.logprobs = has_field ? 1u : 0u;
    return sample_logprobs_check(&sp, n);
}

} // extern "C"

#ifdef LOGPROB_PROBE_MAIN
int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull; // (splitmix64, as sample_probe.cpp)
    auto next = [&] {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    const uint32_t sizes[] = {1, 2, 255, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 50001};
    double sum = 0.0;
    for (int c = 0; c < 200; c++) {
        const uint32_t n = sizes[next() % 11];
        std::vector<float> v(n);
        const uint32_t kind = (uint32_t)(next() % 4);
        for (auto& x : v) {
            const uint64_t r = next();
            x = kind == 0 ? 0.0f : (float)((int64_t)(r % 2001) - 1000) * (kind == 1 ? 0.01f : 0.1f);
            if (kind == 3 && r % 7 == 0) x = (r >> 20) % 3 == 0 ? -INFINITY : (r >> 20) % 3 == 1 ? NAN : -0.0f;
        }
        std::vector<uint32_t> tok = {0, n - 1, (uint32_t)(next() % n)};
        std::vector<float> out(tok.size());
        lp_logprobs(v.data(), n, tok.data(), (uint32_t)tok.size(), out.data());
        for (float o : out) {
            if (o > 0.0f || o != o) return 1; // (no +inf in these rows: every value is a log of a probability)
            if (o > -1e30f) sum += o;
        }
        if (lp_check(n, 0, n, 1, tok.data(), out.data())) return 2;
        tok[0] = n;
        if (!lp_check(n, 0, n, 1, tok.data(), out.data())) return 3;
    }
    printf("logprob_probe ok %.3f\n", sum);
    return 0;
}
#endif
