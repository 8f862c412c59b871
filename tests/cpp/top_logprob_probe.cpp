// top_logprob_probe.cpp — the rule of the alternatives of zgml_amd/csrc/sample.h ("THE ALTERNATIVES") behind a C ABI for the CPU
// tests (tests/test_top_logprob_host.py) and as the host side of the GPU tests (tests/test_hip_top_logprob.py compares the device's
// tokens and values with tl_top over the same logits bits), and the host logic of zgml_amd/csrc/sample_params.h. The header is the
// rule; the only thing added here is the walk over a row's blocks for M and S and the padding of a row of entries.
// Build: g++ -O1 -std=c++17 -ffp-contract=off -shared -fPIC -I include. With -DTOP_LOGPROB_PROBE_MAIN the file is a stand-alone
// program that runs the rows of the sliced-form and edge tests (built with -fsanitize=address,undefined by the tests).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../zgml_amd/csrc/sample_params.h"

using namespace zgml;

// the row's M and S
static void row_ms(const float* v, uint64_t n, float* M, float* S) {
    const uint32_t nb = logprob_blocks(n);
    std::vector<float> m(nb), s(nb);
    for (uint32_t b = 0; b < nb; b++) {
        const uint64_t start = (uint64_t)b * kLogprobBlock;
        logprob_block(v + start, (uint32_t)(n - start < kLogprobBlock ? n - start : kLogprobBlock), &m[b], &s[b]);
    }
    logprob_finish(m.data(), s.data(), nb, M, S);
}

extern "C" {

// the alternatives of the row v[0, n) for the count a into tok[0, width) / val[0, width) (width >= a_eff), -1 and the quiet NaN
// behind a_eff; sliced == 0: the direct form; 1: the sliced form as the select launch cuts the row; > 1: the sliced form over
// slices of `sliced` logits (at most 32 of them: the merge must not depend on where the cuts are). Returns a_eff
uint32_t tl_top(const float* v, uint64_t n, uint32_t a, uint32_t width, int64_t* tok, float* val, uint32_t sliced) {
    uint64_t keys[kTopLogprobsMax];
    std::vector<uint64_t> heads((size_t)kSampleMaxSlices * kTopLogprobsMax);
    const uint32_t cuts = sliced > 1 ? (uint32_t)((n + sliced - 1) / sliced) : 1;
    if (cuts > kSampleMaxSlices) return 0xFFFFFFFFu;
    const uint32_t ae = sliced > 1    ? top_logprobs_keys_cut(v, n, a, cuts, sliced, keys, heads.data())
                        : sliced == 1 ? top_logprobs_keys_sliced(v, n, a, keys, heads.data())
                                      : top_logprobs_keys(v, n, a, keys);
    float M, S;
    row_ms(v, n, &M, &S);
    for (uint32_t j = 0; j < width; j++) {
        tok[j] = -1, val[j] = sample_bits_f32(kLogprobNaNBits);
        if (j >= ae) continue;
        uint32_t t;
        top_logprobs_entry(keys[j], M, S, &t, &val[j]);
        tok[j] = (int64_t)t;
    }
    return ae;
}

uint32_t tl_count(uint32_t a, uint64_t n) { return top_logprobs_count(a, n); }
uint32_t tl_slices(uint64_t n) { return sample_slices(n); }
uint32_t tl_slice_len(uint64_t n) { return sample_slice_len(n); }

// the refusals of zgml_hip_top_logprobs: the reason (a static string) or NULL
const char* tl_check(uint64_t buf_size, uint64_t offset, uint64_t n, uint32_t rows, uint32_t top_n, const int64_t* tokens_out, const float* out) {
    return top_logprobs_check(buf_size, offset, n, rows, top_n, tokens_out, out);
}

// the `top_logprobs` word of a zgml_sampling as the kernels read it
uint32_t tl_word(uint32_t logprobs, uint32_t top_logprobs) {
    zgml_sampling sp{};
    sp.logprobs = logprobs, sp.top_logprobs = top_logprobs;
    return sample_top_logprobs(&sp);
}

} // extern "C"

#ifdef TOP_LOGPROB_PROBE_MAIN
// both forms over one row for a = 1, 5, 64, 65: equal by bits; returns the number of entries, -1 on a difference
static int both(const std::vector<float>& v) {
    int made = 0;
    for (uint32_t a : {1u, 5u, 64u, 65u}) {
        int64_t t0[kTopLogprobsMax], t1[kTopLogprobsMax];
        float x0[kTopLogprobsMax], x1[kTopLogprobsMax];
        const uint32_t e0 = tl_top(v.data(), v.size(), a, kTopLogprobsMax, t0, x0, 0), e1 = tl_top(v.data(), v.size(), a, kTopLogprobsMax, t1, x1, 1);
        if (e0 != e1 || e0 != top_logprobs_count(a, v.size())) return -1;
        // ... and cut so that the last slice holds one element
        const uint32_t len = v.size() > 1 ? (uint32_t)((v.size() - 1 + kSampleMaxSlices - 2) / (kSampleMaxSlices - 1)) : 1;
        int64_t t2[kTopLogprobsMax];
        float x2[kTopLogprobsMax];
        if (len > 1 && (v.size() - 1) % len == 0) {
            if (tl_top(v.data(), v.size(), a, kTopLogprobsMax, t2, x2, len) != e0) return -1;
            for (uint32_t j = 0; j < kTopLogprobsMax; j++)
                if (t0[j] != t2[j] || sample_f32_bits(x0[j]) != sample_f32_bits(x2[j])) return -1;
        }
        for (uint32_t j = 0; j < kTopLogprobsMax; j++) {
            if (t0[j] != t1[j] || sample_f32_bits(x0[j]) != sample_f32_bits(x1[j])) return -1;
            if (j < e0 && (t0[j] < 0 || (uint64_t)t0[j] >= v.size())) return -1;
            if (j >= e0 && t0[j] != -1) return -1;
        }
        made += (int)e0;
    }
    return made;
}

int main() {
    const uint32_t sizes[] = {1, 2, 3, 63, 64, 65, 257, 1792, 1793, 1985, 3585, 4097, 50001, 57345}; // (63, 1985: 31 len + 1)
    long total = 0;
    for (uint32_t n : sizes) {
        const uint32_t slices = sample_slices(n), len = sample_slice_len(n);
        std::vector<std::vector<float>> rows;
        rows.emplace_back(n, -1.25f); // all equal: every alternative comes from slice 0
        std::vector<float> ramp(n), planted(n), mixed(n);
        for (uint32_t i = 0; i < n; i++) {
            ramp[i] = (float)i * 0.01f; // ... from the last slice
            planted[i] = -(float)(i % 97) * 0.125f;
            mixed[i] = i % 5 == 0 ? NAN : i % 7 == 0 ? -INFINITY : (float)((i * 2654435761u) % 1000) * 0.01f;
        }
        for (uint32_t l = 0; l < slices; l++) { // two large values per slice, at its first and its last index
            const uint64_t lo = (uint64_t)l * len, hi = lo + len < n ? lo + len : n;
            if (lo >= n) continue;
            planted[lo] = 100.0f + (float)l, planted[hi - 1] = 200.0f + (float)l;
        }
        rows.push_back(ramp), rows.push_back(planted), rows.push_back(mixed);
        rows.emplace_back(n, -INFINITY);
        std::vector<float> inf(n, 0.5f);
        inf[n / 2] = INFINITY;
        rows.push_back(inf);
        for (const auto& v : rows) {
            const int made = both(v);
            if (made < 0) return 1;
            total += made;
        }
    }
    int64_t t[1];
    float x[1];
    if (tl_check(100, 0, 10, 3, 5, t, x) || !tl_check(100, 0, 10, 3, 0, t, x) || !tl_check(100, 0, 10, 3, 65, t, x) || !tl_check(100, 0, 10, 3, 5, nullptr, x)) return 2;
    if (tl_word(1, 1000) != kTopLogprobsMax || tl_word(0, 7) != 0 || tl_word(2, 7) != 7) return 3;
    printf("top_logprob_probe ok %ld\n", total);
    return 0;
}
#endif
