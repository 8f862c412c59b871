// kvq_probe.cpp — the column quantisation of zgml_amd/csrc/kvq.h on the CPU, as a stand-alone program (tests/test_batch_kvq_host.py
// compares its output with the oracle's kvq_store on the same columns, to the bit). The header is the rule; added here is only the
// way through it: read the columns, quantise each with kvq_quantise_column, write the cache image.
//   kvq_probe <d_head> <n_cols> <in.f32> <out.bin>
// in:  n_cols columns of d_head f32 values, back to back.  out: the quantised cache layout of include/zgml_hip.h for n_cols columns
// and block size 32 — n_cols * d_head int8, then n_cols * d_head / 32 f32 scales.
// Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zgml_amd/csrc/kvq.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: kvq_probe <d_head> <n_cols> <in.f32> <out.bin>\n");
        return 2;
    }
    const uint32_t dh = (uint32_t)atoi(argv[1]), n_cols = (uint32_t)atoi(argv[2]);
    if (!dh || dh % 32 || !n_cols) {
        fprintf(stderr, "kvq_probe: d_head must be a multiple of 32 and n_cols > 0\n");
        return 2;
    }
    std::vector<float> in((size_t)dh * n_cols);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
        fprintf(stderr, "kvq_probe: cannot read %zu floats from %s\n", in.size(), argv[3]);
        return 1;
    }
    fclose(f);
    std::vector<int8_t> q(in.size());
    std::vector<float> scales(in.size() / 32);
    for (uint32_t c = 0; c < n_cols; c++)
        zgml::kvq_quantise_column(in.data() + (size_t)c * dh, dh, 32, q.data() + (size_t)c * dh, scales.data() + (size_t)c * (dh / 32));
    f = fopen(argv[4], "wb");
    if (!f || fwrite(q.data(), 1, q.size(), f) != q.size() || fwrite(scales.data(), sizeof(float), scales.size(), f) != scales.size()) {
        fprintf(stderr, "kvq_probe: cannot write %s\n", argv[4]);
        return 1;
    }
    fclose(f);
    return 0;
}
