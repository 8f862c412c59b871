// kv_shift_probe.cpp — the context shift of zgml_amd/csrc/kv_shift.h on the CPU, as a stand-alone program
// (tests/test_kv_shift_host.py compares its output with the numpy model of tests/kv_shift_model.py, to the bit). The header is the
// rule; added here is only the way through it: read a lane image and the two rows, shift the lane in place, write the image.
//   kv_shift_probe <f32|i8> <d_head> <n_cols> <keep> <discard> <n_filled> <rotate 0|1> <rows.f32> <in.bin> <out.bin>
// rows: d_head / 2 cosines, then d_head / 2 sines. An f32 lane image is n_cols columns of d_head floats back to back; an i8 image
// is the quantised cache layout of include/zgml_hip.h — n_cols * d_head int8, then n_cols * d_head / 32 f32 scales.
// Build: g++ -O2 -std=c++17 -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zgml_amd/csrc/kv_shift.h"

static bool read_all(const char* path, void* dst, size_t bytes) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(dst, 1, bytes, f) == bytes;
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "kv_shift_probe: cannot read %zu bytes from %s\n", bytes, path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        fprintf(stderr, "usage: kv_shift_probe <f32|i8> <d_head> <n_cols> <keep> <discard> <n_filled> <rotate 0|1> <rows.f32> <in.bin> <out.bin>\n");
        return 2;
    }
    const bool i8 = !strcmp(argv[1], "i8");
    const uint32_t dh = (uint32_t)atoi(argv[2]), n_cols = (uint32_t)atoi(argv[3]), keep = (uint32_t)atoi(argv[4]), discard = (uint32_t)atoi(argv[5]),
                   n_filled = (uint32_t)atoi(argv[6]);
    const bool rotate = atoi(argv[7]) != 0;
    if (!dh || dh % 2 || (i8 && dh % 32) || !n_cols || n_filled > n_cols || (uint64_t)keep + discard > n_filled) {
        fprintf(stderr, "kv_shift_probe: d_head must be even (i8: a multiple of 32), keep + discard <= n_filled <= n_cols\n");
        return 2;
    }
    std::vector<float> rows(dh);
    const size_t vals = (size_t)n_cols * dh, bytes = i8 ? vals + vals / 32 * sizeof(float) : vals * sizeof(float);
    std::vector<float> img((bytes + 3) / 4); // (float storage: the scales of an i8 image sit 4-byte aligned behind vals % 4 == 0 bytes)
    if (!read_all(argv[8], rows.data(), dh * sizeof(float)) || !read_all(argv[9], img.data(), bytes)) return 1;
    const float *c = rows.data(), *s = rows.data() + dh / 2;
    if (i8) {
        std::vector<float> tmp(dh);
        zgml::kvs_shift_lane_i8((int8_t*)img.data(), img.data() + vals / 4, dh, keep, discard, n_filled, rotate, c, s, tmp.data());
    } else {
        zgml::kvs_shift_lane_f32(img.data(), dh, keep, discard, n_filled, rotate, c, s);
    }
    FILE* f = fopen(argv[10], "wb");
    if (!f || fwrite(img.data(), 1, bytes, f) != bytes) {
        fprintf(stderr, "kv_shift_probe: cannot write %s\n", argv[10]);
        return 1;
    }
    fclose(f);
    return 0;
}
