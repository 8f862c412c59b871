// kv_shift.h — the context shift of a KV lane (zgml_hip_kv_shift, include/zgml_hip.h), stated once for host and device.
//
// The column map. With n_filled columns in use, columns [keep + discard, n_filled) go to [keep, n_filled - discard); every other
// byte of the lane keeps its pattern (the kept columns, the stale tail [n_filled - discard, n_cols), the scales of both).
//
// The rotation. A K lane holds keys the `rope` op has already turned by their position's angle (pairs (i, i + hd), hd = d_head / 2:
// oracle/zgml_oracle.c zo_rope). A moved key is turned BACK by `discard` positions: with c[i], s[i] the cosine and sine of that
// angle (the first half of row `discard` of the model's own tables, so whatever base or scaling the tables carry is honoured),
//   lo' = fl(fl(lo * c[i]) + fl(hi * s[i]))        hi' = fl(fl(hi * c[i]) - fl(lo * s[i]))
// every product and every sum rounded to f32 on its own: no FMA on either side (device: __fmul_rn / __fadd_rn / __fsub_rn, which
// the compiler never contracts; host: build with -ffp-contract=off), so a device column equals this header's column to the bit.
// V lanes are never touched arithmetically.
//
// int8 lanes (block 32, kvq.h). A moved K column is dequantised with (float)q * scale — one multiply per value —, rotated as above
// and requantised as a whole with kvq_quantise_column, unchanged: the block maxima are taken over the ROTATED values. The
// truncation of kvq_quantise shrinks magnitudes, so every shift costs an int8 K column up to one quantisation unit per value. A
// moved int8 V column is a copy of its bytes and scales.
//
// Plain C++ besides the host / device marks, so a CPU probe compiles it alone (tests/cpp/kv_shift_probe.cpp); kv_shift.hip's
// kernel calls kvs_rotate / kvs_dequantise / kvq_block_scale / kvq_quantise in its own lane layout.
#pragma once
#include <string.h>

#include "kvq.h"

namespace zgml {

// what the kernel's ascending rounds carry (kv_shift.hip): values of a rotated lane, bytes of a copied one
constexpr uint32_t kKvsRotateRound = 8192;
constexpr uint32_t kKvsCopyRound = 32768;

struct KvsPair {
    float lo, hi;
};
ZGML_KVQ_HD KvsPair kvs_rotate(float lo, float hi, float c, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return KvsPair{__fadd_rn(__fmul_rn(lo, c), __fmul_rn(hi, s)), __fsub_rn(__fmul_rn(hi, c), __fmul_rn(lo, s))};
#else
    const float lc = lo * c, hs = hi * s, hc = hi * c, ls = lo * s;
    return KvsPair{lc + hs, hc - ls};
#endif
}
ZGML_KVQ_HD float kvs_dequantise(int8_t q, float scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn((float)q, scale);
#else
    return (float)q * scale;
#endif
}

// one f32 key column, in place or not (a pair is read whole before it is written)
ZGML_KVQ_HD void kvs_rotate_column(const float* src, uint32_t d_head, const float* c, const float* s, float* dst) {
    const uint32_t hd = d_head / 2;
    for (uint32_t i = 0; i < hd; i++) {
        const KvsPair p = kvs_rotate(src[i], src[i + hd], c[i], s[i]);
        dst[i] = p.lo, dst[i + hd] = p.hi;
    }
}
// one int8 key column: dequantise, rotate, requantise; tmp: d_head floats
ZGML_KVQ_HD void kvs_rotate_column_i8(const int8_t* q, const float* scales, uint32_t d_head, const float* c, const float* s, int8_t* q_out,
                                      float* scales_out, float* tmp) {
    for (uint32_t i = 0; i < d_head; i++) tmp[i] = kvs_dequantise(q[i], scales[i / 32]);
    kvs_rotate_column(tmp, d_head, c, s, tmp);
    kvq_quantise_column(tmp, d_head, 32, q_out, scales_out);
}

// The whole shift of one f32 lane of n_cols columns, in place: ascending columns, so a column is written only after every column
// that still has to be read (all of them lie above it). Host reference of the kernel.
inline void kvs_shift_lane_f32(float* lane, uint32_t d_head, uint32_t keep, uint32_t discard, uint32_t n_filled, bool rotate, const float* c,
                               const float* s) {
    if (!discard) return;
    for (uint32_t col = keep + discard; col < n_filled; col++) {
        const float* src = lane + (size_t)col * d_head;
        float* dst = lane + (size_t)(col - discard) * d_head;
        if (rotate)
            kvs_rotate_column(src, d_head, c, s, dst);
        else
            memmove(dst, src, (size_t)d_head * sizeof(float));
    }
}
// ... of one int8 lane: q [n_cols * d_head], scales [n_cols * d_head / 32]; tmp: d_head floats
inline void kvs_shift_lane_i8(int8_t* q, float* scales, uint32_t d_head, uint32_t keep, uint32_t discard, uint32_t n_filled, bool rotate, const float* c,
                              const float* s, float* tmp) {
    if (!discard) return;
    const uint32_t bpc = d_head / 32;
    for (uint32_t col = keep + discard; col < n_filled; col++) {
        const size_t from = col, to = col - discard;
        if (rotate) {
            kvs_rotate_column_i8(q + from * d_head, scales + from * bpc, d_head, c, s, q + to * d_head, scales + to * bpc, tmp);
        } else {
            memmove(q + to * d_head, q + from * d_head, d_head);
            memmove(scales + to * bpc, scales + from * bpc, bpc * sizeof(float));
        }
    }
}

} // namespace zgml
