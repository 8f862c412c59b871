// q6k.h — GGUF's Q6_K super-block (the public k-quant definition), stated once for host and device. 256 consecutive flat
// elements in 210 bytes (a file block is only 2-byte aligned):
//   bytes 0..127 ql[128] | 128..191 qh[64] | 192..207 scales[16], int8 | 208..209 d (f16)
//   element e = 128 h + 32 g + l (h in 0..1, g in 0..3, l in 0..31):
//     low nibble = (ql[64 h + 32 (g & 1) + l] >> 4 (g >> 1)) & 15,  high bits = (qh[32 h + l] >> 2 g) & 3,
//     q = low | high << 4 in 0..63,   w = (d * scales[e >> 4]) * (q - 32)
// d * scale is an f16 times an int8: exact in f32. q - 32 is an exact small integer in f32 and in bf16, so w in f32 carries one
// rounding. The -32 is NOT part of a second sum (as Q4_K's min is): the device kernels (sb_kernels.hip) multiply by the signed integer.
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include "q4k.h" // q4k_f16: every f16 to f32, exactly

namespace zgml {

constexpr uint32_t kQ6kBlock = 256;       // elements of a super-block
constexpr uint32_t kQ6kBytes = 210;       // ... and its bytes in the file (ZGML_QW_GGUF_Q6_K_BLOCK_BYTES)
constexpr uint32_t kQ6kSub = 16;          // elements that share a scale
constexpr uint32_t kQ6kQhOffset = 128, kQ6kScaleOffset = 192, kQ6kDOffset = 208;

// the 6-bit q of element e (0..255) of a file block
ZGML_Q4K_HD uint32_t q6k_quant(const uint8_t* block, uint32_t e) {
    const uint32_t h = e >> 7, g = (e >> 5) & 3, l = e & 31;
    const uint32_t low = (block[64 * h + 32 * (g & 1) + l] >> (4 * (g >> 1))) & 15u;
    const uint32_t high = (block[kQ6kQhOffset + 32 * h + l] >> (2 * g)) & 3u;
    return low | (high << 4);
}
// d * scales[s], s = 0..15: exact in f32
ZGML_Q4K_HD float q6k_factor(const uint8_t* block, uint32_t s) {
    return q4k_f16((uint16_t)(block[kQ6kDOffset] | block[kQ6kDOffset + 1] << 8)) * (float)(int8_t)block[kQ6kScaleOffset + s];
}
// element e of a file block, the value rule in f32 (one rounding)
ZGML_Q4K_HD float q6k_value(const uint8_t* block, uint32_t e) {
    return q6k_factor(block, e >> 4) * (float)((int)q6k_quant(block, e) - 32);
}

} // namespace zgml
