// q5k.h — GGUF's Q5_K super-block (the public k-quant definition), stated once for host and device. 256 consecutive flat
// elements in 176 bytes (a file block is only 2-byte aligned, so it is read by bytes):
//   bytes 0..1 d (f16) | 2..3 dmin (f16) | 4..15 scales[12]: Q4_K's eight 6-bit (sc_j, m_j) pairs (q4k_scale_min) |
//   16..47 qh[32] | 48..175 qs[128]
//   element e = 32 j + l (j in 0..7, l in 0..31):
//     nibble = (qs[32 (j >> 1) + l] >> 4 (j & 1)) & 15 (Q4_K's rule),  high bit = (qh[l] >> j) & 1,
//     q = nibble | high << 4 in 0..31,   w = (d * sc_j) * q - dmin * m_j
// d * sc_j and dmin * m_j are exact in f32 (q4k.h). The device kernels (sb_kernels.hip) never form w: they sum (x * d * sc_j) * q and
// x * dmin * m_j apart, the second once per 32 columns, as Q4_K's do.
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include "q4k.h" // q4k_f16, Q4kHeader, q4k_factors: the 16-byte header is Q4_K's

namespace zgml {

constexpr uint32_t kQ5kBlock = 256; // elements of a super-block
constexpr uint32_t kQ5kBytes = 176; // ... and its bytes in the file (ZGML_QW_GGUF_Q5_K_BLOCK_BYTES)
constexpr uint32_t kQ5kSub = 32;    // elements of a sub-block: one (sc, m) pair
constexpr uint32_t kQ5kQhOffset = 16, kQ5kQsOffset = 48;

// the 5-bit q of element e (0..255) of a file block
ZGML_Q4K_HD uint32_t q5k_quant(const uint8_t* block, uint32_t e) {
    const uint32_t j = e >> 5, l = e & 31;
    const uint32_t nibble = (block[kQ5kQsOffset + 32 * (j >> 1) + l] >> (4 * (j & 1))) & 15u;
    const uint32_t high = (block[kQ5kQhOffset + l] >> j) & 1u;
    return nibble | (high << 4);
}
// element e of a file block, the value rule in f32 (two roundings: the product and the difference)
ZGML_Q4K_HD float q5k_value(const uint8_t* block, uint32_t e) {
    Q4kHeader h;
    memcpy(h.w, block, kQ4kHeaderBytes);
    const Q4kFactors f = q4k_factors(h, e >> 5);
    return f.scale * (float)q5k_quant(block, e) - f.min;
}

} // namespace zgml
