// q2k.h — GGUF's Q2_K super-block (the public k-quant definition), stated once for host and device. 256 consecutive flat
// elements in 84 bytes (every file block is 4-byte aligned):
//   bytes 0..15 scales[16]: sub-block s = e >> 4 has the 4-bit scale scales[s] & 15 and the 4-bit min scales[s] >> 4 |
//   16..79 qs[64] | 80..81 d (f16) | 82..83 dmin (f16)
//   element e (0..255): q = (qs[32 (e >> 7) + (e & 31)] >> 2 ((e >> 5) & 3)) & 3 in 0..3 (q3k.h: k2_field)
//   w = d * (scales[s] & 15) * q - dmin * (scales[s] >> 4)
// Both products are an f16 times a 4-bit integer: exact in f32. The device kernels (sb_kernels.hip) never form w: they sum
// (x * d * sc_s) * q and x * dmin * m_s apart, the second once per 16 columns (Q4_K's arithmetic at Q6_K's scale granularity).
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include "q3k.h" // k2_field; q4k.h: q4k_f16, Q4kFactors

namespace zgml {

constexpr uint32_t kQ2kBlock = 256; // elements of a super-block
constexpr uint32_t kQ2kBytes = 84;  // ... and its bytes in the file (ZGML_QW_GGUF_Q2_K_BLOCK_BYTES)
constexpr uint32_t kQ2kSub = 16;    // elements that share a (scale, min) pair
constexpr uint32_t kQ2kQsOffset = 16, kQ2kDOffset = 80;

// the 2-bit q of element e (0..255) of a file block
ZGML_Q4K_HD uint32_t q2k_quant(const uint8_t* block, uint32_t e) { return k2_field(block + kQ2kQsOffset, e); }
// (d * sc_s, dmin * m_s) from the scale byte of a sub-block and the dword d | dmin << 16
ZGML_Q4K_HD Q4kFactors q2k_factors(uint32_t scale_byte, uint32_t d_dmin) {
    return {q4k_f16((uint16_t)(d_dmin & 0xFFFFu)) * (float)(scale_byte & 15u), q4k_f16((uint16_t)(d_dmin >> 16)) * (float)((scale_byte >> 4) & 15u)};
}
// element e of a file block, the value rule in f32 (two roundings: the product and the difference)
ZGML_Q4K_HD float q2k_value(const uint8_t* block, uint32_t e) {
    uint32_t dm;
    memcpy(&dm, block + kQ2kDOffset, 4);
    const Q4kFactors f = q2k_factors(block[e >> 4], dm);
    return f.scale * (float)q2k_quant(block, e) - f.min;
}

} // namespace zgml
