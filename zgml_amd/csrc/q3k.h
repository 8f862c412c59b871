// q3k.h — GGUF's Q3_K super-block (the public k-quant definition), stated once for host and device. 256 consecutive flat
// elements in 110 bytes (a file block is only 2-byte aligned, so it is read by bytes):
//   bytes 0..31 hmask[32] | 32..95 qs[64] | 96..107 scales[12] | 108..109 d (f16)
//   element e (0..255):
//     low  = (qs[32 (e >> 7) + (e & 31)] >> 2 ((e >> 5) & 3)) & 3      (the 2-bit rule Q2_K shares: q2k.h)
//     high = (hmask[e & 31] >> (e >> 5)) & 1
//     q = low + 4 high - 4 in -4..3
//   the 6-bit scale of sub-block s = e >> 4 (sixteen of 16 elements): low 4 bits scales[s] & 15 (s < 8) or scales[s - 8] >> 4,
//   high 2 bits (scales[8 + (s & 3)] >> 2 (s >> 2)) & 3;   w = d * (sc_s - 32) * q
// d * (sc - 32) is an f16 times an integer of at most 32 in magnitude: exact in f32. q is an exact small integer in f32 and in
// bf16, so w in f32 carries one rounding. The device kernels (sb_kernels.hip) multiply by the signed integer, as Q6_K's do.
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include "q4k.h" // q4k_f16: every f16 to f32, exactly

namespace zgml {

constexpr uint32_t kQ3kBlock = 256; // elements of a super-block
constexpr uint32_t kQ3kBytes = 110; // ... and its bytes in the file (ZGML_QW_GGUF_Q3_K_BLOCK_BYTES)
constexpr uint32_t kQ3kSub = 16;    // elements that share a scale
constexpr uint32_t kQ3kQsOffset = 32, kQ3kScaleOffset = 96, kQ3kDOffset = 108;

// the 2-bit field of element e in a 64-byte qs array (Q3_K's low bits, Q2_K's q)
ZGML_Q4K_HD uint32_t k2_field(const uint8_t* qs, uint32_t e) { return (qs[32 * (e >> 7) + (e & 31)] >> (2 * ((e >> 5) & 3))) & 3u; }
// the low two bits / the high bit of element e (0..255) of a file block, and the signed q
ZGML_Q4K_HD uint32_t q3k_low(const uint8_t* block, uint32_t e) { return k2_field(block + kQ3kQsOffset, e); }
ZGML_Q4K_HD uint32_t q3k_high(const uint8_t* block, uint32_t e) { return (block[e & 31] >> (e >> 5)) & 1u; }
ZGML_Q4K_HD int q3k_quant(const uint8_t* block, uint32_t e) { return (int)(q3k_low(block, e) + 4u * q3k_high(block, e)) - 4; }
// the 6-bit scale of sub-block s = 0..15; `byte(i)` returns scales[i]
template <typename ByteAt>
ZGML_Q4K_HD uint32_t q3k_scale(ByteAt byte, uint32_t s) {
    const uint32_t low = s < 8 ? byte(s) & 15u : byte(s - 8) >> 4;
    return low | (((byte(8 + (s & 3)) >> (2 * (s >> 2))) & 3u) << 4);
}
// d * (sc_s - 32): exact in f32
ZGML_Q4K_HD float q3k_factor(const uint8_t* block, uint32_t s) {
    const uint32_t sc = q3k_scale([&](uint32_t i) { return (uint32_t)block[kQ3kScaleOffset + i]; }, s);
    return q4k_f16((uint16_t)(block[kQ3kDOffset] | block[kQ3kDOffset + 1] << 8)) * (float)((int)sc - 32);
}
// element e of a file block, the value rule in f32 (one rounding)
ZGML_Q4K_HD float q3k_value(const uint8_t* block, uint32_t e) { return q3k_factor(block, e >> 4) * (float)q3k_quant(block, e); }

} // namespace zgml
