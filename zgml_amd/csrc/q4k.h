// q4k.h — GGUF's Q4_K super-block (the public k-quant definition), stated once for host and device. 256 consecutive flat
// elements in 144 bytes:
//   bytes 0..1 d (f16) | 2..3 dmin (f16) | 4..15 scales[12]: eight 6-bit scales sc_j and eight 6-bit mins m_j, one pair per
//   sub-block j = 0..7 of 32 elements | 16..143 qs[128]: element 64 i + l is the low nibble of qs[32 i + l], element
//   64 i + 32 + l the high nibble (i = 0..3, l = 0..31)
//   w = (d * sc_j) * q - (dmin * m_j),   q the nibble itself in 0..15
// d * sc_j and dmin * m_j are products of an f16 and a 6-bit integer: exact in f32, in general not representable in f16. The
// device kernels (sb_kernels.hip) never form w: they sum (x * d * sc_j) * q and x * dmin * m_j apart, the second once per 32 columns.
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#define ZGML_Q4K_HD __host__ __device__ __forceinline__
#else
#define ZGML_Q4K_HD inline
#endif

namespace zgml {

constexpr uint32_t kQ4kBlock = 256;     // elements of a super-block
constexpr uint32_t kQ4kBytes = 144;     // ... and its bytes in the file (ZGML_QW_GGUF_Q4_K_BLOCK_BYTES)
constexpr uint32_t kQ4kSub = 32;        // elements of a sub-block
constexpr uint32_t kQ4kHeaderBytes = 16; // d, dmin, scales[12]

// every f16 (subnormals, infinities and NaNs included) to f32, exactly
ZGML_Q4K_HD float q4k_f16(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half(h));
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, man = h & 0x3FFu;
    uint32_t exp = (h >> 10) & 31u, bits;
    if (exp == 31) {
        bits = sign | 0x7F800000u | (man << 13);
    } else if (exp) {
        bits = sign | ((exp + 112) << 23) | (man << 13);
    } else if (man) { // subnormal: man * 2^-24
        uint32_t m = man;
        exp = 113;
        while (!(m & 0x400u)) m <<= 1, exp--;
        bits = sign | (exp << 23) | ((m & 0x3FFu) << 13);
    } else {
        bits = sign;
    }
    float f;
    memcpy(&f, &bits, 4);
    return f;
#endif
}

struct Q4kPair {
    uint32_t sc, m; // 0..63 each
};
// the 6-bit unpack of sub-block j; `byte(i)` returns scales[i]
template <typename ByteAt>
ZGML_Q4K_HD Q4kPair q4k_scale_min(ByteAt byte, uint32_t j) {
    if (j < 4) return {byte(j) & 63u, byte(j + 4) & 63u};
    return {(byte(j + 4) & 15u) | ((byte(j - 4) >> 6) << 4), (byte(j + 4) >> 4) | ((byte(j) >> 6) << 4)};
}
// the 16-byte header as the device keeps it: four little-endian dwords {d | dmin << 16, scales[0..3], [4..7], [8..11]}
struct Q4kHeader {
    uint32_t w[4];
};
struct Q4kFactors {
    float scale, min; // d * sc_j, dmin * m_j
};
ZGML_Q4K_HD Q4kFactors q4k_factors(const Q4kHeader& h, uint32_t j) {
    // (selects, not an indexed read: the header stays in registers on the device)
    const Q4kPair p = q4k_scale_min([&](uint32_t i) { return ((i < 4 ? h.w[1] : i < 8 ? h.w[2] : h.w[3]) >> (8 * (i & 3))) & 255u; }, j);
    return {q4k_f16((uint16_t)(h.w[0] & 0xFFFFu)) * (float)p.sc, q4k_f16((uint16_t)(h.w[0] >> 16)) * (float)p.m};
}
// nibble of element e (0..255) of a file block
ZGML_Q4K_HD uint32_t q4k_nibble(const uint8_t* block, uint32_t e) {
    return (block[kQ4kHeaderBytes + 32 * (e >> 6) + (e & 31)] >> (4 * ((e >> 5) & 1))) & 15u;
}
// element e of a file block, the value rule in f32 (two roundings: the product and the difference)
ZGML_Q4K_HD float q4k_value(const uint8_t* block, uint32_t e) {
    Q4kHeader h;
    memcpy(h.w, block, kQ4kHeaderBytes);
    const Q4kFactors f = q4k_factors(h, e >> 5);
    return f.scale * (float)q4k_nibble(block, e) - f.min;
}

} // namespace zgml
