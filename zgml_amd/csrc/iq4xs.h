// iq4xs.h — GGUF's IQ4_XS super-block (the public definition), stated once for host and device. 256 consecutive flat elements in
// 136 bytes (a file block is 8-byte aligned):
//   bytes 0..1 d (f16) | 2..3 scales_h (u16, little endian) | 4..7 scales_l[4] | 8..135 qs[128]
//   element e = 32 ib + j (ib in 0..7, j in 0..31):
//     ls  = ((scales_l[ib >> 1] >> 4 (ib & 1)) & 15) | ((scales_h >> 2 ib) & 3) << 4      (0..63)
//     idx = j < 16 ? qs[16 ib + j] & 15 : qs[16 ib + j - 16] >> 4
//     w   = d * (ls - 32) * kvalues[idx]
// The 4-bit field is an INDEX into a table of sixteen signed bytes, not a number: the one non-linear quant of the family. d * (ls - 32)
// is an f16 times an integer of at most 32 in magnitude: exact in f32. Every table value is an integer of at most 127 in magnitude, exact
// in f32 and in bf16, so w in f32 carries one rounding. No index yields 0: a zero weight comes only from ls = 32. The device kernels
// (sb_kernels.hip) look four indices up at a time in registers (sb_codebook4) and multiply by the signed table value, as Q6_K's and
// Q3_K's multiply by their signed integers.
// Plain C++ besides the host / device marks, so the host model builder (host/llama_decode.cpp) compiles it too.
#pragma once
#include "q4k.h" // q4k_f16: every f16 to f32, exactly

namespace zgml {

constexpr uint32_t kIq4xsBlock = 256; // elements of a super-block
constexpr uint32_t kIq4xsBytes = 136; // ... and its bytes in the file (ZGML_QW_GGUF_IQ4_XS_BLOCK_BYTES)
constexpr uint32_t kIq4xsSub = 32;    // elements of a sub-block: one scale
constexpr uint32_t kIq4xsHeaderBytes = 8, kIq4xsQsOffset = 8;

// the table, once. (A local of a constexpr function: host and device both see it, and whatever the device keeps in registers is
// derived from it at compile time: iq4xs_table_dword.)
ZGML_Q4K_HD constexpr int iq4xs_kvalue(uint32_t idx) {
    constexpr int8_t kvalues[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};
    return kvalues[idx];
}
// table entries 4 i .. 4 i + 3 as the bytes of one dword (two's complement), i = 0..3
ZGML_Q4K_HD constexpr uint32_t iq4xs_table_dword(uint32_t i) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; b++) v |= (uint32_t)(uint8_t)iq4xs_kvalue(4 * i + b) << (8 * b);
    return v;
}
// the 8-byte header as the device keeps it: two little-endian dwords {d | scales_h << 16, scales_l[0..3]}. The low nibble of sub-block
// ib sits at bit 4 ib of the second dword (byte ib >> 1, nibble ib & 1), the high pair at bit 16 + 2 ib of the first
ZGML_Q4K_HD int iq4xs_scale(uint32_t h0, uint32_t h1, uint32_t ib) { return (int)(((h1 >> (4 * ib)) & 15u) | (((h0 >> (16 + 2 * ib)) & 3u) << 4)) - 32; }
// d * (ls - 32): exact in f32
ZGML_Q4K_HD float iq4xs_factor(uint32_t h0, uint32_t h1, uint32_t ib) { return q4k_f16((uint16_t)(h0 & 0xFFFFu)) * (float)iq4xs_scale(h0, h1, ib); }
// the table index of element e (0..255) of a file block
ZGML_Q4K_HD uint32_t iq4xs_index(const uint8_t* block, uint32_t e) { return (block[kIq4xsQsOffset + 16 * (e >> 5) + (e & 15)] >> (4 * ((e >> 4) & 1))) & 15u; }
// element e of a file block, the value rule in f32 (one rounding)
ZGML_Q4K_HD float iq4xs_value(const uint8_t* block, uint32_t e) {
    uint32_t h[2];
    memcpy(h, block, kIq4xsHeaderBytes);
    return iq4xs_factor(h[0], h[1], e >> 5) * (float)iq4xs_kvalue(iq4xs_index(block, e));
}

} // namespace zgml
