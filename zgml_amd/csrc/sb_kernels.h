// sb_kernels.h — the GGUF super-block weights on the device (QW_SB4 / QW_SB5 / QW_SB6 / QW_SB3 / QW_SB2 / QW_SB4X = Q4_K / Q5_K / Q6_K /
// Q3_K / Q2_K / IQ4_XS; q4k.h, q5k.h, q6k.h, q3k.h, q2k.h and iq4xs.h state the file formats): what each format states, once, and the
// device functions every super-block kernel is built from. The kernels and their launchers are sb_kernels.hip.
//
// COMMON DEVICE LAYOUT. A weight is cut into ITEMS [N / 32][K]: item (j, k) holds the 32 q of columns 32 j .. 32 j + 31 at row k,
// so 64 consecutive k of one j are contiguous and a wave (lane = k) streams them coalesced. QWeightDev::qs holds the item planes:
//   lo plane, 16 B per item: byte b = low nibble of column b | low nibble of column b + 16 << 4
//   hi plane (Q5_K: 4 B, Q6_K: 8 B per item; Q4_K: none): the bits above the nibble, laid out so that the four q of columns
//   16 h + 4 s .. + 3 (h = 0..1, s = 0..3) come out as ONE dword of bytes by a shift, a mask and an OR (sb_quants)
// Q3_K / Q2_K have a 2-BIT low plane instead, 8 B per item: dword h = columns 16 h .. + 15, bits 2 s .. 2 s + 1 of byte b = column
// 16 h + 4 s + b (Q6_K's high-pair layout), so the four q of a dword come out by one shift and one AND; Q3_K's third bit is a
// 4-byte high plane in Q5_K's layout (sb_quants2).
// IQ4_XS has the 16-byte low plane alone, and its nibbles are INDICES into a table of sixteen signed bytes: the file's 16 qs bytes of a
// sub-block already are the low-plane entry, and sb_codebook4 turns a dword of four indices into a dword of four table bytes in registers.
// QWeightDev::sc holds the FACTOR planes [N / 256][K], one entry per (k, super-block column): Q4_K / Q5_K the file's 16-byte header
// {d, dmin, scales[12]} as it is (Q4kHeader dwords); Q6_K the file's 16 int8 scales (16 B), then a plane of its f16 d (2 B); Q3_K
// the file's twelve scale bytes as they are (12 B), then a plane of d; Q2_K the file's 16 scale bytes, then a plane of d | dmin << 16;
// IQ4_XS the file's 8-byte header {d, scales_h, scales_l[4]} as it is.
//
// ARITHMETIC. y[n] = sum_k (x[k] * d * sc) * (q - bias)  [ -  sum_k x[k] * dmin * m ]. d * sc and dmin * m are formed in f32
// (exact), never rounded to f16. Q4_K / Q5_K: one (d * sc, dmin * m) pair per item, bias 0, the min sum kept apart and formed once
// per 32 columns. Q6_K: two d * sc per item (one per 16 columns), the signed integer q - 32 as the operand (a weight of q = 32
// contributes an exact zero) and nothing summed apart. Q3_K: as Q6_K with q - 4 and d * (sc - 32). Q2_K: two (d * sc, dmin * m)
// pairs per item, bias 0, and TWO min sums per item, one per 16 columns. IQ4_XS: ONE d * (ls - 32) per item and no min; the operand is
// the signed table byte itself (kSbSigned), converted by one sign-extending byte convert.
//
// A FORMAT (Sb4, Sb5, Sb6, Sb3, Sb2, Sb4x below) is a plain struct of constants and static functions, no more: the file block bytes, its planes
// and how qs / sc are cut into them, the high-plane load, quants(), how many d * sc an item has, whether a min sum exists, the
// operand bias, where its factors come from (per 64-k chunk for M > 1, per 256-k round for M = 1), its pack rule, its synth
// pattern and its name. Everything else here is shared: the lane fold, the M = 1 tail through sb_combine, byte -> f32 / bf16 with
// the bias, the three-piece bf16 split, the [column][k] turn and the wave-order fold and store.
#pragma once
#include "iq4xs.h"
#include "q2k.h"
#include "q5k.h"
#include "q6k.h"
#include "sb_combine.h"

namespace zgml {
namespace {

constexpr uint32_t kSbBlock = 256; // columns of a super-block column: one factor entry per k
constexpr uint32_t kSbItem = 32;   // columns of an item
constexpr uint32_t kSbWaves = 8;   // M = 1: waves of a workgroup = item columns of a super-block column
constexpr uint32_t kSbSweep = 64;  // k per wave sweep (one per lane)
constexpr uint32_t kSbSweeps = 4;  // sweeps of a round (Q5_K, Q6_K): all loaded before the first is consumed
constexpr uint32_t kSbRound = kSbSweep * kSbSweeps; // k of a round = rows of the factors in LDS
constexpr uint32_t kSbRowsPerGroup = 4; // 2 <= M <= 8: rows of a row group (128 of a wave's 256 VGPRs are its accumulators)
static_assert(kQ4kBlock == kSbBlock && kQ5kBlock == kSbBlock && kQ6kBlock == kSbBlock && kQ4kSub == kSbItem && kQ5kSub == kSbItem && 2 * kQ6kSub == kSbItem, "");
static_assert(kQ3kBlock == kSbBlock && kQ2kBlock == kSbBlock && 2 * kQ3kSub == kSbItem && 2 * kQ2kSub == kSbItem, "");
static_assert(kIq4xsBlock == kSbBlock && kIq4xsSub == kSbItem, "");
static_assert(kSbWaves * kSbItem == kSbBlock && kSbWaves * 64 == 2 * kSbRound, "the factor duty of a round: one k and half of its factors per thread");

typedef float sb_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 sb_bf8 __attribute__((ext_vector_type(8)));

// ── shared device functions ──────────────────────────────────────────────────────────────────
// the 32 q of an item as eight dwords of four bytes: dword 4 h + s = columns 16 h + 4 s .. + 3. `hi0` / `hi1`: the high bits of
// columns 0..15 / 16..31, BITS of them per column at bit BITS * s of byte b (BITS = 0: no high plane)
template <uint32_t BITS>
__device__ __forceinline__ void sb_quants(uint4 lo, uint32_t hi0, uint32_t hi1, uint32_t (&q)[8]) {
    constexpr uint32_t mask = ((1u << BITS) - 1u) * 0x01010101u;
    const uint32_t l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        q[s] = l[s] & 0x0f0f0f0fu;
        q[4 + s] = (l[s] >> 4) & 0x0f0f0f0fu;
        if constexpr (BITS != 0) {
            q[s] |= ((hi0 >> (BITS * s)) & mask) << 4;
            q[4 + s] |= ((hi1 >> (BITS * s)) & mask) << 4;
        }
    }
}
// the 2-bit low plane: the same eight dwords from 8 bytes. dword 4 h + s = (lo_h >> 2 s) & 3 per byte; HIGH: bit 4 h + s of byte b of
// `hi` is the third bit of column 16 h + 4 s + b, moved to bit 2 by one shift and taken in by one AND-OR. 14 (+ 16) VALU per item
template <bool HIGH>
__device__ __forceinline__ void sb_quants2(uint2 lo, uint32_t hi, uint32_t (&q)[8]) {
    const uint32_t l[2] = {lo.x, lo.y};
#pragma unroll
    for (int d = 0; d < 8; d++) {
        q[d] = (l[d >> 2] >> (2 * (d & 3))) & 0x03030303u;
        if constexpr (HIGH) q[d] |= (d >= 2 ? hi >> (d - 2) : hi << (2 - d)) & 0x04040404u;
        asm("" : "+v"(q[d])); // keep the dword of four bytes: left to itself hipcc takes every 2-bit field out of `lo` on its own (one v_bfe per weight)
    }
}
// the Q4_K / Q5_K header of one (k, super-block column) -> (d * sc, dmin * m) of sub-block j
__device__ __forceinline__ Q4kFactors sb_header_factors(uint4 h, uint32_t j) { return q4k_factors(Q4kHeader{{h.x, h.y, h.z, h.w}}, j); }

// IQ4_XS: a dword of four table indices (0..15 each, as sb_quants<0> leaves them) -> the dword of their four signed table bytes.
// The table is four dword constants; v_perm_b32 picks any byte of a register pair by a selector byte 0..7 (larger selectors mean
// other things to the instruction, hence idx & 7): one perm over entries 0..7, one over 8..15, and a third perm takes byte b from the
// second where bit 3 of index b is set (selector b or 4 + b). Six VALU per four weights, no LDS table, no per-weight lookup. (The third
// perm stands where a bit-field insert under a byte mask would: its selector is a shift and an AND-OR, the mask a shift, an AND, a
// shift and a subtraction.)
__device__ __forceinline__ uint32_t sb_codebook4(uint32_t idx) {
    constexpr uint32_t t0 = iq4xs_table_dword(0), t1 = iq4xs_table_dword(1), t2 = iq4xs_table_dword(2), t3 = iq4xs_table_dword(3);
    const uint32_t sel = idx & 0x07070707u;
    const uint32_t low = __builtin_amdgcn_perm(t1, t0, sel), high = __builtin_amdgcn_perm(t3, t2, sel);
    return __builtin_amdgcn_perm(high, low, ((idx >> 1) & 0x04040404u) | 0x03020100u);
}

// byte b of a quant dword as the f32 operand q - BIAS; BIAS = kSbSigned: the byte is a signed value itself
constexpr int kSbSigned = -1;
template <int BIAS>
__device__ __forceinline__ float sb_operand(uint32_t dword, int b) {
    if constexpr (BIAS == kSbSigned) return (float)(int)(int8_t)(dword >> (8 * b));
    const float q = (float)((dword >> (8 * b)) & 255u);
    if constexpr (BIAS != 0) return q - (float)BIAS;
    return q;
}

// M = 1: the 32 per-lane column sums of wave w -> red[column] (red = the wave's row): halves (16 registers, half h holds column
// 2 m + h), rows (8 registers, row r holds column 4 n + 2 (r & 1) + (r >> 1)), then the 16 lanes of a row; MIN: less the min
// sum over all 64 lanes — one per item (NS = 1) or one per column half (NS = 2: columns 16 h .. + 15 are registers i = 4 h .. + 3)
template <bool MIN, int NS>
__device__ __forceinline__ void sb_fold_lanes(const float (&acc)[32], const float (&macc)[NS], float (&red)[kSbItem], uint32_t r, uint32_t i) {
    float b16[16];
#pragma unroll
    for (int m = 0; m < 16; m++) b16[m] = kon_fold32(acc[2 * m], acc[2 * m + 1]);
    float c8[8];
#pragma unroll
    for (int n = 0; n < 8; n++) c8[n] = row16_sum(kon_fold16(b16[2 * n], b16[2 * n + 1]));
    float mins = 0.f;
    if constexpr (MIN) mins = rows_sum4(row16_sum(macc[0]));
    if constexpr (MIN && NS == 2) {
        const float mins1 = rows_sum4(row16_sum(macc[1]));
        mins = i >= 4 ? mins1 : mins;
    }
    float v = c8[0];
#pragma unroll
    for (int n = 1; n < 8; n++) v = i == (uint32_t)n ? c8[n] : v;
    if (i < 8) red[4 * i + 2 * (r & 1) + (r >> 1)] = MIN ? v - mins : v;
}
// M = 1: red -> y, one column per thread 0..255 -> the parts combined in part order (sb_combine) -> dst. (The column test is
// written out three times on purpose: named once, hipcc merges the split and the unsplit store of dst, which is another tail
// than the Q4_K kernel has had since its measurements.)
template <class Args>
__device__ __forceinline__ void sb_matvec_tail(const Args& a, const float (&red)[kSbWaves][kSbItem], uint32_t* flag, uint32_t nsb, uint32_t part) {
    __syncthreads();
    const uint32_t n = nsb * kSbBlock + threadIdx.x;
    float y = threadIdx.x < kSbBlock ? red[threadIdx.x >> 5][threadIdx.x & 31] : 0.f;
    if (a.parts > 1 && !sb_combine(y, threadIdx.x < kSbBlock, a.partial, a.counter + nsb, part, a.parts, a.N, n, flag)) return;
    if (threadIdx.x < kSbBlock) a.dst[n] = y;
}
// 2 <= M <= 8 rows: the same tail over the R rows of a row group that starts at row m0 (`rows` of them live). red[rr] is row rr's
// M = 1 red; the 512 threads take one column and every second row each, and the group's parts meet on the group's own counter word
template <int R, class Args>
__device__ __forceinline__ void sb_rows_tail(const Args& a, const float (&red)[R][kSbWaves][kSbItem], uint32_t* flag, uint32_t nsb, uint32_t part, uint32_t m0,
                                             uint32_t rows) {
    __syncthreads();
    const uint32_t col = threadIdx.x & (kSbBlock - 1), odd = threadIdx.x >> 8, n = nsb * kSbBlock + col;
    float y[R];
#pragma unroll
    for (int rr = 0; rr < R; rr++) y[rr] = red[rr][col >> 5][col & 31];
    if (a.parts > 1 && !sb_combine_rows<R>(y, odd, rows, a.partial + (uint64_t)m0 * a.N, (uint64_t)a.M * a.N, a.counter + blockIdx.z * (a.N / kSbBlock) + nsb, part,
                                           a.parts, a.N, n, flag))
        return;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
        if ((rr & 1) == (int)odd && rr < (int)rows) a.dst[(uint64_t)(m0 + rr) * a.dst_rs + n] = y[rr];
}

// M > 1: a wave's own LDS slice: its DS operations run in order, so a wave barrier is all that a write -> read (or read -> next
// write) hand-over needs
__device__ __forceinline__ void sb_wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the turn: byte c of lane k's ND dwords -> turned[c][k], so that lane (r, i) of the MFMA reads 8 consecutive k of one byte
// column as ONE 8-byte LDS read (sb_turned8)
template <int ND>
__device__ __forceinline__ void sb_turn(uint8_t* turned, const uint32_t (&q)[ND], uint32_t lane) {
#pragma unroll
    for (int dd = 0; dd < ND; dd++)
#pragma unroll
        for (int b = 0; b < 4; b++) turned[(4 * dd + b) * 64 + lane] = (uint8_t)(q[dd] >> (8 * b));
}
__device__ __forceinline__ uint2 sb_turned8(const uint8_t* turned, uint32_t c, uint32_t kl) { return *(const uint2*)&turned[c * 64 + kl]; }
// ... and those 8 bytes as the bf16 B fragment q - BIAS (exact in bf16)
template <int BIAS>
__device__ __forceinline__ sb_bf8 sb_fragment(uint2 bb) {
    const uint32_t bw[2] = {bb.x, bb.y};
    sb_bf8 qv;
#pragma unroll
    for (int e = 0; e < 8; e++) qv[e] = (__bf16)sb_operand<BIAS>(bw[e >> 2], e & 3);
    return qv;
}
// 8 consecutive f32 of LDS / 8 consecutive x of a row (k = kb .. kb + 7, zero past K) as an array
__device__ __forceinline__ void sb_read8(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
template <bool XVEC>
__device__ __forceinline__ void sb_load_x8(const float* xrow, uint32_t kb, uint32_t K, float (&v)[8]) {
    const float4 a = zero_tail(load_x4<XVEC>(xrow, kb, K), kb, K), b = zero_tail(load_x4<XVEC>(xrow, kb + 4, K), kb + 4, K);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
// element e of the A operand: t = x * (d * sc) in f32 as three bf16 pieces, t = h1 + h2 + h3 up to 2^-26 |t|
__device__ __forceinline__ void sb_split3(float t, sb_bf8& h1, sb_bf8& h2, sb_bf8& h3, int e) {
    h1[e] = (__bf16)t;
    const float r1 = t - (float)h1[e];
    h2[e] = (__bf16)r1;
    const float r2 = r1 - (float)h2[e];
    h3[e] = (__bf16)r2;
}
__device__ __forceinline__ sb_f4 sb_mfma3(sb_bf8 h1, sb_bf8 h2, sb_bf8 h3, sb_bf8 qv, sb_f4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, qv, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, qv, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, qv, acc, 0, 0, 0);
}
// M > 1, the end of a workgroup of WAVES waves that owns item column j and RT row tiles from row m0: D[m = 4 r + v][n = i] of
// tile t = 2 rt + ct is in acc[rt][ct][v]; MIN: the min sum of row i over the four lane rows — one per row tile (NS = 1) or one
// per (row tile, column tile) (NS = 2: a column tile is a scale sub-block with a min of its own); then the waves in wave order
template <uint32_t WAVES, int RT, bool MIN, int NS, class Args>
__device__ __forceinline__ void sb_fold_waves(const Args& a, float (&fold)[WAVES][RT * 2][4][64], float (&mins)[WAVES][RT * NS][16], const sb_f4 (&acc)[RT][2],
                                              const float (&macc)[RT][NS], uint32_t j, uint32_t m0) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < RT * 2; t++)
#pragma unroll
        for (int v = 0; v < 4; v++) fold[w][t][v][lane] = acc[t >> 1][t & 1][v];
    if constexpr (MIN) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int h = 0; h < NS; h++) {
                const float mrow = rows_sum4(macc[rt][h]);
                if (lane >> 4 == 0) mins[w][rt * NS + h][lane & 15] = mrow;
            }
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < RT * 2 * 256; idx += WAVES * 64) {
        const uint32_t t = idx >> 8, rt = RT > 1 ? t >> 1 : 0, v = (idx >> 6) & 3, l = idx & 63, ml = 4 * (l >> 4) + v;
        const uint32_t rn = NS == 2 ? t : rt; // (t = 2 rt + ct)
        float sum = fold[0][t][v][l], mn = 0.f;
        if constexpr (MIN) mn = mins[0][rn][ml];
        for (uint32_t ww = 1; ww < WAVES; ww++) {
            sum += fold[ww][t][v][l];
            if constexpr (MIN) mn += mins[ww][rn][ml];
        }
        const uint32_t m = m0 + 16 * rt + ml, n = j * kSbItem + (t & 1) * 16 + (l & 15);
        if (m < a.M) a.dst[(uint64_t)m * a.dst_rs + n] = MIN ? sum - mn : sum;
    }
}

// ── the formats ──────────────────────────────────────────────────────────────────────────────
// Common members. kItemBytes / kFactorBytes: packed bytes per item / per (k, super-block column). Planes + planes(): the cut of
// qs / sc; at(): every item plane advanced by `item` entries, every factor plane by `factor`. kScales: d * sc per item.
// kRound: served by the shared round / 8-wave kernels (else Q4_K's own bodies). kNtMaxM: the largest M whose M > 1 launch may
// stream the weights non-temporally (beyond it several workgroup rows re-read them: keep them cached).
// pack_item() / pack_factors(): item `idx` = (sub-block js, k) / the factor entry `fidx` from file block `blk`. synth(): the
// deterministic pattern of the micro-benchmark, in the packed layout (every q; sc and m over their ranges; d = 2^-10).
// kRowsRoutedM: the largest M ZGML_HIP_OPT_SMALL_M_MATVEC = 1 routes to the row kernels (measured per format).
// chunk_factors(): the item's factor rows at row k: f[kScales] = d * sc (of the item, or of columns 0..15 and 16..31), mn[kScales] =
// dmin * m beside each (kMin).
// Round kernels only: Lo / Hi + load_lo() / load_hi(): an item's low and high plane entries (Hi = SbNoHi: none); RoundLds: the round's factors in LDS; round_load() / round_store(): the duty of thread
// (kl, half) — one k of the round, half of its factors — from memory to LDS; item_factors(): the t = x * d * sc of wave w's
// item at row kl (and its FMAs into the kScales min sums).
struct Sb4 {
    static constexpr QWFormat kFormat = QW_SB4;
    static constexpr const char* kName = "Q4_K";
    static constexpr uint32_t kFileBytes = kQ4kBytes, kItemBytes = 16, kFactorBytes = kQ4kHeaderBytes; // 4.5 bit/weight like the file
    static constexpr uint32_t kScales = 1, kNtMaxM = 16;
    static constexpr uint32_t kRowsRoutedM = 3;
    static constexpr bool kMin = true, kRound = false;
    static constexpr int kBias = 0;
    struct Planes {
        uint4* lo;
        uint4* hdr;
    };
    static Planes planes(const QWeightDev& w) { return {(uint4*)w.qs, (uint4*)w.sc}; }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.hdr + factor}; }
    __device__ static __forceinline__ void quants(uint4 lo, uint32_t (&q)[8]) { sb_quants<0>(lo, 0, 0, q); }
    // (144 = 9 * 16: every file block is 16-byte aligned.) The file keeps sub-blocks 2 i and 2 i + 1 in the two nibbles of the
    // same 32 bytes; an item takes one of them: bytes l = 0..15 and 16..31 of the pair, nibble js & 1
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        const uint4* src = (const uint4*)(blk + kQ4kHeaderBytes + 32 * (js >> 1));
        const uint4 lo = src[0], hi = src[1];
        const uint32_t sh = 4 * (js & 1), mask = 0x0f0f0f0fu;
        o.lo[idx] = make_uint4(((lo.x >> sh) & mask) | (((hi.x >> sh) & mask) << 4), ((lo.y >> sh) & mask) | (((hi.y >> sh) & mask) << 4),
                               ((lo.z >> sh) & mask) | (((hi.z >> sh) & mask) << 4), ((lo.w >> sh) & mask) | (((hi.w >> sh) & mask) << 4));
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) { o.hdr[fidx] = *(const uint4*)blk; }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) {
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        if (factors) o.hdr[idx] = make_uint4(0x90001400u /* d = 2^-10, dmin = -2^-11 */, a, a * 11u, a * 13u);
    }
};

struct Sb5 {
    static constexpr QWFormat kFormat = QW_SB5;
    static constexpr const char* kName = "Q5_K";
    static constexpr uint32_t kFileBytes = kQ5kBytes, kItemBytes = 16 + 4, kFactorBytes = kQ4kHeaderBytes; // 5.5 bit/weight like the file
    static constexpr uint32_t kScales = 1, kNtMaxM = 32;
    static constexpr uint32_t kRowsRoutedM = 4;
    static constexpr bool kMin = true, kRound = true;
    static constexpr int kBias = 0;
    using Hi = uint32_t; // bit 4 h + s of byte b = high bit of column 16 h + 4 s + b
    struct Planes {
        uint4* lo;
        Hi* hi;
        uint4* hdr;
    };
    static Planes planes(const QWeightDev& w) {
        uint4* lo = (uint4*)w.qs;
        return {lo, (Hi*)(lo + (uint64_t)w.K * (w.N / kSbItem)), (uint4*)w.sc};
    }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.hi + item, p.hdr + factor}; }
    using Lo = uint4;
    template <bool NT>
    __device__ static __forceinline__ Lo load_lo(const Planes& c, uint32_t k) {
        return wload<NT>(c.lo + k);
    }
    template <bool NT>
    __device__ static __forceinline__ Hi load_hi(const Planes& c, uint32_t k) {
        return wload1<NT>(c.hi + k);
    }
    __device__ static __forceinline__ void quants(uint4 lo, Hi hi, uint32_t (&q)[8]) { sb_quants<1>(lo, hi, hi >> 4, q); }
    __device__ static __forceinline__ void chunk_factors(const Planes& c, uint32_t k, uint32_t js, float (&f)[1], float (&mn)[1]) {
        const Q4kFactors hf = sb_header_factors(c.hdr[k], js);
        f[0] = hf.scale, mn[0] = hf.min;
    }
    // [sub-block][k] of 8-byte (d * sc, dmin * m) pairs: a wave reads its own sub-block's pair of 64 k as one conflict-free 8-byte
    // read per lane. A thread turns four of its k's eight sub-blocks
    using RoundLds = float2[kSbWaves][kSbRound];
    using RoundRaw = uint4; // the header
    __device__ static __forceinline__ RoundRaw round_load(const Planes& c, uint32_t k, uint32_t) { return c.hdr[k]; }
    __device__ static __forceinline__ void round_store(RoundLds& fac, const RoundRaw& raw, uint32_t kl, uint32_t half, bool live) {
        if (half == 0) { // (the same for a whole wave; the sub-block is a constant in each arm, so q4k_factors' selects fold away)
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                const Q4kFactors f = sb_header_factors(raw, e);
                fac[e][kl] = live ? make_float2(f.scale, f.min) : make_float2(0.f, 0.f);
            }
        } else {
#pragma unroll
            for (uint32_t e = 4; e < 8; e++) {
                const Q4kFactors f = sb_header_factors(raw, e);
                fac[e][kl] = live ? make_float2(f.scale, f.min) : make_float2(0.f, 0.f);
            }
        }
    }
    __device__ static __forceinline__ void item_factors(const RoundLds& fac, uint32_t w, uint32_t kl, float x, float (&t)[1], float (&macc)[1]) {
        const float2 f = fac[w][kl];
        t[0] = x * f.x;
        macc[0] = __builtin_fmaf(x, f.y, macc[0]);
    }
    // the file block is read by bytes (only 2-byte aligned) through q5k.h's own rule
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        uint32_t lo[4] = {0, 0, 0, 0}, hi = 0;
#pragma unroll
        for (uint32_t c = 0; c < 32; c++) {
            const uint32_t q = q5k_quant(blk, 32 * js + c), h = c >> 4, s = (c >> 2) & 3, b = c & 3;
            lo[s] |= (q & 15u) << (8 * b + 4 * h);
            hi |= (q >> 4) << (8 * b + 4 * h + s);
        }
        o.lo[idx] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        o.hi[idx] = hi;
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) {
        uint32_t hw[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t e = 0; e < kQ4kHeaderBytes; e++) hw[e >> 2] |= (uint32_t)blk[e] << (8 * (e & 3));
        o.hdr[fidx] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
    }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) {
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        o.hi[idx] = a * 17u + 4u;
        if (factors) o.hdr[idx] = make_uint4(0x90001400u /* d = 2^-10, dmin = -2^-11 */, a, a * 11u, a * 13u);
    }
};

struct Sb6 {
    static constexpr QWFormat kFormat = QW_SB6;
    static constexpr const char* kName = "Q6_K";
    static constexpr uint32_t kFileBytes = kQ6kBytes, kItemBytes = 16 + 8, kFactorBytes = 16 + 2; // 6.5625 bit/weight like the file
    static constexpr uint32_t kScales = 2, kNtMaxM = 32;
    static constexpr uint32_t kRowsRoutedM = 4;
    static constexpr bool kMin = false, kRound = true;
    static constexpr int kBias = 32;
    using Hi = uint2; // dword h (columns 16 h .. 16 h + 15), byte b, bits 2 s .. 2 s + 1 = high pair of column 16 h + 4 s + b
    struct Planes {
        uint4* lo;
        Hi* hi;
        uint4* sc;
        uint16_t* d;
    };
    static Planes planes(const QWeightDev& w) {
        uint4* lo = (uint4*)w.qs;
        uint4* sc = (uint4*)w.sc;
        return {lo, (Hi*)(lo + (uint64_t)w.K * (w.N / kSbItem)), sc, (uint16_t*)(sc + (uint64_t)w.K * (w.N / kSbBlock))};
    }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.hi + item, p.sc + factor, p.d + factor}; }
    using Lo = uint4;
    template <bool NT>
    __device__ static __forceinline__ Lo load_lo(const Planes& c, uint32_t k) {
        return wload<NT>(c.lo + k);
    }
    template <bool NT>
    __device__ static __forceinline__ Hi load_hi(const Planes& c, uint32_t k) {
        return wload2<NT>(c.hi + k);
    }
    __device__ static __forceinline__ void quants(uint4 lo, Hi hi, uint32_t (&q)[8]) { sb_quants<2>(lo, hi.x, hi.y, q); }
    __device__ static __forceinline__ float product(float d, uint32_t scale_byte) { return d * (float)(int)(int8_t)scale_byte; }
    __device__ static __forceinline__ void chunk_factors(const Planes& c, uint32_t k, uint32_t js, float (&f)[2], float (&)[2]) {
        const uint32_t sc2 = ((const uint16_t*)(c.sc + k))[js]; // the scales of columns 32 js .. + 15 and + 16 .. + 31
        const float d = q4k_f16(c.d[k]);
        f[0] = product(d, sc2 & 255u), f[1] = product(d, sc2 >> 8);
    }
    // [scale][k] of d * sc, so a wave reads its two scales of 64 k without a bank conflict. A thread turns eight of its k's sixteen
    // scale bytes
    using RoundLds = float[16][kSbRound];
    struct RoundRaw {
        uint2 sbytes;
        uint32_t dbits;
    };
    __device__ static __forceinline__ RoundRaw round_load(const Planes& c, uint32_t k, uint32_t half) { return {((const uint2*)(c.sc + k))[half], c.d[k]}; }
    __device__ static __forceinline__ void round_store(RoundLds& ds, const RoundRaw& raw, uint32_t kl, uint32_t half, bool live) {
        const float d = q4k_f16((uint16_t)raw.dbits);
#pragma unroll
        for (uint32_t e = 0; e < 8; e++) {
            const float ds_e = product(d, ((e < 4 ? raw.sbytes.x : raw.sbytes.y) >> (8 * (e & 3))) & 255u);
            ds[half * 8 + e][kl] = live ? ds_e : 0.f;
        }
    }
    __device__ static __forceinline__ void item_factors(const RoundLds& ds, uint32_t w, uint32_t kl, float x, float (&t)[2], float (&)[2]) {
        t[0] = x * ds[2 * w][kl];
        t[1] = x * ds[2 * w + 1][kl];
    }
    // the file block is read by bytes (210 is no multiple of 4) through q6k.h's own rule
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        uint32_t lo[4] = {0, 0, 0, 0}, hi[2] = {0, 0};
#pragma unroll
        for (uint32_t c = 0; c < 32; c++) {
            const uint32_t q = q6k_quant(blk, 32 * js + c), b = c & 15;
            lo[b >> 2] |= (q & 15u) << (8 * (b & 3) + 4 * (c >> 4));
            hi[c >> 4] |= (q >> 4) << (8 * (c & 3) + 2 * (b >> 2));
        }
        o.lo[idx] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        o.hi[idx] = make_uint2(hi[0], hi[1]);
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) {
        uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t e = 0; e < 16; e++) s[e >> 2] |= (uint32_t)blk[kQ6kScaleOffset + e] << (8 * (e & 3));
        o.sc[fidx] = make_uint4(s[0], s[1], s[2], s[3]);
        o.d[fidx] = (uint16_t)(blk[kQ6kDOffset] | blk[kQ6kDOffset + 1] << 8);
    }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) { // (scales over the int8 range)
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        o.hi[idx] = make_uint2(a * 17u + 4u, a * 19u + 5u);
        if (factors) {
            o.sc[idx] = make_uint4(a * 23u, a * 11u, a * 13u, a * 29u);
            o.d[idx] = 0x1400;
        }
    }
};

// the 2-bit-plane formats. Their item is 8 (+ 4) bytes, so a 256-k round holds 2 / 3.25 KiB per wave in flight
struct SbNoHi {}; // Q2_K: no high plane, nothing loaded
// an 8-byte low-plane entry from the 32 two-bit fields `low(c)` of an item's columns
template <class Low>
__device__ __forceinline__ uint2 sb_pack_lo2(Low low) {
    uint32_t lo[2] = {0, 0};
#pragma unroll
    for (uint32_t c = 0; c < 32; c++) lo[c >> 4] |= low(c) << (8 * (c & 3) + 2 * ((c >> 2) & 3));
    return make_uint2(lo[0], lo[1]);
}

struct Sb3 {
    static constexpr QWFormat kFormat = QW_SB3;
    static constexpr const char* kName = "Q3_K";
    static constexpr uint32_t kFileBytes = kQ3kBytes, kItemBytes = 8 + 4, kFactorBytes = 12 + 2; // 3.4375 bit/weight like the file
    static constexpr uint32_t kScales = 2, kNtMaxM = 32;
    static constexpr uint32_t kRowsRoutedM = 4;
    static constexpr bool kMin = false, kRound = true;
    static constexpr int kBias = 4;
    using Lo = uint2;
    using Hi = uint32_t; // bit 4 h + s of byte b = third bit of column 16 h + 4 s + b (Q5_K's layout)
    struct Sc12 {       // the file's twelve scale bytes
        uint32_t x, y, z;
    };
    struct Planes {
        Lo* lo;
        Hi* hi;
        Sc12* sc;
        uint16_t* d;
    };
    static Planes planes(const QWeightDev& w) {
        Lo* lo = (Lo*)w.qs;
        Sc12* sc = (Sc12*)w.sc;
        return {lo, (Hi*)(lo + (uint64_t)w.K * (w.N / kSbItem)), sc, (uint16_t*)(sc + (uint64_t)w.K * (w.N / kSbBlock))};
    }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.hi + item, p.sc + factor, p.d + factor}; }
    template <bool NT>
    __device__ static __forceinline__ Lo load_lo(const Planes& c, uint32_t k) {
        return wload2<NT>(c.lo + k);
    }
    template <bool NT>
    __device__ static __forceinline__ Hi load_hi(const Planes& c, uint32_t k) {
        return wload1<NT>(c.hi + k);
    }
    __device__ static __forceinline__ void quants(Lo lo, Hi hi, uint32_t (&q)[8]) { sb_quants2<true>(lo, hi, q); }
    __device__ static __forceinline__ float product(float d, uint32_t sc) { return d * (float)((int)sc - 32); }
    __device__ static __forceinline__ void chunk_factors(const Planes& c, uint32_t k, uint32_t js, float (&f)[2], float (&)[2]) {
        const uint32_t* r = (const uint32_t*)(c.sc + k); // bytes 0..7 as one 64-bit value, 8..11 as a dword: shifts, nothing indexed
        const uint64_t r8 = r[0] | (uint64_t)r[1] << 32;
        const uint32_t r4 = r[2];
        const float d = q4k_f16(c.d[k]);
        const auto byte = [&](uint32_t i) { return (i < 8 ? (uint32_t)(r8 >> (8 * i)) : r4 >> (8 * (i & 3))) & 255u; };
        f[0] = product(d, q3k_scale(byte, 2 * js)), f[1] = product(d, q3k_scale(byte, 2 * js + 1));
    }
    // [scale][k] of d * (sc - 32), as Q6_K. A thread turns eight of its k's sixteen scales: the eight 6-bit values of its half
    // come out of the twelve bytes as two dwords of bytes by 4 shifts, 4 ANDs and 2 shift-ORs, ten VALU in all
    using RoundLds = float[16][kSbRound];
    struct RoundRaw {
        Sc12 s;
        uint32_t dbits;
    };
    __device__ static __forceinline__ RoundRaw round_load(const Planes& c, uint32_t k, uint32_t) { return {c.sc[k], c.d[k]}; }
    __device__ static __forceinline__ void round_store(RoundLds& ds, const RoundRaw& raw, uint32_t kl, uint32_t half, bool live) {
        const float d = q4k_f16((uint16_t)raw.dbits);
        const uint32_t sh = 4 * half; // scales 8 half + e: nibble `half` of byte e, top bits 4 half + 2 (e >> 2) of byte 8 + (e & 3)
        const uint32_t sc[2] = {((raw.s.x >> sh) & 0x0f0f0f0fu) | (((raw.s.z >> sh) & 0x03030303u) << 4),
                                ((raw.s.y >> sh) & 0x0f0f0f0fu) | (((raw.s.z >> (sh + 2)) & 0x03030303u) << 4)};
#pragma unroll
        for (uint32_t e = 0; e < 8; e++) {
            const float ds_e = product(d, (sc[e >> 2] >> (8 * (e & 3))) & 255u);
            ds[half * 8 + e][kl] = live ? ds_e : 0.f;
        }
    }
    __device__ static __forceinline__ void item_factors(const RoundLds& ds, uint32_t w, uint32_t kl, float x, float (&t)[2], float (&)[2]) {
        t[0] = x * ds[2 * w][kl];
        t[1] = x * ds[2 * w + 1][kl];
    }
    // the file block is read by bytes (only 2-byte aligned) through q3k.h's own rule
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        uint32_t hi = 0;
#pragma unroll
        for (uint32_t c = 0; c < 32; c++) hi |= q3k_high(blk, 32 * js + c) << (8 * (c & 3) + 4 * (c >> 4) + ((c >> 2) & 3));
        o.lo[idx] = sb_pack_lo2([&](uint32_t c) { return q3k_low(blk, 32 * js + c); });
        o.hi[idx] = hi;
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) {
        uint32_t s[3] = {0, 0, 0};
#pragma unroll
        for (uint32_t e = 0; e < 12; e++) s[e >> 2] |= (uint32_t)blk[kQ3kScaleOffset + e] << (8 * (e & 3));
        o.sc[fidx] = Sc12{s[0], s[1], s[2]};
        o.d[fidx] = (uint16_t)(blk[kQ3kDOffset] | blk[kQ3kDOffset + 1] << 8);
    }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) {
        o.lo[idx] = make_uint2(a, a * 3u + 1u);
        o.hi[idx] = a * 17u + 4u;
        if (factors) {
            o.sc[idx] = Sc12{a * 23u, a * 11u, a * 13u};
            o.d[idx] = 0x1400;
        }
    }
};

struct Sb2 {
    static constexpr QWFormat kFormat = QW_SB2;
    static constexpr const char* kName = "Q2_K";
    static constexpr uint32_t kFileBytes = kQ2kBytes, kItemBytes = 8, kFactorBytes = 16 + 4; // 2.625 bit/weight like the file
    static constexpr uint32_t kScales = 2, kNtMaxM = 32;
    static constexpr uint32_t kRowsRoutedM = 6;
    static constexpr bool kMin = true, kRound = true;
    static constexpr int kBias = 0;
    using Lo = uint2;
    using Hi = SbNoHi;
    struct Planes {
        Lo* lo;
        uint4* sc;    // the file's sixteen (scale, min) nibble pairs
        uint32_t* dm; // d | dmin << 16
    };
    static Planes planes(const QWeightDev& w) {
        uint4* sc = (uint4*)w.sc;
        return {(Lo*)w.qs, sc, (uint32_t*)(sc + (uint64_t)w.K * (w.N / kSbBlock))};
    }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.sc + factor, p.dm + factor}; }
    template <bool NT>
    __device__ static __forceinline__ Lo load_lo(const Planes& c, uint32_t k) {
        return wload2<NT>(c.lo + k);
    }
    template <bool NT>
    __device__ static __forceinline__ Hi load_hi(const Planes&, uint32_t) {
        return {};
    }
    __device__ static __forceinline__ void quants(Lo lo, Hi, uint32_t (&q)[8]) { sb_quants2<false>(lo, 0, q); }
    __device__ static __forceinline__ void chunk_factors(const Planes& c, uint32_t k, uint32_t js, float (&f)[2], float (&mn)[2]) {
        const uint32_t sc2 = ((const uint16_t*)(c.sc + k))[js], dm = c.dm[k]; // the pairs of columns 32 js .. + 15 and + 16 .. + 31
        const Q4kFactors f0 = q2k_factors(sc2 & 255u, dm), f1 = q2k_factors(sc2 >> 8, dm);
        f[0] = f0.scale, f[1] = f1.scale, mn[0] = f0.min, mn[1] = f1.min;
    }
    // [scale][k] of 8-byte (d * sc, dmin * m) pairs: a wave reads the two pairs of its item over 64 k as two conflict-free 8-byte
    // reads per lane. A thread turns eight of its k's sixteen scale bytes
    using RoundLds = float2[16][kSbRound];
    struct RoundRaw {
        uint2 sbytes;
        uint32_t dm;
    };
    __device__ static __forceinline__ RoundRaw round_load(const Planes& c, uint32_t k, uint32_t half) { return {((const uint2*)(c.sc + k))[half], c.dm[k]}; }
    __device__ static __forceinline__ void round_store(RoundLds& fac, const RoundRaw& raw, uint32_t kl, uint32_t half, bool live) {
#pragma unroll
        for (uint32_t e = 0; e < 8; e++) {
            const Q4kFactors f = q2k_factors(((e < 4 ? raw.sbytes.x : raw.sbytes.y) >> (8 * (e & 3))) & 255u, raw.dm);
            fac[half * 8 + e][kl] = live ? make_float2(f.scale, f.min) : make_float2(0.f, 0.f);
        }
    }
    __device__ static __forceinline__ void item_factors(const RoundLds& fac, uint32_t w, uint32_t kl, float x, float (&t)[2], float (&macc)[2]) {
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const float2 f = fac[2 * w + h][kl];
            t[h] = x * f.x;
            macc[h] = __builtin_fmaf(x, f.y, macc[h]);
        }
    }
    // (84 = 21 * 4: every file block is 4-byte aligned; the items go through q2k.h's own rule)
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        o.lo[idx] = sb_pack_lo2([&](uint32_t c) { return q2k_quant(blk, 32 * js + c); });
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) {
        const uint32_t* src = (const uint32_t*)blk;
        o.sc[fidx] = make_uint4(src[0], src[1], src[2], src[3]);
        o.dm[fidx] = src[kQ2kDOffset / 4];
    }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) {
        o.lo[idx] = make_uint2(a, a * 3u + 1u);
        if (factors) {
            o.sc[idx] = make_uint4(a * 23u, a * 11u, a * 13u, a * 29u);
            o.dm[idx] = 0x90001400u; // d = 2^-10, dmin = -2^-11
        }
    }
};

// IQ4_XS: Q4_K's bytes per item, the codebook in place of the nibble's own value, one scale per item and no min
struct Sb4x {
    static constexpr QWFormat kFormat = QW_SB4X;
    static constexpr const char* kName = "IQ4_XS";
    static constexpr uint32_t kFileBytes = kIq4xsBytes, kItemBytes = 16, kFactorBytes = kIq4xsHeaderBytes; // 4.25 bit/weight like the file
    static constexpr uint32_t kScales = 1, kNtMaxM = 32;
    static constexpr uint32_t kRowsRoutedM = 3;
    static constexpr bool kMin = false, kRound = true;
    static constexpr int kBias = kSbSigned;
    using Lo = uint4;
    using Hi = SbNoHi;
    struct Planes {
        Lo* lo;
        uint2* hdr; // d | scales_h << 16, scales_l[4]
    };
    static Planes planes(const QWeightDev& w) { return {(Lo*)w.qs, (uint2*)w.sc}; }
    __device__ static __forceinline__ Planes at(Planes p, uint64_t item, uint64_t factor) { return {p.lo + item, p.hdr + factor}; }
    template <bool NT>
    __device__ static __forceinline__ Lo load_lo(const Planes& c, uint32_t k) {
        return wload<NT>(c.lo + k);
    }
    template <bool NT>
    __device__ static __forceinline__ Hi load_hi(const Planes&, uint32_t) {
        return {};
    }
    // the indices, then the table bytes: what the FMAs convert and what the turn leaves in LDS are table values
    __device__ static __forceinline__ void quants(Lo lo, Hi, uint32_t (&q)[8]) {
        sb_quants<0>(lo, 0, 0, q);
#pragma unroll
        for (int d = 0; d < 8; d++) q[d] = sb_codebook4(q[d]);
    }
    __device__ static __forceinline__ void chunk_factors(const Planes& c, uint32_t k, uint32_t js, float (&f)[1], float (&)[1]) {
        const uint2 h = c.hdr[k];
        f[0] = iq4xs_factor(h.x, h.y, js);
    }
    // [sub-block][k] of d * (ls - 32): a wave reads its own sub-block's factor of 64 k as one conflict-free read per lane. A thread turns
    // the four scales of its half: the header shifted once by the half, then constant fields
    using RoundLds = float[kSbWaves][kSbRound];
    using RoundRaw = uint2; // the header
    __device__ static __forceinline__ RoundRaw round_load(const Planes& c, uint32_t k, uint32_t) { return c.hdr[k]; }
    __device__ static __forceinline__ void round_store(RoundLds& ds, const RoundRaw& raw, uint32_t kl, uint32_t half, bool live) {
        const float d = q4k_f16((uint16_t)(raw.x & 0xFFFFu));
        const uint32_t h0 = raw.x >> (8 * half), h1 = raw.y >> (16 * half); // sub-block 4 half + e: iq4xs_scale's fields of e
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const float ds_e = d * (float)iq4xs_scale(h0, h1, e);
            ds[half * 4 + e][kl] = live ? ds_e : 0.f;
        }
    }
    __device__ static __forceinline__ void item_factors(const RoundLds& ds, uint32_t w, uint32_t kl, float x, float (&t)[1], float (&)[1]) { t[0] = x * ds[w][kl]; }
    // (136 = 17 * 8: every file block is 8-byte aligned.) The file's 16 qs bytes of sub-block js are the low-plane entry as it is: byte
    // b = index of column b | index of column b + 16 << 4
    __device__ static __forceinline__ void pack_item(const uint8_t* blk, uint32_t js, const Planes& o, uint64_t idx) {
        const uint2* src = (const uint2*)(blk + kIq4xsQsOffset + 16 * js);
        const uint2 a = src[0], b = src[1];
        o.lo[idx] = make_uint4(a.x, a.y, b.x, b.y);
    }
    __device__ static __forceinline__ void pack_factors(const uint8_t* blk, const Planes& o, uint64_t fidx) { o.hdr[fidx] = *(const uint2*)blk; }
    __device__ static __forceinline__ void synth(const Planes& o, uint64_t idx, uint32_t a, bool factors) { // (every index; ls over its range)
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        if (factors) o.hdr[idx] = make_uint2(0x1400u /* d = 2^-10 */ | (a * 23u << 16), a * 11u);
    }
};

} // namespace
} // namespace zgml
