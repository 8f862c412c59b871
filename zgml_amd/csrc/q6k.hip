// q6k.hip — GGUF Q6_K weights on the device (QW_SB6, "super-block 6-bit"; q6k.h states the format): the re-pack of the file's
// 210-byte super-blocks, the M = 1 mat-vec and the M > 1 matmul on the matrix cores. With q4k.hip it shares the K-split fan-in
// (sb_combine.h) and nothing else.
//
// DEVICE LAYOUT (6.5625 bit/weight like the file: 128 + 64 B of quants, 16 B of scales and 2 B of d per (k, 256 columns))
//   qs: two planes of ITEMS [N / 32][K]; item (j, k) holds the 32 q of columns 32 j .. 32 j + 31 at row k:
//       lo plane, 16 B: byte b = low nibble of column b | low nibble of column b + 16 << 4
//       hi plane,  8 B: dword h (columns 16 h .. 16 h + 15), byte b, bits 2 s .. 2 s + 1 = high pair of column 16 h + 4 s + b
//       so the four q of columns 16 h + 4 s .. + 3 are ONE dword of bytes: ((lo[s] >> 4 h) & 0x0f0f0f0f) | ((hi[h] >> 2 s) & 0x03030303) << 4
//   sc: two planes [N / 256][K]: the file's 16 int8 scales (16 B), then its f16 d (2 B)
//
// ARITHMETIC (both kernels): y[n] = sum_k (x[k] * d * sc) * (q - 32), the signed integer as the operand: a weight of q = 32
// contributes an exact zero, and nothing is summed apart. d * sc is formed in f32 (exact).
//
// M = 1 (sb6_matvec_kernel): a workgroup of 8 waves owns one super-block column and one K share; wave w streams item column w,
// lane = k. The share is walked in ROUNDS of four 64-k sweeps, and a round issues every load it has — the workgroup's scale
// bytes and d first, then per wave four lo items, four hi items and four x — before anything is consumed: 6 KiB in flight per
// wave. While the items fly the 512 threads turn the round's 256 x 16 scale bytes into f32 products d * sc in LDS, once per
// workgroup ([scale][k], so a wave reads its two scales of 64 k without a bank conflict); a 32-column item has two
// t = x * d * sc, one per 16 columns. Per weight: byte -> f32, - 32, FMA into 32 per-lane column sums, folded over the lanes in
// a fixed tree. K is split over blockIdx.y into parts of whole rounds until the grid has about two workgroups per CU (one
// round per part where that is not reached, at most 16 parts); parts are combined in part order by sb_combine.
//
// M > 1 (sb6_matmul_kernel<RT>): a workgroup of 8 waves owns one item column (32 output columns = two 16-column MFMA tiles, each
// exactly one scale sub-block) and RT = 1 or 2 row tiles of 16; the waves deal the 64-k chunks. Per chunk a wave loads 64 items
// coalesced, assembles the q bytes, turns them ONCE through its own LDS slice into [column][k] order and leaves the chunk's
// 2 x 64 products d * sc beside them; the x rows are loaded once per 32-k step. Both are then shared by every tile the workgroup
// owns: the B operand (q - 32, exact in bf16) of a column tile serves both row tiles, the x of a row tile both column tiles.
// A = t = x * (d * sc) in f32 is per (row tile, column tile), split into three bf16 pieces (t = h1 + h2 + h3 up to 2^-26 |t|)
// and contracted by v_mfma_f32_16x16x32_bf16 with f32 accumulation: three MFMAs per tile and 32 k. Waves are folded in wave order.
#include "q6k.h"
#include "sb_combine.h"

namespace zgml {
namespace {

constexpr uint32_t kS6Waves = 8;          // M = 1: waves of a workgroup = item columns of a super-block column
constexpr uint32_t kS6Sweep = 64;         // k per wave sweep (one per lane)
constexpr uint32_t kS6Sweeps = 4;         // sweeps of a round: all loaded before the first is consumed (28 VGPRs)
constexpr uint32_t kS6Round = kS6Sweep * kS6Sweeps; // k of a round = rows of the scale products in LDS
constexpr uint32_t kS6TargetWaves = 4096; // 256 CUs x 2 workgroups x 8 waves: split K until the grid has this many waves ...
constexpr uint32_t kS6MaxParts = 16;      // ... but into at most this many parts (two batches of the combine)
constexpr uint32_t kS6MmWaves = 8;        // M > 1: waves of a workgroup, dealing the 64-k chunks

typedef float sb6_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 sb6_bf8 __attribute__((ext_vector_type(8)));

struct S6Planes {
    uint4* lo;
    uint2* hi;
    uint4* sc;
    uint16_t* d;
};
S6Planes s6_planes(const QWeightDev& w) {
    uint4* lo = (uint4*)w.qs;
    uint4* sc = (uint4*)w.sc;
    return {lo, (uint2*)(lo + (uint64_t)w.K * (w.N / 32)), sc, (uint16_t*)(sc + (uint64_t)w.K * (w.N / kQ6kBlock))};
}

template <bool NT>
__device__ __forceinline__ uint2 wload2(const uint2* p) {
    if (NT) {
        typedef unsigned int u2v __attribute__((ext_vector_type(2)));
        const u2v v = __builtin_nontemporal_load((const u2v*)p);
        return make_uint2(v.x, v.y);
    }
    return *p;
}

// the 32 q of an item as eight dwords of four bytes: dword 4 h + s = columns 16 h + 4 s .. + 3
__device__ __forceinline__ void s6_quants(uint4 lo, uint2 hi, uint32_t (&q)[8]) {
    const uint32_t l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        q[s] = (l[s] & 0x0f0f0f0fu) | (((hi.x >> (2 * s)) & 0x03030303u) << 4);
        q[4 + s] = ((l[s] >> 4) & 0x0f0f0f0fu) | (((hi.y >> (2 * s)) & 0x03030303u) << 4);
    }
}
__device__ __forceinline__ float s6_product(float d, uint32_t scale_byte) { return d * (float)(int)(int8_t)scale_byte; }

// ── re-pack: one thread per item; the file block is read by bytes (210 is no multiple of 4) through q6k.h's own rule ──
__global__ void __launch_bounds__(kBlock) pack_sb6_kernel(const uint8_t* __restrict__ raw, S6Planes o, uint32_t K, uint32_t N) {
    const uint64_t total = (uint64_t)K * (N / 32);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(idx / K), k = (uint32_t)(idx % K), nsb = j >> 3, js = j & 7;
        const uint8_t* blk = raw + ((uint64_t)k * (N / kQ6kBlock) + nsb) * kQ6kBytes;
        uint32_t lo[4] = {0, 0, 0, 0}, hi[2] = {0, 0};
#pragma unroll
        for (uint32_t c = 0; c < 32; c++) {
            const uint32_t q = q6k_quant(blk, 32 * js + c), b = c & 15;
            lo[b >> 2] |= (q & 15u) << (8 * (b & 3) + 4 * (c >> 4));
            hi[c >> 4] |= (q >> 4) << (8 * (c & 3) + 2 * (b >> 2));
        }
        o.lo[idx] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        o.hi[idx] = make_uint2(hi[0], hi[1]);
        if (js == 0) {
            uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t e = 0; e < 16; e++) s[e >> 2] |= (uint32_t)blk[kQ6kScaleOffset + e] << (8 * (e & 3));
            o.sc[(uint64_t)nsb * K + k] = make_uint4(s[0], s[1], s[2], s[3]);
            o.d[(uint64_t)nsb * K + k] = (uint16_t)(blk[kQ6kDOffset] | blk[kQ6kDOffset + 1] << 8);
        }
    }
}

// deterministic synthetic weights for the micro-benchmark, in the packed layout: every q, scales over the int8 range, d = 2^-10
__global__ void __launch_bounds__(kBlock) synth_sb6_kernel(S6Planes o, uint32_t K, uint32_t N, uint32_t id) {
    const uint64_t total = (uint64_t)K * (N / 32);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t a = (uint32_t)idx * 2654435761u + id * 40503u;
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        o.hi[idx] = make_uint2(a * 17u + 4u, a * 19u + 5u);
        if (idx < (uint64_t)K * (N / kQ6kBlock)) {
            o.sc[idx] = make_uint4(a * 23u, a * 11u, a * 13u, a * 29u);
            o.d[idx] = 0x1400;
        }
    }
}

// ── M = 1 ──
struct S6MvArgs {
    S6Planes w;
    const float* x;
    float* dst;
    float* partial;    // [parts][N] (parts > 1)
    uint32_t* counter; // [N / 256] fan-in words, zero between launches
    uint32_t K, N, share, parts;
};

template <bool NT>
__global__ void __launch_bounds__(kS6Waves * 64) sb6_matvec_kernel(S6MvArgs a) {
    __shared__ float ds[16][kS6Round]; // d * sc of the round: [scale][k]
    __shared__ float red[kS6Waves][32];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y;
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const uint4* items_lo = a.w.lo + (uint64_t)(nsb * kS6Waves + w) * a.K;
    const uint2* items_hi = a.w.hi + (uint64_t)(nsb * kS6Waves + w) * a.K;
    const uint4* scs = a.w.sc + (uint64_t)nsb * a.K;
    const uint16_t* dsrc = a.w.d + (uint64_t)nsb * a.K;
    const uint32_t skl = threadIdx.x & (kS6Round - 1), shalf = threadIdx.x >> 8; // scale duty: one k, eight of its sixteen scales

    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = 0.f;
    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += kS6Round) {
        // every load of the round, the scales first (their wait then leaves the items in flight); past the share: a live
        // address again, with x = 0 and d * sc = 0
        const uint32_t ks = min(k0 + skl, k_hi - 1);
        const uint2 sbytes = ((const uint2*)(scs + ks))[shalf];
        const uint32_t dbits = dsrc[ks];
        uint4 ql[kS6Sweeps];
        uint2 qh[kS6Sweeps];
        float xs[kS6Sweeps];
#pragma unroll
        for (uint32_t s = 0; s < kS6Sweeps; s++) {
            const uint32_t k = k0 + s * kS6Sweep + lane, kc = min(k, k_hi - 1);
            ql[s] = wload<NT>(items_lo + kc);
            qh[s] = wload2<NT>(items_hi + kc);
            xs[s] = k < k_hi ? a.x[kc] : 0.f;
        }
        const float d = q4k_f16((uint16_t)dbits);
        const bool slive = k0 + skl < k_hi;
#pragma unroll
        for (uint32_t e = 0; e < 8; e++)
            ds[shalf * 8 + e][skl] = slive ? s6_product(d, ((e < 4 ? sbytes.x : sbytes.y) >> (8 * (e & 3))) & 255u) : 0.f;
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < kS6Sweeps; s++) {
            if (k0 + s * kS6Sweep >= k_hi) break; // (the same for the whole workgroup)
            const uint32_t kl = s * kS6Sweep + lane;
            const float t[2] = {xs[s] * ds[2 * w][kl], xs[s] * ds[2 * w + 1][kl]};
            uint32_t q[8];
            s6_quants(ql[s], qh[s], q);
#pragma unroll
            for (int dd = 0; dd < 8; dd++)
#pragma unroll
                for (int b = 0; b < 4; b++)
                    acc[4 * dd + b] = __builtin_fmaf(t[dd >> 2], (float)((q[dd] >> (8 * b)) & 255u) - 32.f, acc[4 * dd + b]);
        }
        __syncthreads(); // the next round rewrites ds
    }

    // 32 sums per lane -> columns: halves (16 registers, half h holds column 2 m + h), rows (8 registers, row r holds column
    // 4 n + 2 (r & 1) + (r >> 1)), then the 16 lanes of a row
    float b16[16];
#pragma unroll
    for (int m = 0; m < 16; m++) b16[m] = kon_fold32(acc[2 * m], acc[2 * m + 1]);
    float c8[8];
#pragma unroll
    for (int n = 0; n < 8; n++) c8[n] = row16_sum(kon_fold16(b16[2 * n], b16[2 * n + 1]));
    float v = c8[0];
#pragma unroll
    for (int n = 1; n < 8; n++) v = i == (uint32_t)n ? c8[n] : v;
    if (i < 8) red[w][4 * i + 2 * (r & 1) + (r >> 1)] = v;
    __syncthreads();

    const bool live = threadIdx.x < kQ6kBlock; // threads 0..255: one column each
    const uint32_t n = nsb * kQ6kBlock + threadIdx.x;
    float y = live ? red[threadIdx.x >> 5][threadIdx.x & 31] : 0.f;
    if (a.parts > 1 && !sb_combine(y, live, a.partial, a.counter + nsb, part, a.parts, a.N, n, &flag)) return;
    if (live) a.dst[n] = y;
}

// the K split of an M = 1 launch: parts and the k of each (whole rounds)
struct S6Split {
    uint32_t parts, share;
};
S6Split sb6_split(uint32_t K, uint32_t N) {
    const uint32_t rounds = cdiv(K, kS6Round), want = cdiv(kS6TargetWaves, N / 32);
    const uint32_t per = std::max(cdiv(rounds, want), cdiv(rounds, kS6MaxParts));
    const uint32_t parts = N / kQ6kBlock <= kQmmCounterBytes / 4 ? cdiv(rounds, per) : 1; // (one counter word per super-block column)
    return parts > 1 ? S6Split{parts, per * kS6Round} : S6Split{1, rounds * kS6Round};
}

// ── M > 1 ──
struct S6MmArgs {
    S6Planes w;
    const float* x;
    float* dst;
    uint32_t M, K, N, in_rs, dst_rs;
};

template <int RT, bool XVEC, bool NT>
__global__ void __launch_bounds__(kS6MmWaves * 64) sb6_matmul_kernel(S6MmArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t turned[kS6MmWaves][32 * 64]; // per wave: the chunk's q bytes, [column][k]
    __shared__ __attribute__((aligned(16))) float fs[kS6MmWaves][2][64];         // ... and its d * sc, [column tile][k]
    __shared__ float fold[kS6MmWaves][RT * 2][4][64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t j = blockIdx.x, nsb = j >> 3, js = j & 7, m0 = blockIdx.y * 16 * RT;
    const uint4* items_lo = a.w.lo + (uint64_t)j * a.K;
    const uint2* items_hi = a.w.hi + (uint64_t)j * a.K;
    const uint4* scs = a.w.sc + (uint64_t)nsb * a.K;
    const uint16_t* dsrc = a.w.d + (uint64_t)nsb * a.K;
    const float* xrow[RT]; // A operand: lane (r, i) holds row i, k = 8 r .. 8 r + 7 of a 32-k step
    sb6_f4 acc[RT][2];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        xrow[rt] = a.x + (uint64_t)min(m0 + 16 * rt + i, a.M - 1) * a.in_rs;
        acc[rt][0] = acc[rt][1] = sb6_f4{0.f, 0.f, 0.f, 0.f};
    }
    const uint32_t chunks = (a.K + 63) / 64;
    for (uint32_t c = w; c < chunks; c += kS6MmWaves) {
        const uint32_t k = c * 64 + lane, kc = min(k, a.K - 1);
        const uint4 lo = wload<NT>(items_lo + kc);
        const uint2 hi = wload2<NT>(items_hi + kc);
        const uint32_t sc2 = ((const uint16_t*)(scs + kc))[js]; // the scales of columns 32 js .. + 15 and + 16 .. + 31
        const float d = q4k_f16(dsrc[kc]);
        fs[w][0][lane] = k < a.K ? s6_product(d, sc2 & 255u) : 0.f; // rows past K: t = 0
        fs[w][1][lane] = k < a.K ? s6_product(d, sc2 >> 8) : 0.f;
        uint32_t q[8];
        s6_quants(lo, hi, q);
#pragma unroll
        for (int dd = 0; dd < 8; dd++)
#pragma unroll
            for (int b = 0; b < 4; b++) turned[w][(4 * dd + b) * 64 + lane] = (uint8_t)(q[dd] >> (8 * b));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the wave's own LDS slice: its DS operations run in order
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t kl = 32 * s + 8 * r, kb = c * 64 + kl;
            float xv[RT][8];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const float4 xa = zero_tail(load_x4<XVEC>(xrow[rt], kb, a.K), kb, a.K), xb = zero_tail(load_x4<XVEC>(xrow[rt], kb + 4, a.K), kb + 4, a.K);
                xv[rt][0] = xa.x, xv[rt][1] = xa.y, xv[rt][2] = xa.z, xv[rt][3] = xa.w, xv[rt][4] = xb.x, xv[rt][5] = xb.y, xv[rt][6] = xb.z, xv[rt][7] = xb.w;
            }
#pragma unroll
            for (int ct = 0; ct < 2; ct++) {
                const uint2 bb = *(const uint2*)&turned[w][(16 * ct + i) * 64 + kl];
                const float4 sa = *(const float4*)&fs[w][ct][kl], sb = *(const float4*)&fs[w][ct][kl + 4];
                const float sv[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
                const uint32_t bw[2] = {bb.x, bb.y};
                sb6_bf8 qv;
#pragma unroll
                for (int e = 0; e < 8; e++) qv[e] = (__bf16)((float)((bw[e >> 2] >> (8 * (e & 3))) & 255u) - 32.f); // column 16 ct + i
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    sb6_bf8 h1, h2, h3;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float t = xv[rt][e] * sv[e];
                        h1[e] = (__bf16)t;
                        const float r1 = t - (float)h1[e];
                        h2[e] = (__bf16)r1;
                        const float r2 = r1 - (float)h2[e];
                        h3[e] = (__bf16)r2;
                    }
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, qv, acc[rt][ct], 0, 0, 0);
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, qv, acc[rt][ct], 0, 0, 0);
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, qv, acc[rt][ct], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the reads above stay above the next chunk's writes
        __builtin_amdgcn_wave_barrier();
    }
    // D[m = 4 r + v][n = i] in acc[v]; the waves in wave order
#pragma unroll
    for (int t = 0; t < RT * 2; t++)
#pragma unroll
        for (int v = 0; v < 4; v++) fold[w][t][v][lane] = acc[t >> 1][t & 1][v];
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < RT * 2 * 256; idx += kS6MmWaves * 64) {
        const uint32_t t = idx >> 8, v = (idx >> 6) & 3, l = idx & 63;
        float sum = fold[0][t][v][l];
        for (uint32_t ww = 1; ww < kS6MmWaves; ww++) sum += fold[ww][t][v][l];
        const uint32_t m = m0 + 16 * (t >> 1) + 4 * (l >> 4) + v, n = j * 32 + (t & 1) * 16 + (l & 15);
        if (m < a.M) a.dst[(uint64_t)m * a.dst_rs + n] = sum;
    }
}

template <int RT, bool XVEC>
void launch_mm(hipStream_t s, const S6MmArgs& a, bool nt) {
    const dim3 grid(a.N / 32, cdiv(a.M, 16 * RT));
    if (nt)
        sb6_matmul_kernel<RT, XVEC, true><<<grid, kS6MmWaves * 64, 0, s>>>(a);
    else
        sb6_matmul_kernel<RT, XVEC, false><<<grid, kS6MmWaves * 64, 0, s>>>(a);
}

} // namespace

bool sb6_applies(uint64_t K, uint64_t N) { return sb4_applies(K, N); }

void sb6_packed_bytes(uint64_t K, uint64_t N, uint64_t* qs_bytes, uint64_t* sc_bytes) {
    *qs_bytes = K * (N / 32) * (16 + 8);
    *sc_bytes = K * (N / kQ6kBlock) * (16 + 2);
}

void launch_pack_sb6(hipStream_t s, const uint8_t* raw_blocks, const QWeightDev& out) {
    pack_sb6_kernel<<<2048, kBlock, 0, s>>>(raw_blocks, s6_planes(out), out.K, out.N);
}

void launch_synth_sb6(hipStream_t s, const QWeightDev& w, uint32_t matrix_id) {
    synth_sb6_kernel<<<2048, kBlock, 0, s>>>(s6_planes(w), w.K, w.N, matrix_id);
}

uint64_t sb6_scratch_bytes(const QWeightDev& w, uint32_t M) {
    if (M != 1) return 0;
    const S6Split sp = sb6_split(w.K, w.N);
    return sp.parts > 1 ? (uint64_t)sp.parts * w.N * sizeof(float) : 0;
}

void launch_sb6_matmul(hipStream_t s, const QWeightDev& w, const QMatmulParams& p, float* scratch) {
    if (p.K != w.K || p.N != w.N) {
        fprintf(stderr, "[zgml_hip] ERROR: a %u x %u matmul over a %u x %u Q6_K weight: not launched\n", p.K, p.N, w.K, w.N);
        return;
    }
    if (p.M == 1) {
        const S6Split sp = scratch ? sb6_split(w.K, w.N) : S6Split{1, cdiv(w.K, kS6Round) * kS6Round};
        const S6MvArgs a{s6_planes(w), p.input, p.dst, scratch, scratch ? (uint32_t*)((char*)scratch - kQmmScratchHead) : nullptr, w.K, w.N, sp.share, sp.parts};
        const dim3 grid(w.N / kQ6kBlock, sp.parts);
        if (w.stream_nt)
            sb6_matvec_kernel<true><<<grid, kS6Waves * 64, 0, s>>>(a);
        else
            sb6_matvec_kernel<false><<<grid, kS6Waves * 64, 0, s>>>(a);
        return;
    }
    const S6MmArgs a{s6_planes(w), p.input, p.dst, p.M, w.K, w.N, p.in_rs, p.dst_rs};
    const bool xvec = ((uintptr_t)p.input % 16 == 0) && (p.K % 4 == 0) && (p.in_rs % 4 == 0);
    const bool nt = w.stream_nt != 0 && p.M <= 32; // several workgroup rows re-read the weights: keep them cached
    if (p.M > 16)
        xvec ? launch_mm<2, true>(s, a, nt) : launch_mm<2, false>(s, a, nt);
    else
        xvec ? launch_mm<1, true>(s, a, nt) : launch_mm<1, false>(s, a, nt);
}

} // namespace zgml
