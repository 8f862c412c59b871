// q5k.hip — GGUF Q5_K weights on the device (QW_SB5, "super-block 5-bit"; q5k.h states the format): the re-pack of the file's
// 176-byte super-blocks, the M = 1 mat-vec and the M > 1 matmul on the matrix cores. Q4_K's arithmetic (a (scale, min) pair per 32
// columns, the min term summed apart) over Q6_K's operand problem (a high bit kept apart from the nibble). With q4k.hip and
// q6k.hip it shares the K-split fan-in (sb_combine.h) and nothing else.
//
// DEVICE LAYOUT (5.5 bit/weight like the file: 128 + 32 B of quants and the 16-byte header per (k, 256 columns))
//   qs: two planes of ITEMS [N / 32][K]; item (j, k) holds the 32 q of sub-block column j (columns 32 j .. 32 j + 31) at row k:
//       lo plane, 16 B: byte b = low nibble of column b | low nibble of column b + 16 << 4 (QW_SB4's item)
//       hi plane,  4 B: bit 4 h + s of byte b = high bit of column 16 h + 4 s + b
//       so the four q of columns 16 h + 4 s .. + 3 are ONE dword of bytes: ((lo[s] >> 4 h) & 0x0f0f0f0f) | ((hi >> (4 h + s)) & 0x01010101) << 4
//   sc: 16-byte HEADERS [N / 256][K]: the file's {d, dmin, scales[12]} as Q4kHeader dwords
//
// ARITHMETIC (both kernels): y[n] = sum_k (x[k] * d * sc) * q[k, n]  -  sum_k x[k] * dmin * m, the two sums kept apart and the
// second formed once per 32 columns. d * sc and dmin * m are formed in f32 (exact).
//
// M = 1 (sb5_matvec_kernel): a workgroup of 8 waves owns one super-block column and one K share; wave w streams sub-block column
// w, lane = k. The share is walked in ROUNDS of four 64-k sweeps, and a round issues every load it has — the workgroup's headers
// first, then per wave four lo items, four hi dwords and four x — before anything is consumed: 5.25 KiB in flight per wave. While
// the items fly the 512 threads turn the round's 256 headers into (d * sc, dmin * m) f32 pairs in LDS, once per workgroup
// ([sub-block][k] of 8-byte pairs: a wave reads its own sub-block's pair of 64 k as one conflict-free 8-byte read per lane). Per
// item: t = x * d * sc, one FMA into the min sum, byte -> f32 and an FMA into each of 32 per-lane column sums, folded over the
// lanes in a fixed tree. K is split over blockIdx.y into parts of whole rounds until the grid has about two workgroups per CU
// (at most 16 parts); parts are combined in part order by sb_combine.
//
// M > 1 (sb5_matmul_kernel<RT>): a workgroup of 8 waves owns one item column (32 output columns = two 16-column MFMA tiles) and
// RT = 1 or 2 row tiles of 16; the waves deal the 64-k chunks. Per chunk a wave loads 64 items coalesced, assembles the q bytes,
// turns them ONCE through its own LDS slice into [column][k] order and leaves the chunk's 64 (d * sc, dmin * m) pairs beside them;
// the x rows are loaded once per 32-k step. An item column is ONE scale sub-block, so A = t = x * (d * sc) in f32, split into
// three bf16 pieces (t = h1 + h2 + h3 up to 2^-26 |t|), is formed once per (row tile, 32 k) and feeds BOTH column tiles; B = q
// (0..31, exact in bf16) of a column tile serves both row tiles. v_mfma_f32_16x16x32_bf16 with f32 accumulation, three MFMAs per
// tile and 32 k. The min term is 8 VALU FMAs per (row tile, 32 k) beside them, folded over the four lane rows at the end. Waves
// are folded in wave order.
#include "q5k.h"
#include "sb_combine.h"

namespace zgml {
namespace {

constexpr uint32_t kS5Waves = 8;          // M = 1: waves of a workgroup = sub-block columns of a super-block column
constexpr uint32_t kS5Sweep = 64;         // k per wave sweep (one per lane)
constexpr uint32_t kS5Sweeps = 4;         // sweeps of a round: all loaded before the first is consumed (24 VGPRs)
constexpr uint32_t kS5Round = kS5Sweep * kS5Sweeps; // k of a round = rows of the factor pairs in LDS
constexpr uint32_t kS5TargetWaves = 4096; // 256 CUs x 2 workgroups x 8 waves: split K until the grid has this many waves ...
constexpr uint32_t kS5MaxParts = 16;      // ... but into at most this many parts (two batches of the combine)
constexpr uint32_t kS5MmWaves = 8;        // M > 1: waves of a workgroup, dealing the 64-k chunks
static_assert(kS5Waves * 64 == 2 * kS5Round, "the header duty below: one k and four of its eight sub-blocks per thread");

typedef float sb5_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 sb5_bf8 __attribute__((ext_vector_type(8)));

struct S5Planes {
    uint4* lo;
    uint32_t* hi;
    uint4* hdr;
};
S5Planes s5_planes(const QWeightDev& w) {
    uint4* lo = (uint4*)w.qs;
    return {lo, (uint32_t*)(lo + (uint64_t)w.K * (w.N / kQ5kSub)), (uint4*)w.sc};
}

template <bool NT>
__device__ __forceinline__ uint32_t wload1(const uint32_t* p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}

// the 32 q of an item as eight dwords of four bytes: dword 4 h + s = columns 16 h + 4 s .. + 3
__device__ __forceinline__ void s5_quants(uint4 lo, uint32_t hi, uint32_t (&q)[8]) {
    const uint32_t l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        q[s] = (l[s] & 0x0f0f0f0fu) | (((hi >> s) & 0x01010101u) << 4);
        q[4 + s] = ((l[s] >> 4) & 0x0f0f0f0fu) | (((hi >> (4 + s)) & 0x01010101u) << 4);
    }
}
__device__ __forceinline__ Q4kFactors s5_factors(uint4 h, uint32_t j) { return q4k_factors(Q4kHeader{{h.x, h.y, h.z, h.w}}, j); }

// ── re-pack: one thread per item; the file block is read by bytes (only 2-byte aligned) through q5k.h's own rule ──
__global__ void __launch_bounds__(kBlock) pack_sb5_kernel(const uint8_t* __restrict__ raw, S5Planes o, uint32_t K, uint32_t N) {
    const uint64_t total = (uint64_t)K * (N / kQ5kSub);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(idx / K), k = (uint32_t)(idx % K), nsb = j >> 3, js = j & 7;
        const uint8_t* blk = raw + ((uint64_t)k * (N / kQ5kBlock) + nsb) * kQ5kBytes;
        uint32_t lo[4] = {0, 0, 0, 0}, hi = 0;
#pragma unroll
        for (uint32_t c = 0; c < 32; c++) {
            const uint32_t q = q5k_quant(blk, 32 * js + c), h = c >> 4, s = (c >> 2) & 3, b = c & 3;
            lo[s] |= (q & 15u) << (8 * b + 4 * h);
            hi |= (q >> 4) << (8 * b + 4 * h + s);
        }
        o.lo[idx] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        o.hi[idx] = hi;
        if (js == 0) {
            uint32_t hw[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t e = 0; e < kQ4kHeaderBytes; e++) hw[e >> 2] |= (uint32_t)blk[e] << (8 * (e & 3));
            o.hdr[(uint64_t)nsb * K + k] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        }
    }
}

// deterministic synthetic weights for the micro-benchmark, in the packed layout: every q, sc and m over 0..63
__global__ void __launch_bounds__(kBlock) synth_sb5_kernel(S5Planes o, uint32_t K, uint32_t N, uint32_t id) {
    const uint64_t total = (uint64_t)K * (N / kQ5kSub);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t a = (uint32_t)idx * 2654435761u + id * 40503u;
        o.lo[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        o.hi[idx] = a * 17u + 4u;
        if (idx < (uint64_t)K * (N / kQ5kBlock)) o.hdr[idx] = make_uint4(0x90001400u /* d = 2^-10, dmin = -2^-11 */, a, a * 11u, a * 13u);
    }
}

// ── M = 1 ──
struct S5MvArgs {
    S5Planes w;
    const float* x;
    float* dst;
    float* partial;    // [parts][N] (parts > 1)
    uint32_t* counter; // [N / 256] fan-in words, zero between launches
    uint32_t K, N, share, parts;
};

template <bool NT>
__global__ void __launch_bounds__(kS5Waves * 64) sb5_matvec_kernel(S5MvArgs a) {
    __shared__ float2 fac[kS5Waves][kS5Round]; // (d * sc, dmin * m) of the round: [sub-block][k]
    __shared__ float red[kS5Waves][kQ5kSub];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y;
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const uint4* items_lo = a.w.lo + (uint64_t)(nsb * kS5Waves + w) * a.K;
    const uint32_t* items_hi = a.w.hi + (uint64_t)(nsb * kS5Waves + w) * a.K;
    const uint4* hdrs = a.w.hdr + (uint64_t)nsb * a.K;
    const uint32_t hkl = threadIdx.x & (kS5Round - 1), hhalf = threadIdx.x >> 8; // header duty: one k, four of its eight sub-blocks

    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = 0.f;
    float macc = 0.f;
    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += kS5Round) {
        // every load of the round, the header first (its wait then leaves the items in flight); past the share: a live
        // address again, with x = 0 and both factors 0
        const uint4 hd = hdrs[min(k0 + hkl, k_hi - 1)];
        uint4 ql[kS5Sweeps];
        uint32_t qh[kS5Sweeps];
        float xs[kS5Sweeps];
#pragma unroll
        for (uint32_t s = 0; s < kS5Sweeps; s++) {
            const uint32_t k = k0 + s * kS5Sweep + lane, kc = min(k, k_hi - 1);
            ql[s] = wload<NT>(items_lo + kc);
            qh[s] = wload1<NT>(items_hi + kc);
            xs[s] = k < k_hi ? a.x[kc] : 0.f;
        }
        const bool hlive = k0 + hkl < k_hi;
        if (hhalf == 0) { // (the same for a whole wave; the sub-block is a constant in each arm, so q4k_factors' selects fold away)
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                const Q4kFactors f = s5_factors(hd, e);
                fac[e][hkl] = hlive ? make_float2(f.scale, f.min) : make_float2(0.f, 0.f);
            }
        } else {
#pragma unroll
            for (uint32_t e = 4; e < 8; e++) {
                const Q4kFactors f = s5_factors(hd, e);
                fac[e][hkl] = hlive ? make_float2(f.scale, f.min) : make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < kS5Sweeps; s++) {
            if (k0 + s * kS5Sweep >= k_hi) break; // (the same for the whole workgroup)
            const float2 f = fac[w][s * kS5Sweep + lane];
            const float t = xs[s] * f.x;
            macc = __builtin_fmaf(xs[s], f.y, macc);
            uint32_t q[8];
            s5_quants(ql[s], qh[s], q);
#pragma unroll
            for (int dd = 0; dd < 8; dd++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[4 * dd + b] = __builtin_fmaf(t, (float)((q[dd] >> (8 * b)) & 255u), acc[4 * dd + b]);
        }
        __syncthreads(); // the next round rewrites fac
    }

    // 32 sums per lane -> columns: halves (16 registers, half h holds column 2 m + h), rows (8 registers, row r holds column
    // 4 n + 2 (r & 1) + (r >> 1)), then the 16 lanes of a row; the min sum over all 64 lanes
    float b16[16];
#pragma unroll
    for (int m = 0; m < 16; m++) b16[m] = kon_fold32(acc[2 * m], acc[2 * m + 1]);
    float c8[8];
#pragma unroll
    for (int n = 0; n < 8; n++) c8[n] = row16_sum(kon_fold16(b16[2 * n], b16[2 * n + 1]));
    const float mins = rows_sum4(row16_sum(macc));
    float v = c8[0];
#pragma unroll
    for (int n = 1; n < 8; n++) v = i == (uint32_t)n ? c8[n] : v;
    if (i < 8) red[w][4 * i + 2 * (r & 1) + (r >> 1)] = v - mins;
    __syncthreads();

    const bool live = threadIdx.x < kQ5kBlock; // threads 0..255: one column each
    const uint32_t n = nsb * kQ5kBlock + threadIdx.x;
    float y = live ? red[threadIdx.x >> 5][threadIdx.x & 31] : 0.f;
    if (a.parts > 1 && !sb_combine(y, live, a.partial, a.counter + nsb, part, a.parts, a.N, n, &flag)) return;
    if (live) a.dst[n] = y;
}

// the K split of an M = 1 launch: parts and the k of each (whole rounds)
struct S5Split {
    uint32_t parts, share;
};
S5Split sb5_split(uint32_t K, uint32_t N) {
    const uint32_t rounds = cdiv(K, kS5Round), want = cdiv(kS5TargetWaves, N / kQ5kSub);
    const uint32_t per = std::max(cdiv(rounds, want), cdiv(rounds, kS5MaxParts));
    const uint32_t parts = N / kQ5kBlock <= kQmmCounterBytes / 4 ? cdiv(rounds, per) : 1; // (one counter word per super-block column)
    return parts > 1 ? S5Split{parts, per * kS5Round} : S5Split{1, rounds * kS5Round};
}

// ── M > 1 ──
struct S5MmArgs {
    S5Planes w;
    const float* x;
    float* dst;
    uint32_t M, K, N, in_rs, dst_rs;
};

template <int RT, bool XVEC, bool NT>
__global__ void __launch_bounds__(kS5MmWaves * 64) sb5_matmul_kernel(S5MmArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t turned[kS5MmWaves][32 * 64];           // per wave: the chunk's q bytes, [column][k]
    __shared__ __attribute__((aligned(16))) float fs[kS5MmWaves][64], fm[kS5MmWaves][64]; // ... and its d * sc, dmin * m
    __shared__ float fold[kS5MmWaves][RT * 2][4][64];
    __shared__ float mins[kS5MmWaves][RT][16];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t j = blockIdx.x, nsb = j >> 3, js = j & 7, m0 = blockIdx.y * 16 * RT;
    const uint4* items_lo = a.w.lo + (uint64_t)j * a.K;
    const uint32_t* items_hi = a.w.hi + (uint64_t)j * a.K;
    const uint4* hdrs = a.w.hdr + (uint64_t)nsb * a.K;
    const float* xrow[RT]; // A operand: lane (r, i) holds row i, k = 8 r .. 8 r + 7 of a 32-k step
    sb5_f4 acc[RT][2];
    float macc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        xrow[rt] = a.x + (uint64_t)min(m0 + 16 * rt + i, a.M - 1) * a.in_rs;
        acc[rt][0] = acc[rt][1] = sb5_f4{0.f, 0.f, 0.f, 0.f};
        macc[rt] = 0.f;
    }
    const uint32_t chunks = (a.K + 63) / 64;
    for (uint32_t c = w; c < chunks; c += kS5MmWaves) {
        const uint32_t k = c * 64 + lane, kc = min(k, a.K - 1);
        const uint4 lo = wload<NT>(items_lo + kc);
        const uint32_t hi = wload1<NT>(items_hi + kc);
        const Q4kFactors f = s5_factors(hdrs[kc], js);
        fs[w][lane] = k < a.K ? f.scale : 0.f; // rows past K: t = 0 and no min
        fm[w][lane] = k < a.K ? f.min : 0.f;
        uint32_t q[8];
        s5_quants(lo, hi, q);
#pragma unroll
        for (int dd = 0; dd < 8; dd++)
#pragma unroll
            for (int b = 0; b < 4; b++) turned[w][(4 * dd + b) * 64 + lane] = (uint8_t)(q[dd] >> (8 * b));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the wave's own LDS slice: its DS operations run in order
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t kl = 32 * s + 8 * r, kb = c * 64 + kl;
            const float4 sa = *(const float4*)&fs[w][kl], sb = *(const float4*)&fs[w][kl + 4];
            const float4 ma = *(const float4*)&fm[w][kl], mb = *(const float4*)&fm[w][kl + 4];
            const float sv[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
            const float mv[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            sb5_bf8 qv[2]; // B of the two column tiles: column 16 ct + i
#pragma unroll
            for (int ct = 0; ct < 2; ct++) {
                const uint2 bb = *(const uint2*)&turned[w][(16 * ct + i) * 64 + kl];
                const uint32_t bw[2] = {bb.x, bb.y};
#pragma unroll
                for (int e = 0; e < 8; e++) qv[ct][e] = (__bf16)(float)((bw[e >> 2] >> (8 * (e & 3))) & 255u);
            }
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const float4 xa = zero_tail(load_x4<XVEC>(xrow[rt], kb, a.K), kb, a.K), xb = zero_tail(load_x4<XVEC>(xrow[rt], kb + 4, a.K), kb + 4, a.K);
                const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                sb5_bf8 h1, h2, h3; // one A for both column tiles: the item column is one scale sub-block
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float t = xv[e] * sv[e];
                    macc[rt] = __builtin_fmaf(xv[e], mv[e], macc[rt]);
                    h1[e] = (__bf16)t;
                    const float r1 = t - (float)h1[e];
                    h2[e] = (__bf16)r1;
                    const float r2 = r1 - (float)h2[e];
                    h3[e] = (__bf16)r2;
                }
#pragma unroll
                for (int ct = 0; ct < 2; ct++) {
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, qv[ct], acc[rt][ct], 0, 0, 0);
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, qv[ct], acc[rt][ct], 0, 0, 0);
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, qv[ct], acc[rt][ct], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the reads above stay above the next chunk's writes
        __builtin_amdgcn_wave_barrier();
    }
    // D[m = 4 r + v][n = i] in acc[v]; the min sum of row i over the four lane rows; then the waves in wave order
#pragma unroll
    for (int t = 0; t < RT * 2; t++)
#pragma unroll
        for (int v = 0; v < 4; v++) fold[w][t][v][lane] = acc[t >> 1][t & 1][v];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const float mrow = rows_sum4(macc[rt]);
        if (r == 0) mins[w][rt][i] = mrow;
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < RT * 2 * 256; idx += kS5MmWaves * 64) {
        const uint32_t t = idx >> 8, v = (idx >> 6) & 3, l = idx & 63, ml = 4 * (l >> 4) + v;
        float sum = fold[0][t][v][l], mn = mins[0][t >> 1][ml];
        for (uint32_t ww = 1; ww < kS5MmWaves; ww++) sum += fold[ww][t][v][l], mn += mins[ww][t >> 1][ml];
        const uint32_t m = m0 + 16 * (t >> 1) + ml, n = j * kQ5kSub + (t & 1) * 16 + (l & 15);
        if (m < a.M) a.dst[(uint64_t)m * a.dst_rs + n] = sum - mn;
    }
}

template <int RT, bool XVEC>
void launch_mm(hipStream_t s, const S5MmArgs& a, bool nt) {
    const dim3 grid(a.N / kQ5kSub, cdiv(a.M, 16 * RT));
    if (nt)
        sb5_matmul_kernel<RT, XVEC, true><<<grid, kS5MmWaves * 64, 0, s>>>(a);
    else
        sb5_matmul_kernel<RT, XVEC, false><<<grid, kS5MmWaves * 64, 0, s>>>(a);
}

} // namespace

bool sb5_applies(uint64_t K, uint64_t N) { return sb4_applies(K, N); }

void sb5_packed_bytes(uint64_t K, uint64_t N, uint64_t* qs_bytes, uint64_t* sc_bytes) {
    *qs_bytes = K * (N / kQ5kSub) * (16 + 4);
    *sc_bytes = K * (N / kQ5kBlock) * kQ4kHeaderBytes;
}

void launch_pack_sb5(hipStream_t s, const uint8_t* raw_blocks, const QWeightDev& out) {
    pack_sb5_kernel<<<2048, kBlock, 0, s>>>(raw_blocks, s5_planes(out), out.K, out.N);
}

void launch_synth_sb5(hipStream_t s, const QWeightDev& w, uint32_t matrix_id) {
    synth_sb5_kernel<<<2048, kBlock, 0, s>>>(s5_planes(w), w.K, w.N, matrix_id);
}

uint64_t sb5_scratch_bytes(const QWeightDev& w, uint32_t M) {
    if (M != 1) return 0;
    const S5Split sp = sb5_split(w.K, w.N);
    return sp.parts > 1 ? (uint64_t)sp.parts * w.N * sizeof(float) : 0;
}

void launch_sb5_matmul(hipStream_t s, const QWeightDev& w, const QMatmulParams& p, float* scratch) {
    if (p.K != w.K || p.N != w.N) {
        fprintf(stderr, "[zgml_hip] ERROR: a %u x %u matmul over a %u x %u Q5_K weight: not launched\n", p.K, p.N, w.K, w.N);
        return;
    }
    if (p.M == 1) {
        const S5Split sp = scratch ? sb5_split(w.K, w.N) : S5Split{1, cdiv(w.K, kS5Round) * kS5Round};
        const S5MvArgs a{s5_planes(w), p.input, p.dst, scratch, scratch ? (uint32_t*)((char*)scratch - kQmmScratchHead) : nullptr, w.K, w.N, sp.share, sp.parts};
        const dim3 grid(w.N / kQ5kBlock, sp.parts);
        if (w.stream_nt)
            sb5_matvec_kernel<true><<<grid, kS5Waves * 64, 0, s>>>(a);
        else
            sb5_matvec_kernel<false><<<grid, kS5Waves * 64, 0, s>>>(a);
        return;
    }
    const S5MmArgs a{s5_planes(w), p.input, p.dst, p.M, w.K, w.N, p.in_rs, p.dst_rs};
    const bool xvec = ((uintptr_t)p.input % 16 == 0) && (p.K % 4 == 0) && (p.in_rs % 4 == 0);
    const bool nt = w.stream_nt != 0 && p.M <= 32; // several workgroup rows re-read the weights: keep them cached
    if (p.M > 16)
        xvec ? launch_mm<2, true>(s, a, nt) : launch_mm<2, false>(s, a, nt);
    else
        xvec ? launch_mm<1, true>(s, a, nt) : launch_mm<1, false>(s, a, nt);
}

} // namespace zgml
