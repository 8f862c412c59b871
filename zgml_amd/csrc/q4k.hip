// q4k.hip — GGUF Q4_K weights on the device (QW_SB4, "super-block 4-bit"; q4k.h states the format): the re-pack of the file's
// super-blocks, the M = 1 mat-vec and the M > 1 matmul on the matrix cores. Nothing here is shared with the 32-block formats
// (and QW_Q4K, "Q4_0 with K on lanes", is not this format).
//
// DEVICE LAYOUT (4.5 bit/weight like the file: 128 B of nibbles + 16 B of header per (k, 256 columns))
//   qs: 16-byte ITEMS [N / 32][K]: item (j, k) holds the 32 nibbles of sub-block column j (columns 32 j .. 32 j + 31) at row k;
//       byte b = column b (low nibble) | column b + 16 (high nibble). The file keeps sub-blocks 2 i and 2 i + 1 in the two nibbles
//       of the same bytes; here one item has ONE (d * sc, dmin * m) pair, and 64 consecutive k of one j are 1 KiB in a row.
//   sc: 16-byte HEADERS [N / 256][K]: the file's {d, dmin, scales[12]} of super-block column n / 256 at row k, as they are.
//
// ARITHMETIC (both kernels): y[n] = sum_k (x[k] * d * sc) * q[k, n]  -  sum_k x[k] * dmin * m, the second sum once per sub-block
// column. d * sc and dmin * m are formed in f32 (exact), never rounded to f16.
//
// M = 1 (sb4_matvec_kernel): a workgroup of 8 waves owns one super-block column and one K share; wave w streams the items of
// sub-block column w, lane = k, 64 k per sweep (one dwordx4 of nibbles, one dwordx4 of header — the 8 waves of the workgroup read
// the same headers, so HBM sees each once —, one x). A lane carries 32 column sums and one min sum: one multiply, 32 FMAs and one
// FMA per item. The sums are folded over the lanes by row swaps and DPP row sums in a fixed tree. With fewer sub-block columns than
// the part has wave slots the K range is split over blockIdx.y; every part stores its 256 partial outputs and the LAST part to
// arrive (an integer counter; no float atomics) adds them in part order, so the bytes do not depend on arrival order (sb_combine.h).
//
// M > 1 (sb4_matmul_kernel): a workgroup of 4 waves owns one sub-block column (32 output columns = two 16-column tiles) and 16
// rows; the waves deal the 64-k chunks round-robin. Per chunk a wave loads 64 items coalesced, turns them through its own LDS
// slice into [byte][k] order (so lane (r, i) of the MFMA reads its 8 k of columns i and i + 16 as ONE 8-byte LDS read) and leaves
// the 64 (d * sc, dmin * m) pairs beside them. B = the nibble, exact in bf16; A = t = x * (d * sc) in f32, split into three bf16
// pieces (t = h1 + h2 + h3 up to 2^-26 |t|), contracted by v_mfma_f32_16x16x32_bf16 with f32 accumulation: six MFMAs per 32 k.
// The min term is 8 VALU FMAs per 32 k beside them, folded over the four lane rows at the end. Waves are folded in wave order.
#include "q4k.h"
#include "sb_combine.h"

namespace zgml {
namespace {

constexpr uint32_t kSbWaves = 8;           // M = 1: waves of a workgroup = sub-block columns of a super-block column
constexpr uint32_t kSbSweep = 64;          // k per wave sweep (one per lane)
constexpr uint32_t kSbShareMinSweeps = 4;  // a part's K share is at least this many sweeps (the fold costs about one sweep)
constexpr uint32_t kSbTargetWaves = 2048;  // 256 CUs x 8 waves: split K until the grid has this many waves
constexpr uint32_t kSbMmWaves = 4;        // M > 1: waves of a workgroup, dealing the 64-k chunks

typedef float sb4_f4 __attribute__((ext_vector_type(4)));
typedef __bf16 sb4_bf8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ Q4kFactors factors_of(uint4 h, uint32_t j) { return q4k_factors(Q4kHeader{{h.x, h.y, h.z, h.w}}, j); }

// ── re-pack: one thread per item ──
__global__ void __launch_bounds__(kBlock) pack_sb4_kernel(const uint8_t* __restrict__ raw, uint4* __restrict__ qs, uint4* __restrict__ hdr, uint32_t K, uint32_t N) {
    const uint64_t total = (uint64_t)K * (N / kQ4kSub);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(idx / K), k = (uint32_t)(idx % K), nsb = j >> 3, js = j & 7;
        const uint8_t* blk = raw + ((uint64_t)k * (N / kQ4kBlock) + nsb) * kQ4kBytes; // (144 = 9 * 16: every block is 16-byte aligned)
        const uint4* src = (const uint4*)(blk + kQ4kHeaderBytes + 32 * (js >> 1));
        const uint4 lo = src[0], hi = src[1]; // bytes l = 0..15 and 16..31 of the sub-block pair; this sub-block is nibble js & 1
        const uint32_t sh = 4 * (js & 1), mask = 0x0f0f0f0fu;
        qs[idx] = make_uint4(((lo.x >> sh) & mask) | (((hi.x >> sh) & mask) << 4), ((lo.y >> sh) & mask) | (((hi.y >> sh) & mask) << 4),
                             ((lo.z >> sh) & mask) | (((hi.z >> sh) & mask) << 4), ((lo.w >> sh) & mask) | (((hi.w >> sh) & mask) << 4));
        if (js == 0) hdr[(uint64_t)nsb * K + k] = *(const uint4*)blk;
    }
}

// deterministic synthetic weights for the micro-benchmark, in the packed layout: every nibble pattern, sc and m over 0..63
__global__ void __launch_bounds__(kBlock) synth_sb4_kernel(uint4* __restrict__ qs, uint4* __restrict__ hdr, uint32_t K, uint32_t N, uint32_t id) {
    const uint64_t total = (uint64_t)K * (N / kQ4kSub);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t a = (uint32_t)idx * 2654435761u + id * 40503u;
        qs[idx] = make_uint4(a, a * 3u + 1u, a * 5u + 2u, a * 7u + 3u);
        if (idx < (uint64_t)K * (N / kQ4kBlock)) hdr[idx] = make_uint4(0x90001400u /* d = 2^-10, dmin = -2^-11 */, a, a * 11u, a * 13u);
    }
}

// ── M = 1 ──
struct Sb4MvArgs {
    const uint4* qs;
    const uint4* hdr;
    const float* x;
    float* dst;
    float* partial;    // [parts][N] (parts > 1)
    uint32_t* counter; // [N / 256] fan-in words, zero between launches
    uint32_t K, N, share, parts;
};

template <bool NT>
__global__ void __launch_bounds__(kSbWaves * 64) sb4_matvec_kernel(Sb4MvArgs a) {
    __shared__ float red[kSbWaves][kQ4kSub];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y;
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const uint4* items = a.qs + (uint64_t)(nsb * kSbWaves + w) * a.K;
    const uint4* hdrs = a.hdr + (uint64_t)nsb * a.K;

    struct Item {
        uint4 q, h;
        float x;
    };
    auto load = [&](uint32_t k0) {
        const uint32_t k = k0 + lane, kc = min(k, k_hi - 1); // past the share: a live item again, with x = 0
        Item it;
        it.q = wload<NT>(items + kc);
        it.h = hdrs[kc];
        it.x = k < k_hi ? a.x[kc] : 0.f;
        return it;
    };
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = 0.f;
    float macc = 0.f;
    auto consume = [&](const Item& it) {
        const Q4kFactors f = factors_of(it.h, w);
        const float t = it.x * f.scale;
        macc = __builtin_fmaf(it.x, f.min, macc);
        const uint32_t dw[4] = {it.q.x, it.q.y, it.q.z, it.q.w};
#pragma unroll
        for (int dd = 0; dd < 4; dd++) {
            const uint32_t lo = dw[dd] & 0x0f0f0f0fu, hi = (dw[dd] >> 4) & 0x0f0f0f0fu;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                acc[4 * dd + b] = __builtin_fmaf(t, (float)((lo >> (8 * b)) & 255u), acc[4 * dd + b]);
                acc[16 + 4 * dd + b] = __builtin_fmaf(t, (float)((hi >> (8 * b)) & 255u), acc[16 + 4 * dd + b]);
            }
        }
    };
    Item cur = load(k_lo);
    for (uint32_t k0 = k_lo + kSbSweep; k0 < k_hi; k0 += kSbSweep) { // the next sweep's loads fly while this one is consumed
        const Item nxt = load(k0);
        consume(cur);
        cur = nxt;
    }
    consume(cur);

    // 32 sums per lane -> columns: halves (16 registers, half h holds column 2 m + h), rows (8 registers, row r holds column
    // 4 n + 2 (r & 1) + (r >> 1)), then the 16 lanes of a row
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

    const uint32_t n = nsb * kQ4kBlock + threadIdx.x; // threads 0..255: one column each
    float y = threadIdx.x < kQ4kBlock ? red[threadIdx.x >> 5][threadIdx.x & 31] : 0.f;
    if (a.parts > 1 && !sb_combine(y, threadIdx.x < kQ4kBlock, a.partial, a.counter + nsb, part, a.parts, a.N, n, &flag)) return;
    if (threadIdx.x < kQ4kBlock) a.dst[n] = y;
}

// the K split of an M = 1 launch: parts and the k of each (a multiple of the sweep)
struct Sb4Split {
    uint32_t parts, share;
};
Sb4Split sb4_split(uint32_t K, uint32_t N) {
    const uint32_t sweeps = cdiv(K, kSbSweep), want = cdiv(kSbTargetWaves, N / kQ4kSub);
    const uint32_t per = std::max(kSbShareMinSweeps, cdiv(sweeps, want));
    const uint32_t parts = N / kQ4kBlock <= kQmmCounterBytes / 4 ? cdiv(sweeps, per) : 1; // (one counter word per super-block column)
    return parts > 1 ? Sb4Split{parts, per * kSbSweep} : Sb4Split{1, sweeps * kSbSweep};
}

// ── M > 1 ──
struct Sb4MmArgs {
    const uint4* qs;
    const uint4* hdr;
    const float* x;
    float* dst;
    uint32_t M, K, N, in_rs, dst_rs;
};

template <bool XVEC, bool NT>
__global__ void __launch_bounds__(kSbMmWaves * 64) sb4_matmul_kernel(Sb4MmArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t turned[kSbMmWaves][16 * 64]; // per wave: byte b of the chunk's items, [b][k]
    __shared__ __attribute__((aligned(16))) float fs[kSbMmWaves][64], fm[kSbMmWaves][64]; // ... and their d * sc, dmin * m
    __shared__ float fold[kSbMmWaves][2][4][64];
    __shared__ float mins[kSbMmWaves][16];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t j = blockIdx.x, nsb = j >> 3, js = j & 7, m0 = blockIdx.y * 16;
    const uint4* items = a.qs + (uint64_t)j * a.K;
    const uint4* hdrs = a.hdr + (uint64_t)nsb * a.K;
    const float* xrow = a.x + (uint64_t)min(m0 + i, a.M - 1) * a.in_rs; // A operand: lane (r, i) holds row i, k = 8 r .. 8 r + 7 of a 32-k step
    sb4_f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float macc = 0.f;
    const uint32_t chunks = (a.K + 63) / 64;
    for (uint32_t c = w; c < chunks; c += kSbMmWaves) {
        const uint32_t k = c * 64 + lane, kc = min(k, a.K - 1);
        const uint4 q = wload<NT>(items + kc);
        const Q4kFactors f = factors_of(hdrs[kc], js);
        fs[w][lane] = k < a.K ? f.scale : 0.f; // rows past K: t = 0 and no min
        fm[w][lane] = k < a.K ? f.min : 0.f;
        const uint32_t dw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int dd = 0; dd < 4; dd++)
#pragma unroll
            for (int b = 0; b < 4; b++) turned[w][(4 * dd + b) * 64 + lane] = (uint8_t)(dw[dd] >> (8 * b));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the wave's own LDS slice: its DS operations run in order
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t kl = 32 * s + 8 * r, kb = c * 64 + kl;
            const uint2 bb = *(const uint2*)&turned[w][i * 64 + kl];
            const float4 sa = *(const float4*)&fs[w][kl], sb = *(const float4*)&fs[w][kl + 4];
            const float4 ma = *(const float4*)&fm[w][kl], mb = *(const float4*)&fm[w][kl + 4];
            const float4 xa = zero_tail(load_x4<XVEC>(xrow, kb, a.K), kb, a.K), xb = zero_tail(load_x4<XVEC>(xrow, kb + 4, a.K), kb + 4, a.K);
            const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
            const float sv[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
            const float mv[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            const uint32_t bw[2] = {bb.x, bb.y};
            sb4_bf8 h1, h2, h3, q0, q1;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float t = xv[e] * sv[e];
                macc = __builtin_fmaf(xv[e], mv[e], macc);
                h1[e] = (__bf16)t;
                const float r1 = t - (float)h1[e];
                h2[e] = (__bf16)r1;
                const float r2 = r1 - (float)h2[e];
                h3[e] = (__bf16)r2;
                const uint32_t byte = (bw[e >> 2] >> (8 * (e & 3))) & 255u;
                q0[e] = (__bf16)(float)(byte & 15u); // column i
                q1[e] = (__bf16)(float)(byte >> 4);  // column i + 16
            }
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, q0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, q1, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, q0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, q1, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, q0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, q1, acc1, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the reads above stay above the next chunk's writes
        __builtin_amdgcn_wave_barrier();
    }
    // D[m = 4 r + v][n = i] in acc[v]; the min sum of row i over the four lane rows; then the waves in wave order
#pragma unroll
    for (int v = 0; v < 4; v++) fold[w][0][v][lane] = acc0[v], fold[w][1][v][lane] = acc1[v];
    const float mrow = rows_sum4(macc);
    if (r == 0) mins[w][i] = mrow;
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < 512; idx += kSbMmWaves * 64) {
        const uint32_t ct = idx >> 8, v = (idx >> 6) & 3, l = idx & 63, ml = 4 * (l >> 4) + v;
        float sum = fold[0][ct][v][l], mn = mins[0][ml];
        for (uint32_t ww = 1; ww < kSbMmWaves; ww++) sum += fold[ww][ct][v][l], mn += mins[ww][ml];
        const uint32_t m = m0 + ml, n = j * kQ4kSub + ct * 16 + (l & 15);
        if (m < a.M) a.dst[(uint64_t)m * a.dst_rs + n] = sum - mn;
    }
}

template <bool XVEC>
void launch_mm(hipStream_t s, const Sb4MmArgs& a, bool nt) {
    const dim3 grid(a.N / kQ4kSub, cdiv(a.M, 16));
    if (nt)
        sb4_matmul_kernel<XVEC, true><<<grid, kSbMmWaves * 64, 0, s>>>(a);
    else
        sb4_matmul_kernel<XVEC, false><<<grid, kSbMmWaves * 64, 0, s>>>(a);
}

} // namespace

bool sb4_applies(uint64_t K, uint64_t N) { return K >= 1 && K < (1ull << 31) && N >= kQ4kBlock && N % kQ4kBlock == 0 && N < (1ull << 31); }

void sb4_packed_bytes(uint64_t K, uint64_t N, uint64_t* qs_bytes, uint64_t* sc_bytes) {
    *qs_bytes = K * (N / kQ4kSub) * 16;
    *sc_bytes = K * (N / kQ4kBlock) * kQ4kHeaderBytes;
}

void launch_pack_sb4(hipStream_t s, const uint8_t* raw_blocks, const QWeightDev& out) {
    pack_sb4_kernel<<<2048, kBlock, 0, s>>>(raw_blocks, (uint4*)out.qs, (uint4*)out.sc, out.K, out.N);
}

void launch_synth_sb4(hipStream_t s, const QWeightDev& w, uint32_t matrix_id) {
    synth_sb4_kernel<<<2048, kBlock, 0, s>>>((uint4*)w.qs, (uint4*)w.sc, w.K, w.N, matrix_id);
}

uint64_t sb4_scratch_bytes(const QWeightDev& w, uint32_t M) {
    if (M != 1) return 0;
    const Sb4Split sp = sb4_split(w.K, w.N);
    return sp.parts > 1 ? (uint64_t)sp.parts * w.N * sizeof(float) : 0;
}

void launch_sb4_matmul(hipStream_t s, const QWeightDev& w, const QMatmulParams& p, float* scratch) {
    if (p.K != w.K || p.N != w.N) {
        fprintf(stderr, "[zgml_hip] ERROR: a %u x %u matmul over a %u x %u Q4_K weight: not launched\n", p.K, p.N, w.K, w.N);
        return;
    }
    if (p.M == 1) {
        const Sb4Split sp = scratch ? sb4_split(w.K, w.N) : Sb4Split{1, cdiv(w.K, kSbSweep) * kSbSweep};
        const Sb4MvArgs a{(const uint4*)w.qs, (const uint4*)w.sc, p.input, p.dst, scratch, scratch ? (uint32_t*)((char*)scratch - kQmmScratchHead) : nullptr,
                          w.K, w.N, sp.share, sp.parts};
        const dim3 grid(w.N / kQ4kBlock, sp.parts);
        if (w.stream_nt)
            sb4_matvec_kernel<true><<<grid, kSbWaves * 64, 0, s>>>(a);
        else
            sb4_matvec_kernel<false><<<grid, kSbWaves * 64, 0, s>>>(a);
        return;
    }
    const Sb4MmArgs a{(const uint4*)w.qs, (const uint4*)w.sc, p.input, p.dst, p.M, w.K, w.N, p.in_rs, p.dst_rs};
    const bool xvec = ((uintptr_t)p.input % 16 == 0) && (p.K % 4 == 0) && (p.in_rs % 4 == 0);
    const bool nt = w.stream_nt != 0 && p.M <= 16; // several row tiles re-read the weights: keep them cached
    xvec ? launch_mm<true>(s, a, nt) : launch_mm<false>(s, a, nt);
}

} // namespace zgml
