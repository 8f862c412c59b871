// dense_f16.hip — dense matmul with f16-promoted weights (the one place the path is a real
// contraction on 16-bit data, so the one place the XDL matrix cores are used).
//
// Semantics (the reference's f16 weight promotion: src/backend/wgpu.zig:1071-1104 packs the B
// operand of a `matmul` op that has an initial upload to f16 [K,N]; src/backend/metal.zig:680-760
// `matvec_f16` / `matmul_f16` then compute
//     M == 1:  C[n]   = sum_k A[k]            * f32(B16[k,n])      (A stays f32)
//     M  > 1:  C[m,n] = sum_k f16(A[m,k])     * B16[k,n]           (A rounded to half, f32 accumulate)
// Same here; only the summation order differs.
//
// Device layout of a promoted weight ("MFMA-packed", chosen at compile_program time):
//   Bp: half[N/16][KC][64][8],  KC = ceil(K/32), item (g, c, lane = 16r+i) = the 8 values
//       B[k = 32c + 8r + e][n = 16g + i], e = 0..7 (zero for k >= K)
// which is exactly the B operand of v_mfma_f32_16x16x32_f16 for lane (i, r): one 16-byte load per
// lane, 1 KiB contiguous per wave, and no LDS or shuffles on the weight stream.
//
// Thread mapping (same shape as the quantized mat-vec): a workgroup owns one 16-column group and all
// of K; its waves split K. Per step a wave takes DEPTH consecutive 32-k chunks (4 KiB of weights in
// flight per wave, next step prefetched; DEPTH = 8: with 4 the step count doubled and every step exposed
// the x-load latency, 4096^2 at M = 32 15.3 -> 12.2 us), x for the step is staged through LDS by row-contiguous
// loads — as f16 [16R rows][chunk] for the MFMA form (ds_read_b128 = one A operand), as f32 for the
// M == 1 form (v_fma_mix_f32: f32 x times the f16 weight, no rounding of x).
#include "kernels.h"

#include <hip/hip_fp16.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>

namespace zgml {

namespace {

constexpr int kBlock = 256;

typedef float mfma_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct F16Args {
    const uint4* bp;
    const float* a;
    float* out;
    uint32_t M, K, KC, a_rs, out_rs, NB2;
};

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

__device__ __forceinline__ uint32_t column_group(uint32_t b, uint32_t NB2) {
    // groups b and b+8 land on the same XCD (round-robin dispatch); nothing to share here, keep it linear
    (void)NB2;
    return b;
}

template <bool XVEC>
__device__ __forceinline__ float4 load_a4(const float* x, uint32_t i, uint32_t K) {
    if (XVEC) return *(const float4*)(x + (i < K ? i : 0));
    const uint32_t last = K - 1;
    return make_float4(x[min(i, last)], x[min(i + 1, last)], x[min(i + 2, last)], x[min(i + 3, last)]);
}
__device__ __forceinline__ float4 zero_tail(float4 v, uint32_t i, uint32_t K) {
    return make_float4(i < K ? v.x : 0.f, i + 1 < K ? v.y : 0.f, i + 2 < K ? v.z : 0.f, i + 3 < K ? v.w : 0.f);
}

__device__ __forceinline__ uint2 pack_half4(float4 v) {
    const __half2 lo = __floats2half2_rn(v.x, v.y), hi = __floats2half2_rn(v.z, v.w);
    uint2 r;
    r.x = *(const uint32_t*)&lo, r.y = *(const uint32_t*)&hi;
    return r;
}

// R m-tiles of 16 rows (MFMA form), or R == 0: the M == 1 mat-vec form. G column groups per workgroup:
// wave w = (column group w / KW, K slice w % KW); the G wave sets share every staged x chunk, which is
// what the M > 1 form is bound by (x re-staged per 16 columns costs ~1/3 of the kernel at M = 32).
template <int R, bool XVEC, int G, bool NT>
__global__ void __launch_bounds__(512) dense_f16_kernel(F16Args a) {
    // 32-k chunks per wave per step. 8 halves the step count (every step exposes one x-load latency:
    // 4096^2 at M = 1 9.7 -> 8.5 us); the R = 2 form cannot afford the staging registers for that and
    // runs 8 K-slice waves of depth 4 instead (same 1024-k step).
    constexpr int kDepth = R == 2 ? 4 : 8;
    constexpr bool MV = R == 0;
    constexpr int ROWS = MV ? 1 : 16 * R;
    constexpr int NX = MV ? 1 : 2 * kDepth * R / G; // float4 of x each thread stages per step (16R rows x KW*kDepth*32 k)
    extern __shared__ float smem[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n_kw = (blockDim.x >> 6) / G;
    const uint32_t w = wv % n_kw, cgi = wv / n_kw; // K slice, column group within the workgroup
    const uint32_t g_raw = blockIdx.x * G + cgi, g = min(g_raw, a.NB2 - 1), m0 = blockIdx.y * ROWS;
    const uint32_t n_waves = n_kw;
    const uint32_t row = lane >> 4, i = lane & 15;
    const uint32_t step_chunks = n_waves * kDepth, chf = step_chunks * 32;
    // LDS row: f16 form chf halves + 8 pad (= (chf + 8) / 2 floats); f32 form chf floats
    const uint32_t row_floats = MV ? chf : (chf + 8) / 2;
    const uint32_t buf_floats = ROWS * row_floats;
    const uint4* bp = a.bp + ((uint64_t)g * a.KC) * 64 + lane;
    const uint32_t n_steps = (a.KC + step_chunks - 1) / step_chunks;

    const uint32_t f4_per_row = chf / 4;
    uint32_t st_col[NX], st_lds[NX];
    const float* st_src[NX];
    bool st_on[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) {
        const uint32_t f = threadIdx.x + j * blockDim.x, r = f / f4_per_row;
        st_on[j] = r < (uint32_t)ROWS; // mat-vec form: only chf/4 threads stage
        st_col[j] = 4 * (f % f4_per_row);
        st_lds[j] = MV ? st_col[j] : r * row_floats + st_col[j] / 2;
        st_src[j] = a.a + (uint64_t)min(m0 + min(r, (uint32_t)ROWS - 1), a.M - 1) * a.a_rs;
    }
    float4 stage[NX];
    auto stage_load = [&](uint32_t step) {
#pragma unroll
        for (int j = 0; j < NX; j++) stage[j] = load_a4<XVEC>(st_src[j], step * chf + st_col[j], a.K);
    };
    auto stage_store = [&](uint32_t step) {
        float* dst = smem + (step & 1) * buf_floats;
        const bool full = (step + 1) * chf <= a.K; // whole chunk inside K (uniform): no selects
#pragma unroll
        for (int j = 0; j < NX; j++) {
            const float4 v = full ? stage[j] : zero_tail(stage[j], step * chf + st_col[j], a.K);
            if (MV) {
                if (st_on[j]) *(float4*)(dst + st_lds[j]) = v;
            } else {
                *(uint2*)(dst + st_lds[j]) = pack_half4(v); // f16(A), round to nearest even
            }
        }
    };
    auto load_b = [&](uint4 (&b)[kDepth], uint32_t step) {
#pragma unroll
        for (int d = 0; d < kDepth; d++) { // clamped, unconditional; only the last step has chunks >= KC (zeroed before its compute, below)
            const uint32_t c = min(step * step_chunks + w * kDepth + d, a.KC - 1);
            if (NT) { // weight set beyond the Infinity Cache: read-once stream, do not allocate (see qmatvec.hip wload)
                typedef unsigned int u4v __attribute__((ext_vector_type(4)));
                const u4v v = __builtin_nontemporal_load((const u4v*)(bp + (uint64_t)c * 64));
                b[d] = make_uint4(v.x, v.y, v.z, v.w);
            } else {
                b[d] = bp[(uint64_t)c * 64];
            }
        }
    };

    mfma_f4 acc[MV ? 1 : R];
#pragma unroll
    for (int t = 0; t < (MV ? 1 : R); t++) acc[t] = mfma_f4{0.f, 0.f, 0.f, 0.f};
    float acc_mv = 0.f;

    auto compute = [&](const uint4 (&b)[kDepth], uint32_t step) {
        const float* xs = smem + (step & 1) * buf_floats;
#pragma unroll
        for (int d = 0; d < kDepth; d++) {
            const uint32_t k_local = (w * kDepth + d) * 32 + 8 * row; // this lane's 8 k within the step
            if (MV) {
                const float4 x0 = *(const float4*)(xs + k_local), x1 = *(const float4*)(xs + k_local + 4);
                const __half2* h = (const __half2*)&b[d];
                // fmaf(f32, f32(f16), f32) -> v_fma_mix_f32
                acc_mv = fmaf(x0.x, __low2float(h[0]), acc_mv);
                acc_mv = fmaf(x0.y, __high2float(h[0]), acc_mv);
                acc_mv = fmaf(x0.z, __low2float(h[1]), acc_mv);
                acc_mv = fmaf(x0.w, __high2float(h[1]), acc_mv);
                acc_mv = fmaf(x1.x, __low2float(h[2]), acc_mv);
                acc_mv = fmaf(x1.y, __high2float(h[2]), acc_mv);
                acc_mv = fmaf(x1.z, __low2float(h[3]), acc_mv);
                acc_mv = fmaf(x1.w, __high2float(h[3]), acc_mv);
            } else {
                const half8 bv = *(const half8*)&b[d];
#pragma unroll
                for (int t = 0; t < (MV ? 1 : R); t++) {
                    const half8 av = *(const half8*)(xs + (t * 16 + i) * row_floats + k_local / 2);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[t], 0, 0, 0);
                }
            }
        }
    };

    uint4 cur[kDepth];
    stage_load(0);
    load_b(cur, 0);
    stage_store(0);
    __syncthreads();
    for (uint32_t st = 1; st < n_steps; st++) {
        uint4 nxt[kDepth];
        stage_load(st);
        load_b(nxt, st);
        __builtin_amdgcn_sched_barrier(0); // keep the prefetch ahead of the compute block
        compute(cur, st - 1);
        __builtin_amdgcn_sched_barrier(0);
        stage_store(st);
        __syncthreads();
#pragma unroll
        for (int d = 0; d < kDepth; d++) cur[d] = nxt[d];
    }
    // chunks >= KC of the last step carry zero weights (wave-uniform select). x is staged as zero there, but the clamped duplicate
    // of the last chunk would turn an f16 inf of that chunk (|b| >= 65520) into 0 * inf = NaN where the sum is +-inf. Here and not
    // in load_b: there the select would wait for the prefetch it follows (measured 7.7 -> 9.6 us at 4096^2, M = 1).
    {
        const uint32_t c0 = (n_steps - 1) * step_chunks + __builtin_amdgcn_readfirstlane(w) * kDepth;
#pragma unroll
        for (int d = 0; d < kDepth; d++)
            if (c0 + d >= a.KC) cur[d] = make_uint4(0, 0, 0, 0);
    }
    compute(cur, n_steps - 1);
    __syncthreads();

    if (MV) {
        // fold the 4 k-rows of the wave, then the waves, in fixed order
        acc_mv += __shfl_xor(acc_mv, 16, 64);
        acc_mv += __shfl_xor(acc_mv, 32, 64);
        if (lane < 16) smem[w * 16 + lane] = acc_mv;
        __syncthreads();
        if (threadIdx.x < 16) {
            float v = smem[threadIdx.x];
            for (uint32_t ww = 1; ww < n_waves; ww++) v += smem[ww * 16 + threadIdx.x];
            a.out[(uint64_t)m0 * a.out_rs + g * 16 + threadIdx.x] = v;
        }
    } else {
        constexpr int RT = MV ? 1 : R;
#pragma unroll
        for (int t = 0; t < RT; t++)
#pragma unroll
            for (int v = 0; v < 4; v++) smem[((wv * RT + t) * 4 + v) * 64 + lane] = acc[t][v];
        __syncthreads();
        for (uint32_t idx = threadIdx.x; idx < (uint32_t)G * RT * 256; idx += blockDim.x) {
            const uint32_t cg = idx / (RT * 256), rem = idx % (RT * 256);
            const uint32_t t = rem >> 8, v = (rem >> 6) & 3, l = rem & 63;
            const uint32_t w0 = cg * n_kw; // this column group's K-slice waves, summed in wave order
            float sum = smem[((w0 * RT + t) * 4 + v) * 64 + l];
            for (uint32_t ww = 1; ww < n_kw; ww++) sum += smem[(((w0 + ww) * RT + t) * 4 + v) * 64 + l];
            const uint32_t gg = blockIdx.x * G + cg;
            const uint32_t m = m0 + t * 16 + 4 * (l >> 4) + v, n = gg * 16 + (l & 15);
            if (m < a.M && gg < a.NB2) a.out[(uint64_t)m * a.out_rs + n] = sum;
        }
    }
}

// ── M > 1, second form: A pre-rounded and pre-laid-out, no LDS in the K loop ─────────────────
// The staged form above re-reads f32 x through LDS in every workgroup (rounding it to f16 each time) with a
// barrier per step: 13.3 us for 32 x 4096 x 4096 against 4.2 us of weight streaming. Here pack_a_f16_kernel
// rounds x to f16 ONCE per matmul (same round-to-nearest-even, so the products are the same numbers) into
// the MFMA A-operand layout  Ap: half[tiles][KC][64][8], item (t, c, lane = 16 r + i) = A[16 t + i][32 c + 8 r + e],
// and a lane's A operand is one 16-byte load of a wave-contiguous 1 KB block (L2-resident), exactly like
// its B operand. Waves split the 32-k chunks round-robin and keep DEPTH chunks (B and A) in flight.
struct F16Part2 { // one weight of a grouped launch (q/k/v, gate/up: same rows, same K)
    const uint4* bp;
    float* out;
    uint32_t out_rs, block_begin; // first workgroup (column group) of the part
};
constexpr int kMaxF16Parts = 3;
struct F16Args2 {
    F16Part2 parts[kMaxF16Parts];
    const uint4* ap;
    uint32_t n_parts, M, KC;
};

__global__ void __launch_bounds__(kBlock) pack_a_f16_kernel(const float* __restrict__ x, uint32_t M, uint32_t K, uint32_t a_rs, uint32_t KC,
                                                            uint32_t tiles, uint4* __restrict__ ap) {
    const uint64_t n_items = (uint64_t)tiles * KC * 64;
    for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < n_items; it += (uint64_t)gridDim.x * kBlock) {
        const uint32_t lane = it & 63, i = lane & 15, r = lane >> 4;
        const uint64_t tc = it >> 6;
        const uint32_t c = tc % KC, t = tc / KC, m = 16 * t + i, k0 = 32 * c + 8 * r;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = (m < M && k0 + e < K) ? x[(uint64_t)m * a_rs + k0 + e] : 0.f;
        const uint2 lo = pack_half4(make_float4(v[0], v[1], v[2], v[3])), hi = pack_half4(make_float4(v[4], v[5], v[6], v[7]));
        ap[it] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
}

// What paces this kernel (the sink experiment of round 4, removed since): with its MFMAs replaced by a vector-ALU
// sink of the operands (an xor of every loaded dword into the accumulators) the stream was UNCHANGED; with the A operand's global
// loads gone as well it rose to 5.6 TB/s from 3.6-4.4 — not the matrix instructions, the R KiB of L2 hits per KiB of weights
// through the CU's one vector-memory path. (Taking A out of that path — shared through LDS, or stationary in LDS — was measured
// no faster all the same; those two forms are removed too.)
template <int R, bool NT, int CG = 1>
__global__ void __launch_bounds__(512) dense_f16_tile2_kernel(F16Args2 a) {
    // chunks in flight per wave, (CG + R) x 16 B per lane each (8 measured no faster at R = 2). R = 4 / 8 (prefill chunks of
    // 64 / 128 tokens): all m-tiles in one workgroup, so the weights are read ONCE per matmul instead of once per tile pair
    // (Llama-2-7B at 128 tokens: 13.5 GB of f16 weights per chunk instead of 54 GB); 3 / 2 chunks in flight keep the ring
    // within the register budget of two waves per SIMD.
    // CG (round 4): column groups per workgroup. Every workgroup re-reads the whole pre-laid-out A operand from L2 (R x 1 KiB per
    // 32-k chunk) next to ONE KiB of weights per column group: at CG = 1 and R = 2 two of every three bytes a CU's vector-memory
    // path returns are A, and that path (64 B / clk per CU whatever the hit level), not HBM, paces the launch (3.6 TB/s at
    // 32 x 4096 x 22016). With CG column groups per workgroup one A chunk feeds CG x R MFMAs: A : B = R : CG.
    constexpr int DEPTH = R >= 8 ? 2 : (R >= 4 ? 3 : (CG >= 4 ? 3 : 4));
    extern __shared__ float smem[];
    // w in an SGPR: the chunk guard below must be a scalar branch — a v_mfma ignores EXEC, so a predicated
    // (if-converted) guard would still accumulate the clamped duplicate chunks
    const uint32_t lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
    uint32_t pi = 0;
#pragma unroll
    for (uint32_t t = 1; t < (uint32_t)kMaxF16Parts; t++)
        if (t < a.n_parts && blockIdx.x >= a.parts[t].block_begin) pi = t;
    const F16Part2& P = a.parts[pi];
    const uint32_t g = (blockIdx.x - P.block_begin) * CG, t0 = blockIdx.y * R; // first column group of this workgroup
    const uint4* bp = P.bp + (uint64_t)g * a.KC * 64 + lane;
    const uint4* ap = a.ap + (uint64_t)t0 * a.KC * 64 + lane;
    const uint64_t tile_stride = (uint64_t)a.KC * 64;
    struct Chunk {
        uint4 b[CG];
        uint4 av[R];
    };
    auto load = [&](Chunk& x, uint32_t c) { // clamped, unconditional: a repeated chunk is never used twice (the loop bounds decide)
        const uint32_t cc = min(c, a.KC - 1);
#pragma unroll
        for (int j = 0; j < CG; j++) {
            if (NT) {
                typedef unsigned int u4v __attribute__((ext_vector_type(4)));
                const u4v v = __builtin_nontemporal_load((const u4v*)(bp + j * tile_stride + (uint64_t)cc * 64));
                x.b[j] = make_uint4(v.x, v.y, v.z, v.w);
            } else {
                x.b[j] = bp[j * tile_stride + (uint64_t)cc * 64];
            }
        }
#pragma unroll
        for (int t = 0; t < R; t++) x.av[t] = ap[t * tile_stride + (uint64_t)cc * 64];
    };
    mfma_f4 acc[R][CG];
#pragma unroll
    for (int t = 0; t < R; t++)
#pragma unroll
        for (int j = 0; j < CG; j++) acc[t][j] = mfma_f4{0.f, 0.f, 0.f, 0.f};
    // wave w takes chunks w, w + n_waves, ...; ring of DEPTH chunks
    Chunk ring[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; d++) load(ring[d], w + d * n_waves);
    for (uint32_t c = w; c < a.KC; c += DEPTH * n_waves) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            const Chunk cur = ring[d];
            load(ring[d], c + (d + DEPTH) * n_waves);
            __builtin_amdgcn_sched_barrier(0); // the refill is issued before the MFMAs of this chunk
            if (c + d * n_waves < a.KC) { // (wave-uniform)
#pragma unroll
                for (int j = 0; j < CG; j++) {
                    const half8 bv = __builtin_bit_cast(half8, cur.b[j]);
#pragma unroll
                    for (int t = 0; t < R; t++)
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, cur.av[t]), bv, acc[t][j], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int t = 0; t < R; t++)
#pragma unroll
        for (int j = 0; j < CG; j++)
#pragma unroll
            for (int v = 0; v < 4; v++) smem[(((w * R + t) * CG + j) * 4 + v) * 64 + lane] = acc[t][j][v];
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < (uint32_t)R * CG * 256; idx += blockDim.x) {
        const uint32_t t = idx / (CG * 256), j = (idx >> 8) % CG, v = (idx >> 6) & 3, l = idx & 63;
        float sum = smem[((t * CG + j) * 4 + v) * 64 + l];
        for (uint32_t ww = 1; ww < n_waves; ww++) sum += smem[(((ww * R + t) * CG + j) * 4 + v) * 64 + l]; // waves in order: deterministic
        const uint32_t m = (t0 + t) * 16 + 4 * (l >> 4) + v, n = (g + j) * 16 + (l & 15);
        if (m < a.M) P.out[(uint64_t)m * P.out_rs + n] = sum;
    }
}

// f32 B (any strides, device memory) -> MFMA-packed f16. One thread per 16-byte item.
__global__ void __launch_bounds__(kBlock) pack_f16_kernel(const float* __restrict__ b, uint32_t b_rs, uint32_t b_cs,
                                                          uint32_t K, uint32_t N, uint32_t KC, uint4* __restrict__ out) {
    const uint64_t n_items = (uint64_t)(N / 16) * KC * 64;
    for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < n_items; it += (uint64_t)gridDim.x * kBlock) {
        const uint32_t lane = it & 63, i = lane & 15, r = lane >> 4;
        const uint64_t gc = it >> 6;
        const uint32_t c = gc % KC, g = gc / KC;
        const uint32_t n = g * 16 + i;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t k = c * 32 + 8 * r + e;
            v[e] = k < K ? b[(uint64_t)k * b_rs + (uint64_t)n * b_cs] : 0.f;
        }
        const uint2 lo = pack_half4(make_float4(v[0], v[1], v[2], v[3])), hi = pack_half4(make_float4(v[4], v[5], v[6], v[7]));
        out[it] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
}

} // namespace

uint64_t f16_packed_bytes(uint64_t K, uint64_t N) { return (N / 16) * ((K + 31) / 32) * 64 * 16; }

bool f16_packable(uint64_t K, uint64_t N) { return K > 0 && N > 0 && N % 16 == 0; }

void launch_pack_f16(hipStream_t s, const float* b, uint32_t b_rs, uint32_t b_cs, uint32_t K, uint32_t N, void* out) {
    pack_f16_kernel<<<2048, kBlock, 0, s>>>(b, b_rs, b_cs, K, N, (K + 31) / 32, (uint4*)out);
}

static uint32_t f16_tiles_per_wg(uint32_t M) { // m-tiles a workgroup of the A-pre-laid-out kernel carries
    const bool wide = sw().f16_tile2_wide;
    return M > 64 && wide ? 8 : (M > 32 && wide ? 4 : (M > 16 ? 2 : 1));
}
// the pre-laid-out A operand of an M x K matmul has no padding rows / columns (a producer may then write it in place of
// pack_a_f16_kernel: kernels.h a_f16_index)
bool dense_f16_a_unpadded(uint32_t M, uint32_t K) {
    return M > 1 && M % 16 == 0 && K % 32 == 0 && (M / 16) % f16_tiles_per_wg(M) == 0 && dense_f16_scratch_bytes(M, K) != 0;
}
static uint64_t f16_a_bytes(uint32_t M, uint32_t K) { // the pre-laid-out A operand (rounded up to 256 B)
    const uint64_t tiles = (M + 15) / 16, R = f16_tiles_per_wg(M);
    return ((tiles + R - 1) / R * R * ((K + 31) / 32) * 1024 + 255) / 256 * 256;
}
uint64_t dense_f16_scratch_bytes(uint32_t M, uint32_t K) {
    if (!sw().f16_tile2 || M <= 1) return 0;
    return f16_a_bytes(M, K);
}

static void launch_dense_f16_tile2(hipStream_t s, const DenseF16Params* p, uint32_t n) {
    const uint32_t KC = (p[0].K + 31) / 32, R = f16_tiles_per_wg(p[0].M), tiles = cdiv(cdiv(p[0].M, 16), R) * R;
    if (!p[0].reuse_a) {
        const uint64_t items = (uint64_t)tiles * KC * 64;
        pack_a_f16_kernel<<<(uint32_t)std::min<uint64_t>(2048, (items + kBlock - 1) / kBlock), kBlock, 0, s>>>(p[0].a, p[0].M, p[0].K, p[0].a_rs, KC,
                                                                                                             tiles, (uint4*)p[0].scratch);
    }
    const uint32_t waves = std::max(1u, std::min<uint32_t>(KC, (uint32_t)sw().f16_tile2_waves));
    // column groups per workgroup (R <= 2 only: the wide-M forms already amortise A over 4 / 8 m-tiles): as many as keep the grid
    // at >= ~1.3 workgroups per CU, every part a whole number of workgroups
    uint32_t total_groups = 0;
    for (uint32_t t = 0; t < n; t++) total_groups += p[t].N / 16;
    const int env_cg = sw().f16_tile2_cg;
    uint32_t CG = 1;
    if (R <= 2) {
        // measured at M = 32, K = 4096 (tools/bench_matvec.py --fmts f16 --M 32 under ZGML_F16_TILE2_CG, us per launch incl. the A pack; CG = 1 / 2 / 4): N = 4096 13.6 / 16.8 / 22.9,
        // N = 12288 29.9 / 30.0 / 28.5, N = 22016 51.3 / 44.0 / 48.4, N = 32000 68.5 / 55.4 / 56.1; K = 11008, N = 4096 27.8 / 35.3 / 47.2:
        // two groups per workgroup once that still leaves >= 2.5 workgroups per CU (CG = 4 runs one workgroup per CU: 142 registers)
        {
            bool fits = total_groups / 2 >= 640;
            for (uint32_t t = 0; t < n; t++) fits = fits && (p[t].N / 16) % 2 == 0;
            if (fits) CG = 2;
        }
        if (env_cg == 1 || env_cg == 2 || env_cg == 4) {
            bool fits = true;
            for (uint32_t t = 0; t < n; t++) fits = fits && (p[t].N / 16) % (uint32_t)env_cg == 0;
            if (fits) CG = (uint32_t)env_cg;
        }
    }
    F16Args2 a{};
    uint32_t blocks = 0;
    for (uint32_t t = 0; t < n; t++) {
        a.parts[t] = {(const uint4*)p[t].bp, p[t].dst, p[t].dst_rs, blocks};
        blocks += p[t].N / 16 / CG;
    }
    a.ap = (const uint4*)p[0].scratch, a.n_parts = n, a.M = p[0].M, a.KC = KC;
    const dim3 grid(blocks, tiles / R);
    const size_t lds = (size_t)waves * R * CG * 256 * sizeof(float);
    const bool nt = p[0].stream_nt != 0 && tiles / R == 1;
    using Fn2 = void (*)(F16Args2);
#define ZGML_T2(RV) (CG == 4 ? (nt ? (Fn2)dense_f16_tile2_kernel<RV, true, 4> : (Fn2)dense_f16_tile2_kernel<RV, false, 4>)                    \
                     : CG == 2 ? (nt ? (Fn2)dense_f16_tile2_kernel<RV, true, 2> : (Fn2)dense_f16_tile2_kernel<RV, false, 2>)                 \
                               : (nt ? (Fn2)dense_f16_tile2_kernel<RV, true, 1> : (Fn2)dense_f16_tile2_kernel<RV, false, 1>))
    const Fn2 fn = R == 8   ? (nt ? (Fn2)dense_f16_tile2_kernel<8, true> : (Fn2)dense_f16_tile2_kernel<8, false>)
             : R == 4 ? (nt ? (Fn2)dense_f16_tile2_kernel<4, true> : (Fn2)dense_f16_tile2_kernel<4, false>)
             : R == 2 ? ZGML_T2(2)
                      : ZGML_T2(1);
#undef ZGML_T2
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(fn, grid, dim3(waves * 64), lds, s, a);
}

bool dense_f16_can_group(const DenseF16Params& a, const DenseF16Params& b) {
    auto span = [](const float* base, uint32_t M, uint32_t rs, uint32_t n) { return std::make_pair(base, base + (uint64_t)(M - 1) * rs + n); };
    auto apart = [](std::pair<const float*, const float*> x, std::pair<const float*, const float*> y) { return x.second <= y.first || y.second <= x.first; };
    const auto da = span(a.dst, a.M, a.dst_rs, a.N), db = span(b.dst, b.M, b.dst_rs, b.N), in = span(a.a, a.M, a.a_rs, a.K);
    return a.M > 1 && a.scratch && a.scratch == b.scratch && dense_f16_scratch_bytes(a.M, a.K) && a.a == b.a && a.M == b.M && a.K == b.K &&
           a.a_rs == b.a_rs && a.stream_nt == b.stream_nt && apart(da, db) && apart(da, in) && apart(db, in);
}
uint32_t dense_f16_max_group() { return (uint32_t)kMaxF16Parts; }

void launch_dense_f16_group(hipStream_t s, const DenseF16Params* p, uint32_t n) {
    if (n == 1) {
        launch_dense_f16(s, p[0]);
        return;
    }
    launch_dense_f16_tile2(s, p, n);
}

void launch_dense_f16(hipStream_t s, const DenseF16Params& p) {
    if (p.M == 0 || p.N == 0) return;
    if (p.M > 1 && p.scratch && dense_f16_scratch_bytes(p.M, p.K)) {
        launch_dense_f16_tile2(s, &p, 1);
        return;
    }
    F16Args a{(const uint4*)p.bp, p.a, p.dst, p.M, p.K, (p.K + 31) / 32, p.a_rs, p.dst_rs, p.N / 16};
    const uint32_t R = p.M == 1 ? 0 : (p.M > 16 ? 2 : 1);
    // see kDepth in the kernel; the 8-wave R = 2 form only pays while the grid is about one round (N <= 6144)
    const uint32_t depth = R == 2 ? 4 : 8, max_kw = (R == 2 && a.NB2 <= 384) ? 8 : 4;
    uint32_t waves = cdiv(a.KC, depth);
    if (waves > max_kw) waves = max_kw;
    const bool xvec = ((uintptr_t)p.a % 16 == 0) && (p.K % 4 == 0) && (p.M == 1 || p.a_rs % 4 == 0);
    const uint32_t chf = waves * depth * 32;
    using Fn = void (*)(F16Args);
    const bool nt = p.stream_nt != 0;
    if (R == 0) {
        const size_t lds = 2ull * chf * sizeof(float);
        const Fn fn = nt ? (xvec ? (Fn)dense_f16_kernel<0, true, 1, true> : (Fn)dense_f16_kernel<0, false, 1, true>)
                         : (xvec ? (Fn)dense_f16_kernel<0, true, 1, false> : (Fn)dense_f16_kernel<0, false, 1, false>);
        if (lds > 64 * 1024) hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL(fn, dim3(a.NB2, 1), dim3(waves * 64), lds, s, a);
        return;
    }
    // two column groups per workgroup share the staged x chunk — only worth it when the grid stays several
    // rounds deep (measured at M = 32: N = 32000 75 -> 67 us; N = 11008 neutral, N = 4096 slower); the
    // 8-wave R = 2 form has no room for a second wave set
    uint32_t G = sw().f16_groups ? (uint32_t)sw().f16_groups : (a.NB2 >= 1536 ? 2u : 1u);
    if (waves * G > 8) G = 1;
    size_t lds = 2ull * 16 * R * ((chf + 8) / 2) * sizeof(float);
    const size_t red = (size_t)waves * G * R * 256 * sizeof(float);
    if (red > lds) lds = red;
    const dim3 grid(cdiv(a.NB2, G), cdiv(p.M, 16 * R));
    Fn fn;
#define ZGML_F16_PICK(NTV)                                                                                                   \
    (G == 2 ? (R == 2 ? (xvec ? (Fn)dense_f16_kernel<2, true, 2, NTV> : (Fn)dense_f16_kernel<2, false, 2, NTV>)               \
                      : (xvec ? (Fn)dense_f16_kernel<1, true, 2, NTV> : (Fn)dense_f16_kernel<1, false, 2, NTV>))              \
            : (R == 2 ? (xvec ? (Fn)dense_f16_kernel<2, true, 1, NTV> : (Fn)dense_f16_kernel<2, false, 1, NTV>)               \
                      : (xvec ? (Fn)dense_f16_kernel<1, true, 1, NTV> : (Fn)dense_f16_kernel<1, false, 1, NTV>)))
    fn = nt ? ZGML_F16_PICK(true) : ZGML_F16_PICK(false);
#undef ZGML_F16_PICK
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(fn, grid, dim3(waves * G * 64), lds, s, a);
}

} // namespace zgml
