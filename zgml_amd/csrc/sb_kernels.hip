// sb_kernels.hip — the kernels and launchers of the GGUF super-block weights (Q4_K / Q5_K / Q6_K / Q3_K / Q2_K / IQ4_XS); sb_kernels.h states the
// layout, the arithmetic, the six formats and the device functions the kernels below are built from. Nothing here is shared
// with the 32-block formats (and QW_Q4K, "Q4_0 with K on lanes", is none of these).
//
// M = 1. A workgroup of 8 waves owns one super-block column and one K share; wave w streams item column w, lane = k. A lane
// carries 32 column sums (and one min sum; Q2_K: two, one per 16 columns), folded over the lanes by row swaps and DPP row sums in a fixed tree. With fewer item
// columns than the part has wave slots the K range is split over blockIdx.y; every part stores its 256 partial outputs and the
// LAST part to arrive (an integer counter; no float atomics) adds them in part order, so the bytes do not depend on arrival order
// (sb_combine.h).
//   Q5_K, Q6_K, Q3_K, Q2_K, IQ4_XS (sb_round_matvec_kernel): the share is walked in ROUNDS of four 64-k sweeps, and a round issues every load it has
//   — the workgroup's factors first, then per wave four lo items, four hi items and four x — before anything is consumed: 5.25 /
//   6 / 3.25 / 2.25 KiB in flight per wave. While the items fly the 512 threads turn the round's 256 factor entries into f32 products in LDS,
//   once per workgroup. K is split into parts of whole rounds until the grid has about two workgroups per CU (at most 16 parts).
//   Q4_K (sb4_matvec_kernel): sweep by sweep with a one-sweep look-ahead (one dwordx4 of nibbles, one dwordx4 of header — the 8
//   waves of the workgroup read the same headers, so HBM sees each once —, one x), the header unpacked per item.
//
// 2 <= M <= 8, opt-in (ZGML_HIP_OPT_SMALL_M_MATVEC -> QMatmulParams::sb_rows_m). sb_round_rows_kernel<F, R> / sb4_rows_kernel<R>: the
// M = 1 kernels over the R = 2..4 rows of a row group (blockIdx.z; M = 5..8: two groups of cdiv(M, 2) and M / 2 rows, each streaming the
// weights): the quants of a sweep are unpacked once and every weight converted once for R FMAs, the factors in LDS serve all rows. A
// row keeps the M = 1 launch's K split, FMA order, lane fold and part-order combine ([parts][M][N] partials, one counter word per (row
// group, super-block column)), so row m is bit-identical to the M = 1 launch over x[m].
//
// M > 1. A workgroup owns one item column (32 output columns = two 16-column MFMA tiles) and its waves deal the 64-k chunks. Per
// chunk a wave loads 64 items coalesced, turns their bytes ONCE through its own LDS slice into [column][k] order and leaves the
// chunk's two factor rows beside them. B = q - bias, exact in bf16; A = t = x * (d * sc) in f32, split into three bf16 pieces,
// contracted by v_mfma_f32_16x16x32_bf16 with f32 accumulation: three MFMAs per tile and 32 k. The min term is 8 VALU FMAs per
// (row tile, 32 k) beside them, folded over the four lane rows at the end. Waves are folded in wave order.
//   Q5_K, Q6_K, Q3_K, Q2_K, IQ4_XS (sb_matmul_kernel<F, RT>): 8 waves, RT = 1 or 2 row tiles of 16; the turned bytes are the assembled q
//   (IQ4_XS: the table values, looked up once per chunk in front of the turn). The B of a
//   column tile serves both row tiles. With ONE d * sc per item (Q5_K, IQ4_XS) A is formed once per (row tile, 32 k) and feeds both
//   column tiles; with two (Q6_K, Q3_K, Q2_K: a column tile is exactly one scale sub-block) A is per (row tile, column tile), and
//   Q2_K's min sum is per (row tile, column tile) as well.
//   Q4_K (sb4_matmul_kernel): 4 waves, one row tile; the turned byte keeps the nibble pair (columns i and i + 16), so the two
//   column tiles are ONE 8-byte LDS read.
#include "sb_kernels.h"

namespace zgml {
namespace {

constexpr uint32_t kSb4ShareMinSweeps = 4;    // Q4_K: a part's K share is at least this many sweeps (the fold costs about one sweep)
constexpr uint32_t kSb4TargetWaves = 2048;    // ... 256 CUs x 8 waves: split K until the grid has this many waves
constexpr uint32_t kSbRoundTargetWaves = 4096; // rounds: 256 CUs x 2 workgroups x 8 waves: split K until the grid has this many waves ...
constexpr uint32_t kSbRoundMaxParts = 16;     // ... but into at most this many parts (two batches of the combine)
constexpr uint32_t kSb4MmWaves = 4;           // M > 1: waves of a workgroup, dealing the 64-k chunks (Q4_K)
constexpr uint32_t kSbMmWaves = 8;            // ... (Q5_K, Q6_K)

// ── re-pack of the file's super-blocks and the micro-benchmark's synthetic weights: one thread per item ──
template <class F>
__global__ void __launch_bounds__(kBlock) pack_sb_kernel(const uint8_t* __restrict__ raw, typename F::Planes o, uint32_t K, uint32_t N) {
    const uint64_t total = (uint64_t)K * (N / kSbItem);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock) {
        const uint32_t j = (uint32_t)(idx / K), k = (uint32_t)(idx % K), nsb = j >> 3, js = j & 7;
        const uint8_t* blk = raw + ((uint64_t)k * (N / kSbBlock) + nsb) * F::kFileBytes;
        F::pack_item(blk, js, o, idx);
        if (js == 0) F::pack_factors(blk, o, (uint64_t)nsb * K + k);
    }
}
template <class F>
__global__ void __launch_bounds__(kBlock) synth_sb_kernel(typename F::Planes o, uint32_t K, uint32_t N, uint32_t id) {
    const uint64_t total = (uint64_t)K * (N / kSbItem);
    for (uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * kBlock)
        F::synth(o, idx, (uint32_t)idx * 2654435761u + id * 40503u, idx < (uint64_t)K * (N / kSbBlock));
}

// ── M = 1 ──
template <class F>
struct SbMvArgs {
    typename F::Planes w;
    const float* x;
    float* dst;
    float* partial;    // [parts][N] (parts > 1)
    uint32_t* counter; // [N / 256] fan-in words, zero between launches
    uint32_t K, N, share, parts;
};

template <class F, bool NT>
__global__ void __launch_bounds__(kSbWaves * 64) sb_round_matvec_kernel(SbMvArgs<F> a) {
    __shared__ typename F::RoundLds fac; // the round's factors
    __shared__ float red[kSbWaves][kSbItem];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y;
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const typename F::Planes c = F::at(a.w, (uint64_t)(nsb * kSbWaves + w) * a.K, (uint64_t)nsb * a.K);
    const uint32_t fkl = threadIdx.x & (kSbRound - 1), fhalf = threadIdx.x >> 8; // factor duty: one k, half of its factors

    float acc[32];
#pragma unroll
    for (int n = 0; n < 32; n++) acc[n] = 0.f;
    float macc[F::kScales];
#pragma unroll
    for (uint32_t h = 0; h < F::kScales; h++) macc[h] = 0.f;
    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += kSbRound) {
        // every load of the round, the factors first (their wait then leaves the items in flight); past the share: a live
        // address again, with x = 0 and every factor 0
        const typename F::RoundRaw raw = F::round_load(c, min(k0 + fkl, k_hi - 1), fhalf);
        typename F::Lo ql[kSbSweeps];
        typename F::Hi qh[kSbSweeps];
        float xs[kSbSweeps];
#pragma unroll
        for (uint32_t s = 0; s < kSbSweeps; s++) {
            const uint32_t k = k0 + s * kSbSweep + lane, kc = min(k, k_hi - 1);
            ql[s] = F::template load_lo<NT>(c, kc);
            qh[s] = F::template load_hi<NT>(c, kc);
            xs[s] = k < k_hi ? a.x[kc] : 0.f;
        }
        F::round_store(fac, raw, fkl, fhalf, k0 + fkl < k_hi);
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < kSbSweeps; s++) {
            if (k0 + s * kSbSweep >= k_hi) break; // (the same for the whole workgroup)
            float t[F::kScales];
            F::item_factors(fac, w, s * kSbSweep + lane, xs[s], t, macc);
            uint32_t q[8];
            F::quants(ql[s], qh[s], q);
#pragma unroll
            for (int dd = 0; dd < 8; dd++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[4 * dd + b] = __builtin_fmaf(t[F::kScales == 2 ? dd >> 2 : 0], sb_operand<F::kBias>(q[dd], b), acc[4 * dd + b]);
        }
        __syncthreads(); // the next round rewrites fac
    }
    sb_fold_lanes<F::kMin, (int)F::kScales>(acc, macc, red[w], r, i);
    sb_matvec_tail(a, red, &flag, nsb, part);
}

template <bool NT>
__global__ void __launch_bounds__(kSbWaves * 64) sb4_matvec_kernel(SbMvArgs<Sb4> a) {
    __shared__ float red[kSbWaves][kSbItem];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y;
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const Sb4::Planes c = Sb4::at(a.w, (uint64_t)(nsb * kSbWaves + w) * a.K, (uint64_t)nsb * a.K);

    struct Item {
        uint4 q, h;
        float x;
    };
    auto load = [&](uint32_t k0) {
        const uint32_t k = k0 + lane, kc = min(k, k_hi - 1); // past the share: a live item again, with x = 0
        Item it;
        it.q = wload<NT>(c.lo + kc);
        it.h = c.hdr[kc];
        it.x = k < k_hi ? a.x[kc] : 0.f;
        return it;
    };
    float acc[32];
#pragma unroll
    for (int n = 0; n < 32; n++) acc[n] = 0.f;
    float macc[1] = {0.f};
    auto consume = [&](const Item& it) {
        const Q4kFactors f = sb_header_factors(it.h, w);
        const float t = it.x * f.scale;
        macc[0] = __builtin_fmaf(it.x, f.min, macc[0]);
        uint32_t q[8];
        Sb4::quants(it.q, q);
#pragma unroll
        for (int dd = 0; dd < 4; dd++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                acc[4 * dd + b] = __builtin_fmaf(t, sb_operand<0>(q[dd], b), acc[4 * dd + b]);
                acc[16 + 4 * dd + b] = __builtin_fmaf(t, sb_operand<0>(q[4 + dd], b), acc[16 + 4 * dd + b]);
            }
    };
    Item cur = load(k_lo);
    for (uint32_t k0 = k_lo + kSbSweep; k0 < k_hi; k0 += kSbSweep) { // the next sweep's loads fly while this one is consumed
        const Item nxt = load(k0);
        consume(cur);
        cur = nxt;
    }
    consume(cur);
    sb_fold_lanes<true, 1>(acc, macc, red[w], r, i);
    sb_matvec_tail(a, red, &flag, nsb, part);
}

// the K split of an M = 1 launch: parts and the k of each (Q4_K: a multiple of the sweep; rounds: whole rounds). `split` = false:
// the launch has no scratch to split through
struct SbSplit {
    uint32_t parts, share;
};
SbSplit sb4_split(uint32_t K, uint32_t N, bool split) {
    const uint32_t sweeps = cdiv(K, kSbSweep), want = cdiv(kSb4TargetWaves, N / kSbItem);
    const uint32_t per = std::max(kSb4ShareMinSweeps, cdiv(sweeps, want));
    const uint32_t parts = split && N / kSbBlock <= kQmmCounterBytes / 4 ? cdiv(sweeps, per) : 1; // (one counter word per super-block column)
    return parts > 1 ? SbSplit{parts, per * kSbSweep} : SbSplit{1, sweeps * kSbSweep};
}
SbSplit sb_round_split(uint32_t K, uint32_t N, bool split) {
    const uint32_t rounds = cdiv(K, kSbRound), want = cdiv(kSbRoundTargetWaves, N / kSbItem);
    const uint32_t per = std::max(cdiv(rounds, want), cdiv(rounds, kSbRoundMaxParts));
    const uint32_t parts = split && N / kSbBlock <= kQmmCounterBytes / 4 ? cdiv(rounds, per) : 1;
    return parts > 1 ? SbSplit{parts, per * kSbRound} : SbSplit{1, rounds * kSbRound};
}
template <class F>
SbSplit sb_split(uint32_t K, uint32_t N, bool split) {
    return F::kRound ? sb_round_split(K, N, split) : sb4_split(K, N, split);
}

// ── 2 <= M <= 8: the M = 1 kernels over R rows at once ──
// A row group of R rows (blockIdx.z) streams the weights once: per sweep the quants are unpacked once and every weight converted
// once, and the conversion feeds R FMAs. Every row keeps the M = 1 kernel's own split, FMA order, lane fold and part-order
// combine, so row m of the launch is bit-identical to the M = 1 launch over x[m].
template <class F>
struct SbRowsArgs {
    typename F::Planes w;
    const float* x;
    float* dst;
    float* partial;    // [parts][M][N] (parts > 1)
    uint32_t* counter; // [row groups][N / 256] fan-in words, zero between launches
    uint32_t M, K, N, in_rs, dst_rs, share, parts;
};

template <class F, int R, bool NT>
__global__ void __launch_bounds__(kSbWaves * 64) sb_round_rows_kernel(SbRowsArgs<F> a) {
    __shared__ typename F::RoundLds fac; // the round's factors, shared by the rows
    __shared__ float red[R][kSbWaves][kSbItem];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y, m0 = blockIdx.z * R, rows = min((uint32_t)R, a.M - m0);
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const typename F::Planes c = F::at(a.w, (uint64_t)(nsb * kSbWaves + w) * a.K, (uint64_t)nsb * a.K);
    const uint32_t fkl = threadIdx.x & (kSbRound - 1), fhalf = threadIdx.x >> 8;
    const float* xr[R]; // (a row past the group's last: the last row of the launch again, never stored)
#pragma unroll
    for (int rr = 0; rr < R; rr++) xr[rr] = a.x + (uint64_t)min(m0 + rr, a.M - 1) * a.in_rs;

    float acc[R][32], macc[R][F::kScales];
#pragma unroll
    for (int rr = 0; rr < R; rr++) {
#pragma unroll
        for (int n = 0; n < 32; n++) acc[rr][n] = 0.f;
#pragma unroll
        for (uint32_t h = 0; h < F::kScales; h++) macc[rr][h] = 0.f;
    }
    for (uint32_t k0 = k_lo; k0 < k_hi; k0 += kSbRound) {
        const typename F::RoundRaw raw = F::round_load(c, min(k0 + fkl, k_hi - 1), fhalf);
        typename F::Lo ql[kSbSweeps];
        typename F::Hi qh[kSbSweeps];
        float xs[kSbSweeps][R];
#pragma unroll
        for (uint32_t s = 0; s < kSbSweeps; s++) {
            const uint32_t k = k0 + s * kSbSweep + lane, kc = min(k, k_hi - 1);
            ql[s] = F::template load_lo<NT>(c, kc);
            qh[s] = F::template load_hi<NT>(c, kc);
#pragma unroll
            for (int rr = 0; rr < R; rr++) xs[s][rr] = k < k_hi ? xr[rr][kc] : 0.f;
        }
        F::round_store(fac, raw, fkl, fhalf, k0 + fkl < k_hi);
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < kSbSweeps; s++) {
            if (k0 + s * kSbSweep >= k_hi) break; // (the same for the whole workgroup)
            float t[R][F::kScales];
#pragma unroll
            for (int rr = 0; rr < R; rr++) F::item_factors(fac, w, s * kSbSweep + lane, xs[s][rr], t[rr], macc[rr]);
            uint32_t q[8];
            F::quants(ql[s], qh[s], q);
#pragma unroll
            for (int dd = 0; dd < 8; dd++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const float v = sb_operand<F::kBias>(q[dd], b); // one conversion, R FMAs
#pragma unroll
                    for (int rr = 0; rr < R; rr++) acc[rr][4 * dd + b] = __builtin_fmaf(t[rr][F::kScales == 2 ? dd >> 2 : 0], v, acc[rr][4 * dd + b]);
                }
        }
        __syncthreads(); // the next round rewrites fac
    }
#pragma unroll
    for (int rr = 0; rr < R; rr++) sb_fold_lanes<F::kMin, (int)F::kScales>(acc[rr], macc[rr], red[rr][w], r, i);
    sb_rows_tail<R>(a, red, &flag, nsb, part, m0, rows);
}

template <int R, bool NT>
__global__ void __launch_bounds__(kSbWaves * 64) sb4_rows_kernel(SbRowsArgs<Sb4> a) {
    __shared__ float red[R][kSbWaves][kSbItem];
    __shared__ uint32_t flag;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t nsb = blockIdx.x, part = blockIdx.y, m0 = blockIdx.z * R, rows = min((uint32_t)R, a.M - m0);
    const uint32_t k_lo = part * a.share, k_hi = min(a.K, k_lo + a.share); // k_lo < K: the host sizes `parts` so
    const Sb4::Planes c = Sb4::at(a.w, (uint64_t)(nsb * kSbWaves + w) * a.K, (uint64_t)nsb * a.K);
    const float* xr[R];
#pragma unroll
    for (int rr = 0; rr < R; rr++) xr[rr] = a.x + (uint64_t)min(m0 + rr, a.M - 1) * a.in_rs;

    struct Item {
        uint4 q, h;
        float x[R];
    };
    auto load = [&](uint32_t k0) {
        const uint32_t k = k0 + lane, kc = min(k, k_hi - 1); // past the share: a live item again, with x = 0
        Item it;
        it.q = wload<NT>(c.lo + kc);
        it.h = c.hdr[kc];
#pragma unroll
        for (int rr = 0; rr < R; rr++) it.x[rr] = k < k_hi ? xr[rr][kc] : 0.f;
        return it;
    };
    float acc[R][32], macc[R][1];
#pragma unroll
    for (int rr = 0; rr < R; rr++) {
#pragma unroll
        for (int n = 0; n < 32; n++) acc[rr][n] = 0.f;
        macc[rr][0] = 0.f;
    }
    auto consume = [&](const Item& it) {
        const Q4kFactors f = sb_header_factors(it.h, w); // the header unpacked once for the rows
        float t[R];
#pragma unroll
        for (int rr = 0; rr < R; rr++) {
            t[rr] = it.x[rr] * f.scale;
            macc[rr][0] = __builtin_fmaf(it.x[rr], f.min, macc[rr][0]);
        }
        uint32_t q[8];
        Sb4::quants(it.q, q);
#pragma unroll
        for (int dd = 0; dd < 4; dd++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const float v0 = sb_operand<0>(q[dd], b), v1 = sb_operand<0>(q[4 + dd], b);
#pragma unroll
                for (int rr = 0; rr < R; rr++) {
                    acc[rr][4 * dd + b] = __builtin_fmaf(t[rr], v0, acc[rr][4 * dd + b]);
                    acc[rr][16 + 4 * dd + b] = __builtin_fmaf(t[rr], v1, acc[rr][16 + 4 * dd + b]);
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
#pragma unroll
    for (int rr = 0; rr < R; rr++) sb_fold_lanes<true, 1>(acc[rr], macc[rr], red[rr][w], r, i);
    sb_rows_tail<R>(a, red, &flag, nsb, part, m0, rows);
}

// ── M > 1 ──
template <class F>
struct SbMmArgs {
    typename F::Planes w;
    const float* x;
    float* dst;
    uint32_t M, K, N, in_rs, dst_rs;
};

template <class F, int RT, bool XVEC, bool NT>
__global__ void __launch_bounds__(kSbMmWaves * 64) sb_matmul_kernel(SbMmArgs<F> a) {
    __shared__ __attribute__((aligned(16))) uint8_t turned[kSbMmWaves][32 * 64]; // per wave: the chunk's q bytes, [column][k]
    __shared__ __attribute__((aligned(16))) float fs[kSbMmWaves][F::kScales][64]; // ... and its d * sc: one row, or one per column tile
    __shared__ __attribute__((aligned(16))) float fm[kSbMmWaves][F::kScales][64]; // ... and its dmin * m beside each (F::kMin)
    __shared__ float fold[kSbMmWaves][RT * 2][4][64];
    __shared__ float mins[kSbMmWaves][RT * F::kScales][16];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t j = blockIdx.x, nsb = j >> 3, js = j & 7, m0 = blockIdx.y * 16 * RT;
    const typename F::Planes c = F::at(a.w, (uint64_t)j * a.K, (uint64_t)nsb * a.K);
    const float* xrow[RT]; // A operand: lane (r, i) holds row i, k = 8 r .. 8 r + 7 of a 32-k step
    sb_f4 acc[RT][2];
    float macc[RT][F::kScales]; // the min sums: per row tile, or per (row tile, column tile)
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        xrow[rt] = a.x + (uint64_t)min(m0 + 16 * rt + i, a.M - 1) * a.in_rs;
        acc[rt][0] = acc[rt][1] = sb_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t h = 0; h < F::kScales; h++) macc[rt][h] = 0.f;
    }
    const uint32_t chunks = (a.K + 63) / 64;
    for (uint32_t ch = w; ch < chunks; ch += kSbMmWaves) {
        const uint32_t k = ch * 64 + lane, kc = min(k, a.K - 1);
        const typename F::Lo lo = F::template load_lo<NT>(c, kc);
        const typename F::Hi hi = F::template load_hi<NT>(c, kc);
        float f[F::kScales], mn[F::kScales];
        F::chunk_factors(c, kc, js, f, mn);
#pragma unroll
        for (uint32_t h = 0; h < F::kScales; h++) {
            fs[w][h][lane] = k < a.K ? f[h] : 0.f; // rows past K: t = 0 and no min
            if constexpr (F::kMin) fm[w][h][lane] = k < a.K ? mn[h] : 0.f;
        }
        uint32_t q[8];
        F::quants(lo, hi, q);
        sb_turn(turned[w], q, lane);
        sb_wave_lds_fence();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t kl = 32 * s + 8 * r, kb = ch * 64 + kl;
            if constexpr (F::kScales == 1) { // one A per row tile, for both column tiles
                float sv[8], mv[8];
                sb_read8(&fs[w][0][kl], sv);
                if constexpr (F::kMin) sb_read8(&fm[w][0][kl], mv); // (IQ4_XS: one scale and no min row)
                sb_bf8 qv[2]; // B of the two column tiles: column 16 ct + i
#pragma unroll
                for (int ct = 0; ct < 2; ct++) qv[ct] = sb_fragment<F::kBias>(sb_turned8(turned[w], 16 * ct + i, kl));
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    float xv[8];
                    sb_load_x8<XVEC>(xrow[rt], kb, a.K, xv);
                    sb_bf8 h1, h2, h3;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float t = xv[e] * sv[e];
                        if constexpr (F::kMin) macc[rt][0] = __builtin_fmaf(xv[e], mv[e], macc[rt][0]);
                        sb_split3(t, h1, h2, h3, e);
                    }
#pragma unroll
                    for (int ct = 0; ct < 2; ct++) acc[rt][ct] = sb_mfma3(h1, h2, h3, qv[ct], acc[rt][ct]);
                }
            } else { // one A per (row tile, column tile): a column tile is one scale sub-block
                float xv[RT][8];
#pragma unroll
                for (int rt = 0; rt < RT; rt++) sb_load_x8<XVEC>(xrow[rt], kb, a.K, xv[rt]);
#pragma unroll
                for (int ct = 0; ct < 2; ct++) {
                    const uint2 bb = sb_turned8(turned[w], 16 * ct + i, kl);
                    float sv[8], mv[8];
                    sb_read8(&fs[w][ct][kl], sv);
                    if constexpr (F::kMin) sb_read8(&fm[w][ct][kl], mv); // the column tile's own dmin * m
                    const sb_bf8 qv = sb_fragment<F::kBias>(bb);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        sb_bf8 h1, h2, h3;
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            if constexpr (F::kMin) macc[rt][ct] = __builtin_fmaf(xv[rt][e], mv[e], macc[rt][ct]);
                            sb_split3(xv[rt][e] * sv[e], h1, h2, h3, e);
                        }
                        acc[rt][ct] = sb_mfma3(h1, h2, h3, qv, acc[rt][ct]);
                    }
                }
            }
        }
        sb_wave_lds_fence(); // the reads above stay above the next chunk's writes
    }
    sb_fold_waves<kSbMmWaves, RT, F::kMin, (int)F::kScales>(a, fold, mins, acc, macc, j, m0);
}

template <bool XVEC, bool NT>
__global__ void __launch_bounds__(kSb4MmWaves * 64) sb4_matmul_kernel(SbMmArgs<Sb4> a) {
    __shared__ __attribute__((aligned(16))) uint8_t turned[kSb4MmWaves][16 * 64]; // per wave: byte b of the chunk's items, [b][k]
    __shared__ __attribute__((aligned(16))) float fs[kSb4MmWaves][64], fm[kSb4MmWaves][64]; // ... and their d * sc, dmin * m
    __shared__ float fold[kSb4MmWaves][2][4][64];
    __shared__ float mins[kSb4MmWaves][1][16];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane >> 4, i = lane & 15;
    const uint32_t j = blockIdx.x, nsb = j >> 3, js = j & 7, m0 = blockIdx.y * 16;
    const Sb4::Planes c = Sb4::at(a.w, (uint64_t)j * a.K, (uint64_t)nsb * a.K);
    const float* xrow = a.x + (uint64_t)min(m0 + i, a.M - 1) * a.in_rs; // A operand: lane (r, i) holds row i, k = 8 r .. 8 r + 7 of a 32-k step
    sb_f4 acc[1][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
    float macc[1][1] = {{0.f}};
    const uint32_t chunks = (a.K + 63) / 64;
    for (uint32_t ch = w; ch < chunks; ch += kSb4MmWaves) {
        const uint32_t k = ch * 64 + lane, kc = min(k, a.K - 1);
        const uint4 q = wload<NT>(c.lo + kc);
        const Q4kFactors f = sb_header_factors(c.hdr[kc], js);
        fs[w][lane] = k < a.K ? f.scale : 0.f; // rows past K: t = 0 and no min
        fm[w][lane] = k < a.K ? f.min : 0.f;
        const uint32_t dw[4] = {q.x, q.y, q.z, q.w};
        sb_turn(turned[w], dw, lane);
        sb_wave_lds_fence();
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint32_t kl = 32 * s + 8 * r, kb = ch * 64 + kl;
            const uint2 bb = sb_turned8(turned[w], i, kl);
            float sv[8], mv[8], xv[8];
            sb_read8(&fs[w][kl], sv);
            sb_read8(&fm[w][kl], mv);
            sb_load_x8<XVEC>(xrow, kb, a.K, xv);
            const uint32_t bw[2] = {bb.x, bb.y};
            sb_bf8 h1, h2, h3, q0, q1;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float t = xv[e] * sv[e];
                macc[0][0] = __builtin_fmaf(xv[e], mv[e], macc[0][0]);
                sb_split3(t, h1, h2, h3, e);
                const uint32_t byte = (bw[e >> 2] >> (8 * (e & 3))) & 255u;
                q0[e] = (__bf16)(float)(byte & 15u); // column i
                q1[e] = (__bf16)(float)(byte >> 4);  // column i + 16
            }
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, q0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, q1, acc[0][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, q0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, q1, acc[0][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, q0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, q1, acc[0][1], 0, 0, 0);
        }
        sb_wave_lds_fence(); // the reads above stay above the next chunk's writes
    }
    sb_fold_waves<kSb4MmWaves, 1, true, 1>(a, fold, mins, acc, macc, j, m0);
}

// ── launches ──
template <class F, bool NT>
void launch_mv(hipStream_t s, const SbMvArgs<F>& a) {
    const dim3 grid(a.N / kSbBlock, a.parts);
    if constexpr (F::kRound)
        sb_round_matvec_kernel<F, NT><<<grid, kSbWaves * 64, 0, s>>>(a);
    else
        sb4_matvec_kernel<NT><<<grid, kSbWaves * 64, 0, s>>>(a);
}
template <class F, int RT, bool XVEC, bool NT>
void launch_mm(hipStream_t s, const SbMmArgs<F>& a) {
    const dim3 grid(a.N / kSbItem, cdiv(a.M, 16 * RT));
    if constexpr (F::kRound)
        sb_matmul_kernel<F, RT, XVEC, NT><<<grid, kSbMmWaves * 64, 0, s>>>(a);
    else
        sb4_matmul_kernel<XVEC, NT><<<grid, kSb4MmWaves * 64, 0, s>>>(a);
}
template <class F, int RT>
void launch_mm(hipStream_t s, const SbMmArgs<F>& a, bool xvec, bool nt) {
    if (xvec)
        nt ? launch_mm<F, RT, true, true>(s, a) : launch_mm<F, RT, true, false>(s, a);
    else
        nt ? launch_mm<F, RT, false, true>(s, a) : launch_mm<F, RT, false, false>(s, a);
}

// the row groups of an M-row launch: one of M rows up to kSbRowsPerGroup, else two of cdiv(M, 2) and M / 2 (blockIdx.z)
constexpr uint32_t sb_row_groups(uint32_t M) { return M > kSbRowsPerGroup ? 2 : 1; }
template <class F, int R, bool NT>
void launch_rows(hipStream_t s, const SbRowsArgs<F>& a) {
    const dim3 grid(a.N / kSbBlock, a.parts, sb_row_groups(a.M));
    if constexpr (F::kRound)
        sb_round_rows_kernel<F, R, NT><<<grid, kSbWaves * 64, 0, s>>>(a);
    else
        sb4_rows_kernel<R, NT><<<grid, kSbWaves * 64, 0, s>>>(a);
}
template <class F, int R>
void launch_rows(hipStream_t s, const SbRowsArgs<F>& a, bool nt) {
    nt ? launch_rows<F, R, true>(s, a) : launch_rows<F, R, false>(s, a);
}

// does an M-row launch over a K x N weight take the row kernels under the bound `max_m`? One counter word per (row group,
// super-block column) has to fit the head — the condition under which the M = 1 launch splits K, times the groups —, so a
// routed row always has its M = 1 split
bool sb_rows_take(uint32_t N, uint32_t M, uint32_t max_m) {
    return M >= 2 && M <= std::min(max_m, 2 * kSbRowsPerGroup) && (uint64_t)sb_row_groups(M) * (N / kSbBlock) <= kQmmCounterBytes / 4;
}

template <class F>
void launch_matmul(hipStream_t s, const QWeightDev& w, const QMatmulParams& p, float* scratch) {
    if (p.K != w.K || p.N != w.N) {
        fprintf(stderr, "[zgml_hip] ERROR: a %u x %u matmul over a %u x %u %s weight: not launched\n", p.K, p.N, w.K, w.N, F::kName);
        return;
    }
    if (sb_rows_take(w.N, p.M, p.sb_rows_m)) {
        const SbSplit sp = sb_split<F>(w.K, w.N, true); // the M = 1 launch's own split
        if (sp.parts > 1 && !scratch) {
            fprintf(stderr, "[zgml_hip] ERROR: a %u-row %s launch that splits K has no scratch: not launched\n", p.M, F::kName);
            return;
        }
        const SbRowsArgs<F> a{F::planes(w), p.input, p.dst, scratch, scratch ? (uint32_t*)((char*)scratch - kQmmScratchHead) : nullptr, p.M, w.K, w.N, p.in_rs, p.dst_rs, sp.share, sp.parts};
        switch (cdiv(p.M, sb_row_groups(p.M))) { // rows of the (first) group
        case 2: return launch_rows<F, 2>(s, a, w.stream_nt != 0);
        case 3: return launch_rows<F, 3>(s, a, w.stream_nt != 0);
        default: return launch_rows<F, 4>(s, a, w.stream_nt != 0);
        }
    }
    if (p.M == 1) {
        const SbSplit sp = sb_split<F>(w.K, w.N, scratch != nullptr);
        const SbMvArgs<F> a{F::planes(w), p.input, p.dst, scratch, scratch ? (uint32_t*)((char*)scratch - kQmmScratchHead) : nullptr, w.K, w.N, sp.share, sp.parts};
        w.stream_nt ? launch_mv<F, true>(s, a) : launch_mv<F, false>(s, a);
        return;
    }
    const SbMmArgs<F> a{F::planes(w), p.input, p.dst, p.M, w.K, w.N, p.in_rs, p.dst_rs};
    const bool xvec = ((uintptr_t)p.input % 16 == 0) && (p.K % 4 == 0) && (p.in_rs % 4 == 0);
    const bool nt = w.stream_nt != 0 && p.M <= F::kNtMaxM;
    if constexpr (F::kRound) // (Q4_K's kernel has one row tile)
        if (p.M > 16) return launch_mm<F, 2>(s, a, xvec, nt);
    launch_mm<F, 1>(s, a, xvec, nt);
}

// fn(F{}) for the format struct F of a super-block QWFormat
template <class Fn>
auto sb_dispatch(QWFormat format, Fn fn) {
    switch (format) {
    case Sb4::kFormat: return fn(Sb4{});
    case Sb5::kFormat: return fn(Sb5{});
    case Sb6::kFormat: return fn(Sb6{});
    case Sb3::kFormat: return fn(Sb3{});
    case Sb2::kFormat: return fn(Sb2{});
    case Sb4x::kFormat: return fn(Sb4x{});
    default: break;
    }
    fprintf(stderr, "[zgml_hip] ERROR: weight format %u is no super-block format\n", (uint32_t)format);
    abort();
}

} // namespace

bool sb_applies(uint64_t K, uint64_t N) { return K >= 1 && K < (1ull << 31) && N >= kSbBlock && N % kSbBlock == 0 && N < (1ull << 31); }

void sb_packed_bytes(QWFormat format, uint64_t K, uint64_t N, uint64_t* qs_bytes, uint64_t* sc_bytes) {
    sb_dispatch(format, [&](auto f) {
        *qs_bytes = K * (N / kSbItem) * f.kItemBytes;
        *sc_bytes = K * (N / kSbBlock) * f.kFactorBytes;
    });
}

void launch_pack_sb(hipStream_t s, const uint8_t* raw_blocks, const QWeightDev& out) {
    sb_dispatch(out.format, [&](auto f) { pack_sb_kernel<decltype(f)><<<2048, kBlock, 0, s>>>(raw_blocks, f.planes(out), out.K, out.N); });
}

void launch_synth_sb(hipStream_t s, const QWeightDev& w, uint32_t matrix_id) {
    sb_dispatch(w.format, [&](auto f) { synth_sb_kernel<decltype(f)><<<2048, kBlock, 0, s>>>(f.planes(w), w.K, w.N, matrix_id); });
}

uint32_t sb_rows_bound(QWFormat format, uint32_t option) {
    if (option != 1) return std::min(option, 2 * kSbRowsPerGroup);
    return sb_dispatch(format, [](auto f) { return f.kRowsRoutedM; });
}

bool sb_rows_routed(const QWeightDev& w, uint32_t M, uint32_t max_m) { return sb_rows_take(w.N, M, max_m); }

uint64_t sb_scratch_bytes(const QWeightDev& w, uint32_t M) {
    if (M != 1 && !sb_rows_routed(w, M, M)) return 0; // (the partials of M rows under a bound >= M: a caller with a smaller bound asks for its bound's rows, or for none)
    const SbSplit sp = sb_dispatch(w.format, [&](auto f) { return sb_split<decltype(f)>(w.K, w.N, true); });
    return sp.parts > 1 ? (uint64_t)sp.parts * M * w.N * sizeof(float) : 0;
}

void launch_sb_matmul(hipStream_t s, const QWeightDev& w, const QMatmulParams& p, float* scratch) {
    sb_dispatch(w.format, [&](auto f) { launch_matmul<decltype(f)>(s, w, p, scratch); });
}

} // namespace zgml
