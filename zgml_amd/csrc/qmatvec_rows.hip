// qmatvec_rows.hip — the K-on-lanes Q4_0 mat-vec over R = 2..8 activation rows (batched decode: one row per sequence).
//
// Layout, column ownership and K split are those of qmatvec_kon_kernel (qmatvec.hip, "K ON LANES"): a workgroup owns the 16
// columns of group g and all of K, a lane owns the k-pairs p = tid, tid + stride, ...; per item it loads ONE 16-byte weight
// unit and ONE scale pair, and R pairs of x (row r at input + r * in_rs). The fp8 converts of a weight dword are issued once
// and their four results feed R sets of packed FMAs, so the per-weight VALU work is 3/8 + R/2 instructions instead of the
// R * (3/8 + 1/2) of R mat-vecs, and every weight byte is read once per step instead of once per sequence. Per row the
// arithmetic is the M = 1 kernel's, term by term: t = fl(scale * x) (reference.zig:552), the chain over the lane's items in
// the same order, the -8 of the offset-binary nibbles through the row's own sum of t (kon_fold_wave), the same wave fold;
// an all-(q = 8) weight therefore gives exactly 0 in every row. The waves' column sums meet in LDS as red[row][wave][column]
// and are added in wave order.
// Opt-in (ZGML_HIP_OPT_SMALL_M_MATVEC): compile_program packs a weight K-on-lanes when every qmatmul over it has M <= 8, and
// launch_qmatmul sends 2 <= M <= 8 over such a weight here. No prologue, no epilogue, one matrix per launch.
#include "qmv_common.h"
#include "switches.h"

#include <algorithm>

namespace zgml {
namespace {

struct KonRowsArgs {
    const uint4* qs;
    const uint32_t* sc;
    float* dst;
    const float* input;
    uint32_t in_rs, dst_rs, K, NB2;
};

// the four column pairs of one dword, converted once (c0: columns b, b + 1 of the low nibbles' bytes 0 / 1, c1: bytes 2 / 3,
// c2 / c3: the high nibbles) ...
__device__ __forceinline__ void kon_rows_cvt(f32x2& c0, f32x2& c1, f32x2& c2, f32x2& c3, uint32_t dw) {
    uint32_t lo, hi;
    asm("v_and_b32_e32 %4, 0xf0f0f0f, %6\n\t"
        "v_lshrrev_b32_e32 %5, 4, %6\n\t"
        "v_cvt_pk_f32_fp8_e32 %0, %4\n\t"
        "v_and_b32_e32 %5, 0xf0f0f0f, %5\n\t"
        "v_cvt_pk_f32_fp8_sdwa %1, %4 src0_sel:WORD_1\n\t"
        "v_cvt_pk_f32_fp8_e32 %2, %5\n\t"
        "v_cvt_pk_f32_fp8_sdwa %3, %5 src0_sel:WORD_1"
        : "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(c3), "=&v"(lo), "=&v"(hi)
        : "v"(dw));
}
// ... and one row's share: four packed FMAs. `tt` = (t of k = 2p, t of k = 2p + 1) of that row; HI picks which half is
// broadcast to both halves of the FMA (op_sel: the low result's source half, op_sel_hi: the high result's).
template <bool HI>
__device__ __forceinline__ void kon_rows_fma(f32x2& a0, f32x2& a1, f32x2& a2, f32x2& a3, f32x2 c0, f32x2 c1, f32x2 c2, f32x2 c3, f32x2 tt) {
    if (HI)
        asm("v_pk_fma_f32 %0, %4, %8, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %1, %5, %8, %1 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %2, %6, %8, %2 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
            "v_pk_fma_f32 %3, %7, %8, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
            : "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(tt));
    else
        asm("v_pk_fma_f32 %0, %4, %8, %0 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %1, %5, %8, %1 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %2, %6, %8, %2 op_sel_hi:[1,0,1]\n\t"
            "v_pk_fma_f32 %3, %7, %8, %3 op_sel_hi:[1,0,1]"
            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
            : "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(tt));
}

template <int R, bool HI>
__device__ __forceinline__ void kon_rows_dword(f32x2 (&acc)[R][8], int c, uint32_t dw, const f32x2 (&tt)[R]) {
    f32x2 c0, c1, c2, c3;
    kon_rows_cvt(c0, c1, c2, c3, dw);
#pragma unroll
    for (int r = 0; r < R; r++) kon_rows_fma<HI>(acc[r][c], acc[r][c + 1], acc[r][c + 2], acc[r][c + 3], c0, c1, c2, c3, tt[r]);
    __builtin_amdgcn_sched_barrier(0); // (the next dword's converts stay behind this one's FMAs: four temporaries live, not sixteen)
}

template <int R, bool NT, bool XV>
struct KonRowsItem { // one lane's share of a step: k = 2p, 2p + 1 x 16 columns x R rows
    uint4 wq;
    uint32_t s2;
    f32x2 x[R];
    // unconditional, clamped; XV: every row is 8-byte aligned and K is even
    __device__ __forceinline__ void load(const uint4* qs, const uint32_t* sc, const float* in, uint32_t in_rs, uint32_t p, uint32_t p_last, uint32_t K) {
        const uint32_t pd = min(p, p_last);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float* a = in + (uint64_t)r * in_rs;
            if (XV)
                x[r] = *(const f32x2*)(a + 2 * pd);
            else
                x[r] = f32x2{a[2 * pd], a[min(2 * pd + 1, K - 1)]};
        }
        s2 = sc[pd];
        wq = wload<NT>(qs + pd);
    }
    __device__ __forceinline__ void compute(uint32_t pd, uint32_t P, uint32_t K, f32x2 (&acc)[R][8], float (&T)[R]) const {
        const bool ok0 = pd < P, ok1 = ok0 && (XV || 2 * pd + 1 < K);
        const __half2 h = *(const __half2*)&s2;
        const float s0 = __low2float(h), s1 = __high2float(h);
        f32x2 tt[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float t0 = s0 * (ok0 ? x[r].x : 0.f), t1 = s1 * (ok1 ? x[r].y : 0.f); // (scale * x as the reference rounds it, reference.zig:552)
            T[r] += t0;
            T[r] += t1;
            tt[r] = f32x2{t0, t1};
        }
        kon_rows_dword<R, false>(acc, 0, wq.x, tt);
        kon_rows_dword<R, false>(acc, 4, wq.y, tt);
        kon_rows_dword<R, true>(acc, 0, wq.z, tt);
        kon_rows_dword<R, true>(acc, 4, wq.w, tt);
    }
};

// DEPTH items per lane in flight, refilled one by one as in qmatvec_kon_body. Registers: 16 accumulators + 1 sum per row,
// DEPTH x (5 + 2 R) of loads, 2 R of multipliers, 8 of converts: R = 8, DEPTH = 2 -> ~200, inside the 256 a 512-thread bound leaves.
template <int R, int DEPTH, bool NT, bool XV>
__global__ void __launch_bounds__(512) qmatvec_kon_rows_kernel(KonRowsArgs a) {
    __shared__ float red[R * kMaxWaves * 16];
    const uint32_t K = a.K, P = (K + 1) >> 1, p_last = P - 1;
    const uint32_t n_waves = blockDim.x >> 6, stride = blockDim.x;
    const uint32_t g = column_group(blockIdx.x, a.NB2);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, rr = lane >> 4, i = lane & 15;
    const uint4* qs = a.qs + (uint64_t)g * P;
    const uint32_t* sc = a.sc + (uint64_t)(g >> 1) * P;
    const uint32_t n_groups = (P + stride * DEPTH - 1) / (stride * DEPTH);
    uint32_t p = threadIdx.x;
    KonRowsItem<R, NT, XV> it[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; d++) it[d].load(qs, sc, a.input, a.in_rs, p + d * stride, p_last, K);
    __builtin_amdgcn_sched_barrier(0);
    f32x2 acc[R][8];
    float T[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        T[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; c++) acc[r][c] = f32x2{0.f, 0.f};
    }
    for (uint32_t gi = 1; gi < n_groups; gi++) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            it[d].compute(p + d * stride, P, K, acc, T);
            __builtin_amdgcn_sched_barrier(0); // (hipcc otherwise moves the refills to the end of the body)
            it[d].load(qs, sc, a.input, a.in_rs, p + (DEPTH + d) * stride, p_last, K);
            __builtin_amdgcn_sched_barrier(0);
        }
        p += DEPTH * stride;
    }
#pragma unroll
    for (int d = 0; d < DEPTH; d++) it[d].compute(p + d * stride, P, K, acc, T);
#pragma unroll
    for (int r = 0; r < R; r++) kon_fold_wave(acc[r], T[r], red + (r * kMaxWaves + w) * 16, rr, i);
    __syncthreads();
    // row r, column c of the group: the waves' sums in wave order, times the 2^9 of the fp8 converts
    for (uint32_t o = threadIdx.x; o < (uint32_t)R * 16; o += blockDim.x) {
        const uint32_t r = o >> 4, c = o & 15;
        float v = 0.f;
        for (uint32_t ww = 0; ww < n_waves; ww++) v += red[(r * kMaxWaves + ww) * 16 + c];
        a.dst[(uint64_t)r * a.dst_rs + g * 16 + c] = v * 512.0f;
    }
}

using RowsFn = void (*)(KonRowsArgs);

template <int R, int DEPTH>
RowsFn pick_rows_mode(bool nt, bool xv) {
    if (nt) return xv ? qmatvec_kon_rows_kernel<R, DEPTH, true, true> : qmatvec_kon_rows_kernel<R, DEPTH, true, false>;
    return xv ? qmatvec_kon_rows_kernel<R, DEPTH, false, true> : qmatvec_kon_rows_kernel<R, DEPTH, false, false>;
}
// four items per lane in flight up to four rows, two above (the x pairs of a deeper pipeline no longer fit the registers)
RowsFn pick_rows(uint32_t M, bool nt, bool xv) {
    switch (M) {
        case 2: return pick_rows_mode<2, 4>(nt, xv);
        case 3: return pick_rows_mode<3, 4>(nt, xv);
        case 4: return pick_rows_mode<4, 4>(nt, xv);
        case 5: return pick_rows_mode<5, 2>(nt, xv);
        case 6: return pick_rows_mode<6, 2>(nt, xv);
        case 7: return pick_rows_mode<7, 2>(nt, xv);
        case 8: return pick_rows_mode<8, 2>(nt, xv);
        default: return nullptr;
    }
}

} // namespace

bool launch_qmatvec_kon_rows(hipStream_t s, const QWeightDev& w, const QMatmulParams& p) {
    if (w.format != QW_Q4K || p.M < 2 || p.M > kKonRowsMaxM || p.K != w.K || p.N != w.N || p.N % 16 != 0) return false;
    // waves: the M = 1 rule (kon_waves in qmatvec.hip: one wave per 64 k-pairs, 4 up to K = 6144, 8 above; ZGML_QMV_KON_WAVES overrides)
    const uint32_t P = (p.K + 1) / 2, wave_steps = cdiv(P, 64);
    const uint32_t cap = (uint32_t)std::max(1, std::min(8, sw().qmv_kon_waves > 0 ? sw().qmv_kon_waves : (p.K > 6144 ? 8 : 4)));
    const uint32_t waves = std::max(1u, std::min(wave_steps, cap));
    const bool xv = (uintptr_t)p.input % 8 == 0 && p.in_rs % 2 == 0 && p.K % 2 == 0;
    const RowsFn fn = pick_rows(p.M, w.stream_nt != 0, xv);
    const KonRowsArgs a{(const uint4*)w.qs, (const uint32_t*)w.sc, p.dst, p.input, p.in_rs, p.dst_rs, p.K, p.N / 16};
    hipLaunchKernelGGL(fn, dim3(p.N / 16), dim3(waves * 64), 0, s, a);
    return true;
}

} // namespace zgml
