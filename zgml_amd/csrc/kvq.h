// kvq.h — the column quantisation of the int8 KV cache (QuantizedKVCache.storeColumn, src/quant.zig:687-699 -> quantizeInput
// :320-341), stated once for host and device. Per block of `block` consecutive dims of a column:
//   mx = max|v|,  scale = mx > 0 ? mx / 127 : 1,  inv = mx > 0 ? 127 / mx : 0,  q = trunc(clamp(v * inv, -127, 127))
// (no FMA anywhere: one multiply, then the clamp; the conversion truncates toward zero). zgml_hip_kv_move's quantising form
// (kv_move.hip) calls it; kvq_store_kernel (kernels_generic.hip) and the fused store of attention_decode.h spell the same
// arithmetic out in their own lane layouts — unchanged, so their bytes cannot move — and tests hold the forms together
// (tests/test_hip_kv_move.py: device against device, to the bit; tests/test_batch_kvq_host.py: this header against the oracle). Plain C++ besides the host / device marks, so a CPU probe compiles it alone (tests/cpp/kvq_probe.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZGML_KVQ_HD __host__ __device__ __forceinline__
#else
#define ZGML_KVQ_HD inline
#endif

namespace zgml {

struct KvqScale {
    float scale; // what the cache stores for the block
    float inv;   // what the block's values are multiplied by
};
ZGML_KVQ_HD KvqScale kvq_block_scale(float max_abs) {
    return max_abs > 0.f ? KvqScale{max_abs / 127.0f, 127.0f / max_abs} : KvqScale{1.0f, 0.0f};
}
// The clamp is the reference's std.math.clamp, max(-127, min(x, 127)), whose min / max keep the operand that is a number. It only
// shows in one corner: a block whose maximum is below 127 / FLT_MAX (3.7e-37) has inv = +inf, so an exact zero in it gives
// 0 * inf = NaN, which this order turns into 127 as the reference and the oracle do. kvq_store_kernel and the fused store clamp
// in the other order (-127 for that NaN); every other input gives the same byte in either order.
ZGML_KVQ_HD int8_t kvq_quantise(float v, float inv) { return (int8_t)(int)fmaxf(-127.0f, fminf(v * inv, 127.0f)); }

// one whole column: d_head values -> d_head bytes and d_head / block scales
ZGML_KVQ_HD void kvq_quantise_column(const float* src, uint32_t d_head, uint32_t block, int8_t* q, float* scales) {
    for (uint32_t b = 0; b * block < d_head; b++) {
        float mx = 0.f;
        for (uint32_t i = 0; i < block; i++) mx = fmaxf(mx, fabsf(src[b * block + i]));
        const KvqScale s = kvq_block_scale(mx);
        scales[b] = s.scale;
        for (uint32_t i = 0; i < block; i++) q[b * block + i] = kvq_quantise(src[b * block + i], s.inv);
    }
}

} // namespace zgml
